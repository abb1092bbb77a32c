"""GPU: every camera's clock offset on the device (include/uu3d.h, ONE CLOCK; views.py).  The references are the rules in numpy
(tests/test_view_align_cpu.py pins them); every comparison is on the bits.
  1. predict.view_lag_sums / view_offsets equal their mirrors: views of 300 / 40 / 257 / 3 / 50 frames in one call (fewer frames than a
     workgroup has lanes, one frame past the 256-lane stride, a ragged second round), J in {5, 17}, max_lag in {1, 6} -- lags +-L, lags of
     partial overlap and, against the view of 3 frames, of no overlap --, a view of one track, an empty view, a coincident camera pair,
     flags, NaN joints and no flags; same_index on and off; M = 64 tracks of 8 frames; the inputs are unchanged afterwards
  2. align_views equals align_views_host with a distorted view, and two calls give the same bytes
  3. every guard of the C ABI returns its code and leaves the outputs alone
  4. predict_views(align=True) and align=[...] (h36m_81 at mask stride 4, seeded weights; 3 cameras, views of 34 / 30 / 36 frames) equal
     the call on the cropped views, with match None and True and with every option at once; a view that cannot be aligned is named
  5. predict_views(align=None) returns what it returned before"""
import ctypes as C

import numpy as np
import pytest

from tests import view_align_util as AU
from tests.test_distortion_cpu import SETS
from tests.test_distortion_gpu import _host, _same
from tests.tracks_util import _model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
MS, J17 = 4, 17
OFFSETS, LENGTHS = [0, 3, -2, 1, 0, -4], [300, 40, 257, 3, 50, 60]


def _bits(a, b):
    a, b = _host(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _both(predict, views, cams, valid, L, min_terms, same_index):
    """The two launches against the two mirrors, on the mirror's tables and on the device's -> the mirror's results."""
    kp, view_of, frames, flags = AU.stacked(views, valid)
    dk = torch.from_numpy(kp).cuda()
    df = None if flags is None else torch.from_numpy(flags).cuda()
    before = dk.clone()
    want_s, want_n = predict.view_lag_sums_host(kp, view_of, cams, frames, L, flags)
    got_s, got_n = predict.view_lag_sums(dk, view_of, cams, frames, L, df)
    assert got_s.dtype == torch.float64 and got_n.dtype == torch.int32
    assert _bits(got_n, want_n) and _bits(got_s, want_s), (L, same_index)
    want = predict.view_offsets_host(want_s, want_n, view_of, len(cams), L, min_terms, same_index)
    for s, n in ((torch.from_numpy(want_s).cuda(), torch.from_numpy(want_n).cuda()), (got_s, got_n)):
        got = predict.view_offsets(s, n, view_of, len(cams), L, min_terms, same_index)
        assert [g.dtype for g in got] == [torch.int32, torch.int32, torch.float64]
        assert all(_bits(g, w) for g, w in zip(got, want)), [(_host(g).tolist(), w.tolist()) for g, w in zip(got, want)]
    assert _same(dk, before)                                             # only read
    return want_s, want_n, want


# ---- 1. the two launches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 6])
@pytest.mark.parametrize("J", [5, 17])
def test_lag_sums_and_offsets_equal_the_mirrors(J, L):
    from uplift_upsample_3dhpe_amd import predict
    # views of (2, 2, 2, 1, 0, 2) shuffled tracks; camera 5 is camera 0 once more: no terms
    cams, views, _, valid = AU.scene(OFFSETS, LENGTHS, 2, J, 10 * J + L, counts=[2, 2, 2, 1, 0, 2])
    cams[5] = cams[0]
    for fl in (valid, None):
        sums, terms, (off, state, score) = _both(predict, views, cams, fl, L, 10, False)
        assert sums.shape == (2, 9, 2 * L + 1) and not terms[:, :2].any() and not terms[:, 7:].any() and terms[:, 2:7].any()
        assert state.tolist() == [1, 1, 1, 1, 1, 0]                      # the coincident camera cannot be aligned, the empty view need not be
        short = terms[:, 6]                                              # the view of 3 frames: g = f - l < 3
        assert not short[:, :max(0, L - 2)].any() and short[:, L:].all()
        if L == 6:
            assert off.tolist()[:3] == OFFSETS[:3]
    # the same counts in every non-empty view, the short reference first: same_index on and off
    cams, views, _, valid = AU.scene(OFFSETS[1:4], LENGTHS[1:3] + [300], 2, J, 20 * J + L)
    for same_index in (True, False):
        _, terms, (off, state, _) = _both(predict, views, cams, valid, L, 50, same_index)
        assert state.tolist() == [1, 1, 1] and terms[:, 2:].all()
        if L == 6:
            assert off.tolist() == [0, -5, -2]
    kp, view_of, frames, flags = AU.stacked(views, valid)
    dev = [torch.from_numpy(t).cuda() for tracks in views for t in tracks]
    lists = predict.view_lag_sums(dev, view_of, cams, None, L, [torch.from_numpy(f).cuda() for per in valid for f in per])
    flat = predict.view_lag_sums(torch.from_numpy(kp).cuda(), view_of, cams, frames, L, torch.from_numpy(flags).cuda())
    assert _same(lists[0], flat[0]) and _same(lists[1], flat[1])         # a list of tracks is their rows back to back
    with pytest.raises(ValueError):
        predict.view_lag_sums(torch.from_numpy(kp), view_of, cams, frames, L)                                      # a host tensor
    with pytest.raises(ValueError):
        predict.view_lag_sums(torch.from_numpy(kp).cuda(), view_of, cams, frames[:-1], L)
    with pytest.raises(ValueError):
        predict.view_offsets(flat[0], flat[1], view_of, 3, L + 1, 50)


def test_lag_sums_and_offsets_of_64_tracks():
    from uplift_upsample_3dhpe_amd import predict
    cams, views, _, valid = AU.scene([0, 1, -1, 2, -2, 3, -3, 0], [8] * 8, 8, 5, 77, lost=0.1)
    for same_index in (True, False):
        sums, terms, (off, state, _) = _both(predict, views, cams, valid, 6, 10, same_index)
        assert sums.shape == (8, 64, 13) and state.tolist() == [1] * 8 and terms[:, 8:].all() and off.tolist() == [0, 1, -1, 2, -2, 3, -3, 0]
    _both(predict, views, cams, None, 1, 1, False)


# ---- 2. align_views ------------------------------------------------------------------------------------------------------------------------
def test_align_views_equals_the_host_call_and_repeats():
    from uplift_upsample_3dhpe_amd import predict
    offsets, lengths = [0, 4, -3], [90, 70, 100]
    cams, views, _, valid = AU.scene(offsets, lengths, 2, J17, 61, distortion={1: SETS[0]})
    for kw in (dict(valid=valid, same_index=True), dict(valid="finite"), dict()):
        want = predict.align_views_host(views, cams, max_lag=6, min_terms=50, **kw)
        got = predict.align_views(views, cams, max_lag=6, min_terms=50, **kw)
        again = predict.align_views([[torch.from_numpy(t).cuda() for t in v] for v in views], cams, max_lag=6, min_terms=50, **kw)
        assert all(_bits(g, w) for g, w in zip(got, want)) and want[0].tolist() == offsets and want[1].tolist() == [1, 1, 1]
        assert all(_same(a, g) for a, g in zip(again, got))              # two calls, the same bytes
    with pytest.raises(ValueError):
        predict.align_views([views[0], views[1][:1], views[2]], cams, same_index=True)


# ---- 3. the guards -------------------------------------------------------------------------------------------------------------------------
def test_every_guard_returns_its_code_and_leaves_the_outputs_alone():
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    J, L, M, V = 5, 2, 3, 2
    kp = torch.zeros((30, J, 2), dtype=torch.float32, device="cuda")
    cams = torch.zeros((V, 16), dtype=torch.float64, device="cuda")
    scratch = torch.zeros((int(lib.uu3d_view_lag_scratch_bytes(30, J)) + 8,), dtype=torch.uint8, device="cuda")
    sums = torch.full((1, M, 2 * L + 1), -7.0, dtype=torch.float64, device="cuda")
    terms = torch.full((1, M, 2 * L + 1), -7, dtype=torch.int32, device="cuda")
    out = [torch.full((V,), -7, dtype=torch.int32, device="cuda"), torch.full((V,), -7, dtype=torch.int32, device="cuda"),
           torch.full((V,), -7.0, dtype=torch.float64, device="cuda")]
    assert lib.uu3d_view_lag_scratch_bytes(30, J) >= 30 * J * 25 and lib.uu3d_view_lag_scratch_bytes(0, J) == 0 and lib.uu3d_view_lag_scratch_bytes(30, 65) == 0
    i32, i64, p = (lambda a: (C.c_int32 * len(a))(*a)), (lambda a: (C.c_int64 * len(a))(*a)), (lambda t, o=0: C.c_void_p(t.data_ptr() + o))
    long_view, long_rows = [0] * 65, list(range(66))
    good = dict(kp=p(kp), flags=None, view_of=i32([0, 1, 1]), first=i64([0, 10, 20, 30]), tracks=M, J=J, views=V, cams=p(cams), L=L, scratch=p(scratch),
                sums=p(sums), terms=p(terms))
    lag_cases = [(dict(views=9), 2), (dict(tracks=65, view_of=i32(long_view), first=i64(long_rows)), 2), (dict(J=65), 2), (dict(L=513), 2),
                 (dict(L=0), 1), (dict(J=0), 1), (dict(tracks=0), 1), (dict(views=0), 1), (dict(view_of=i32([1, 0, 1])), 1), (dict(view_of=i32([0, 1, 2])), 1),
                 (dict(view_of=None), 1), (dict(first=None), 1), (dict(first=i64([0, 10, 10, 30])), 1), (dict(first=i64([0, 20, 10, 30])), 1),
                 (dict(first=i64([-1, 10, 20, 30])), 1), (dict(first=i64([0, 10, 20, 20 + 2 ** 31 // J + 1])), 1),
                 (dict(kp=None), 1), (dict(cams=None), 1), (dict(scratch=None), 1), (dict(sums=None), 1), (dict(terms=None), 1),
                 (dict(kp=p(kp, 4)), 1), (dict(scratch=p(scratch, 4)), 1), (dict(sums=p(sums, 4)), 1), (dict(terms=p(terms, 2)), 1), (dict(cams=p(cams, 4)), 1)]
    order = ("kp", "flags", "view_of", "first", "tracks", "J", "views", "cams", "L", "scratch", "sums", "terms")
    for change, code in lag_cases:
        args = dict(good)
        args.update(change)
        assert lib.uu3d_view_lag_sums(*[args[k] for k in order], None) == code, change
    good = dict(sums=p(sums), terms=p(terms), view_of=i32([0, 1, 1]), tracks=M, views=V, L=L, min_terms=1, same=0, offset=p(out[0]), state=p(out[1]),
                score=p(out[2]))
    off_cases = [(dict(views=9), 2), (dict(tracks=65, view_of=i32(long_view)), 2), (dict(L=513), 2), (dict(L=0), 1), (dict(min_terms=0), 1),
                 (dict(view_of=i32([1, 0, 1])), 1), (dict(view_of=None), 1), (dict(same=1), 1), (dict(sums=None), 1), (dict(terms=None), 1),
                 (dict(offset=None), 1), (dict(state=None), 1), (dict(score=None), 1), (dict(sums=p(sums, 4)), 1), (dict(terms=p(terms, 2)), 1),
                 (dict(offset=p(out[0], 2)), 1), (dict(state=p(out[1], 2)), 1), (dict(score=p(out[2], 4)), 1)]
    order = ("sums", "terms", "view_of", "tracks", "views", "L", "min_terms", "same", "offset", "state", "score")
    for change, code in off_cases:
        args = dict(good)
        args.update(change)
        assert lib.uu3d_view_offsets(*[args[k] for k in order], None) == code, change
    torch.cuda.synchronize()
    assert (sums == -7.0).all() and (terms == -7).all() and all((o == -7).all() for o in out) and not scratch.any()


# ---- 4. predict_views(align=...) -----------------------------------------------------------------------------------------------------------
VIEW_OFFSETS, VIEW_LENGTHS = [0, 3, -2], [34, 30, 36]                  # common times 3 .. 32: 30 frames


def _equal_results(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(g[0], (list, tuple)) and len(g[0]) and isinstance(g[0][0], torch.Tensor):        # the per-view world poses
            assert all(_same(torch.cat(a, 0), torch.cat(b, 0)) for a, b in zip(g, w))
        elif isinstance(g[0], torch.Tensor):
            assert [tuple(t.shape) for t in g] == [tuple(t.shape) for t in w] and _same(torch.cat(g, 0), torch.cat(w, 0))
        else:
            assert g == w                                                # the persons of match


@pytest.mark.parametrize("form", ["plain", "match", "all_options"])
def test_predict_views_with_align_equals_the_call_on_the_cropped_views(form):
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    full = form == "all_options"
    cams, views, truth, valid = AU.scene(VIEW_OFFSETS, VIEW_LENGTHS, 2, J17, 83, counts=[2, 2, 2] if form == "match" else None,
                                         distortion={1: SETS[0]} if full else None, lost=0.0 if form == "plain" else 0.04)
    if full:                                                             # flags given per joint: they name the NaN joints as well
        valid = [[(f * np.isfinite(t).all(axis=2)).astype(np.uint8) for f, t in zip(fv, tv)] for fv, tv in zip(valid, views)]
    kw = dict(resolutions=(1024, 1024), mask_stride=MS)
    if form == "match":
        kw.update(match=True, valid="finite")
    if full:
        kw.update(bones="track", smooth=True, rotations=True, fps=30, return_views=True)
    given = valid if full else kw.pop("valid", None)
    params = predict.AlignViews(max_lag=6, min_terms=50)
    host = predict.align_views_host(views, cams, given, 6, 50, same_index=form != "match")
    assert host[0].tolist() == VIEW_OFFSETS and host[1].tolist() == [1, 1, 1]
    cropped, kept, first = predict.crop_views(views, VIEW_OFFSETS, given)
    assert first == [3, 0, 5] and {len(t) for v in cropped for t in v} == {30}
    want = predict.predict_views(model, cfg, cropped, cams, valid=kept, **kw)
    for align in (params, VIEW_OFFSETS):
        got = predict.predict_views(model, cfg, views, cams, valid=given, align=align, **kw)
        assert got[-2] == VIEW_OFFSETS and got[-1] == first
        _equal_results(got[:-2], want)
    if form == "match":
        assert got[-3] == want[-1] and [len(p) for p in want[-1]] == [2, 2, 2] and truth[0] != truth[1]
    if form == "plain":
        shifted = predict.predict_views(model, cfg, views, cams, align=[1, 4, -1], **kw)            # the offsets count up to a common shift
        assert shifted[-1] == first and shifted[-2] == [1, 4, -1]
        _equal_results(shifted[:-2], want)
        gone = [views[0], [np.full_like(t, np.nan) for t in views[1]], views[2]]
        with pytest.raises(ValueError, match="view 1"):
            predict.predict_views(model, cfg, gone, cams, align=params, **kw)


# ---- 5. the unchanged call -----------------------------------------------------------------------------------------------------------------
def test_predict_views_without_align_returns_what_it_returned():
    from tests import views_util as VU
    from tests.test_views_gpu import LENS, _composition, _views
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    cams = VU.ring_cameras(2, 41)
    views = _views(cams, 43)
    kw = dict(resolutions=(1024, 1024), mask_stride=MS)
    want, world, _ = _composition(model, cfg, views, cams, kw, False)
    got = predict.predict_views(model, cfg, views, cams, align=None, **kw)
    assert len(got) == len(want) == 4
    for name, g, r in zip(("poses", "roots", "root_state", "view_count"), got, want):
        assert [int(t.shape[0]) for t in g] == LENS and _same(torch.cat(g, 0), r), name
