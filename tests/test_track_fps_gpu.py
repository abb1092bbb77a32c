"""GPU: predict.predict_tracks(fps=...) -- tracks at any frame rate -- and its kernel, uu3d_resample_tracks (csrc/uu3d_tracks.h).

The kernel's arithmetic is fixed (h36m.normalize_screen_coordinates per source frame, then two float64 products and one sum, each rounded,
stored as float32), so the pose table is compared BITWISE against that expression in numpy.  End to end, model frames that coincide with a
source frame are that frame's bits, hence the poses at those frames equal, bit for bit, the poses of the plain call on the host-resampled
track; all other frames carry an ulp bound that is derived where it is asserted."""
import functools

import numpy as np
import pytest

from tests import test_predict_tracks_gpu as base
from tests import util

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
RES, MASK_STRIDE = base.RES, base.MASK_STRIDE
LENS, RATES = [1, 2, 13, 40], [24, 30, 25, 60]


@functools.lru_cache(maxsize=None)
def _model(cfgname):
    return base._model(cfgname)


def _res(n):
    return [RES[i % len(RES)] for i in range(n)]


def _host_table(src, left, right, weight):
    """The kernel's expression on the (normalised) source rows ``src`` (R, J, 2) float32."""
    a, b = src[left].astype(np.float64), src[right].astype(np.float64)
    w = np.asarray(weight, np.float64)[:, None, None]
    with np.errstate(invalid="ignore"):
        mixed = (a * (1.0 - w) + b * w).astype(np.float32)
    return np.where((left == right)[:, None, None], src[left], mixed)


def _host_resampled(tracks, fps, normalise=True):
    """Per track: the table rows the kernel should write, from the host's normalisation of every source frame -> (list, plan)."""
    from uplift_upsample_3dhpe_amd import predict
    lens = [len(t) for t in tracks]
    plan = predict.resample_plan(lens, fps)
    src = np.concatenate(base._host_normalised(tracks) if normalise else tracks, 0)
    table = _host_table(src, *plan[1:])
    return np.split(table, np.cumsum(plan[0])[:-1]), plan


@pytest.mark.parametrize("lens,fps", [(LENS, RATES), (LENS[2:], RATES[:2]), (LENS, (30000, 1001)), (LENS[2:], (30000, 1001))],
                         ids=["4tracks-mixed", "2tracks-mixed", "4tracks-ntsc", "2tracks-ntsc"])
def test_resample_tracks_equals_the_host_expression_bitwise(lens, fps):
    from uplift_upsample_3dhpe_amd import predict
    tracks = base._pixel_tracks(lens, seed=21)
    want, (model_lens, left, right, weight) = _host_resampled(tracks, fps)
    want = np.concatenate(want, 0)
    assert (left != right).sum() > 10 and (left == right).sum() > 2
    table, got_lens, src_lens = predict.resampled_pose_table(tracks, "cuda", fps, resolutions=_res(len(lens)))
    assert list(got_lens) == list(model_lens) and list(src_lens) == lens and table.valid is None
    assert tuple(table.kp2d.shape) == (int(model_lens.sum()), 17, 2) and base._same_bits(table.kp2d, want)
    # device input: the caller's tensors are not written; a second call gives the same bits
    dev_tracks = [torch.from_numpy(t).cuda() for t in tracks]
    table2, _, _ = predict.resampled_pose_table(dev_tracks, "cuda", fps, resolutions=_res(len(lens)))
    assert base._same_bits(table2.kp2d, want) and all(base._same_bits(d, t) for d, t in zip(dev_tracks, tracks))
    # res = None: the coordinates are taken as they are
    raw, _ = _host_resampled(tracks, fps, normalise=False)
    table3, _, _ = predict.resampled_pose_table(dev_tracks, "cuda", fps)
    assert base._same_bits(table3.kp2d, np.concatenate(raw, 0)) and all(base._same_bits(d, t) for d, t in zip(dev_tracks, tracks))
    # a plan row out of range gives NaN in that row only, never a read out of bounds
    src = torch.cat(dev_tracks, 0)
    bad_l, bad_r = left.copy(), right.copy()
    rows = len(left)
    hit = sorted({0, rows // 2, rows - 1})
    bad_l[hit[0]] = len(src)
    bad_r[hit[-1]] = -1
    bad_l[hit[len(hit) // 2]] = np.iinfo(np.int64).max
    out = torch.empty((rows, 17, 2), dtype=torch.float32, device="cuda")
    predict.resample_tracks(src, out, model_lens, bad_l, bad_r, weight, np.asarray(_res(len(lens)), np.float64))
    out = out.cpu().numpy()
    assert np.isnan(out[hit]).all() and base._same_bits(np.delete(out, hit, 0), np.delete(want, hit, 0))


def test_both_store_widths_are_covered():
    """The cases above leave an even and an odd number of (x, y) pairs: with and without the 8-byte tail behind the 16-byte stores."""
    from uplift_upsample_3dhpe_amd import predict
    parity = {int(predict.resample_plan(l, f)[0].sum()) * 17 % 2 for l, f in [(LENS, RATES), (LENS[2:], RATES[:2])]}
    assert parity == {0, 1}


def test_missing_source_frames_on_the_model_grid():
    from uplift_upsample_3dhpe_amd import predict
    lens, fps = LENS[2:], RATES[:2]                                    # 13 frames at 24 fps, 40 at 30 fps
    clean = base._pixel_tracks(lens, seed=22)
    want, (model_lens, left, right, weight) = _host_resampled(clean, fps)
    want = np.concatenate(want, 0)
    s = lens[0] + 4                                                    # frame 4 of the 30 fps track: between the exact frames 3 and 6
    tracks = [t.copy() for t in clean]
    tracks[1][4, 9, 1] = np.nan
    missing = (left == s) | (right == s)                               # right == s implies weight > 0: weight 0 has right == left
    k5 = int(model_lens[0]) + 5                                        # model frame 5 of that track IS source frame 3; its right neighbour is s
    assert left[k5] == right[k5] == s - 1 and weight[k5] == 0 and not missing[k5] and 2 <= missing.sum() <= 4
    expect = np.where(missing[:, None, None], np.float32(0), want)
    for valid in ("finite", [np.ones(13, bool), np.arange(40) != 4]):
        given = tracks if isinstance(valid, str) else clean             # the list form marks the same frame without a NaN in it
        table, _, _ = predict.resampled_pose_table(given, "cuda", fps, resolutions=_res(2), valid=valid)
        assert table.valid.dtype == torch.uint8 and np.array_equal(table.valid.cpu().numpy() != 0, ~missing)
        assert base._same_bits(table.kp2d, expect)                     # zeros in the missing rows, every other row keeps its bits
    # without validity the NaN reaches exactly those rows -- and not the integral-position frame whose unread right neighbour it is
    table, _, _ = predict.resampled_pose_table(tracks, "cuda", fps, resolutions=_res(2))
    got = table.kp2d.cpu().numpy()
    assert np.array_equal(np.isnan(got).any(axis=(1, 2)), missing) and base._same_bits(got[~missing], want[~missing])
    # a model frame behind the last source frame repeats it (left == right): the frame before it is not read
    tail = base._pixel_tracks([12], seed=27)                          # 12 frames at 24 fps: model frame 23 sits at 11.04
    want, (model_lens, left, right, weight) = _host_resampled(tail, 24)
    assert model_lens[0] == 24 and left[23] == right[23] == 11 and left[22] == 10 and right[22] == 11
    tail[0][10] = np.nan
    table, _, _ = predict.resampled_pose_table(tail, "cuda", 24, resolutions=_res(1), valid="finite")
    assert np.array_equal(table.valid.cpu().numpy() != 0, ~((left == 10) | (right == 10))) and bool(table.valid[23] != 0)
    assert base._same_bits(table.kp2d[23], want[0][23])


def _bracket(R, num, den):
    """R (T', J, 3) at the positions num / den, linear between the two bracketing frames in float64."""
    p = num // den
    fr = ((num - p * den) / den)[:, None, None]
    a, b = R[p].astype(np.float64), R[np.minimum(p + 1, len(R) - 1)].astype(np.float64)
    return a * (1.0 - fr) + b * fr


@pytest.mark.parametrize("cfgname,fps,src_step,model_step", [("h36m_351", 30, 3, 5), ("h36m_81", 25, 1, 2)])
def test_exact_at_coinciding_frames_end_to_end(cfgname, fps, src_step, model_step):
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model(cfgname)
    ms = MASK_STRIDE[cfgname]
    lens = [61, 200]
    tracks = base._pixel_tracks(lens, seed=23)
    kw = dict(resolutions=_res(2), mask_stride=ms, root_relative=False)
    # fps = 50 is the call without fps, bit for bit
    plain = predict.predict_tracks(model, cfg, tracks, **kw)
    same = predict.predict_tracks(model, cfg, tracks, fps=50, **kw)
    assert all(base._same_bits(a, b) for a, b in zip(plain, same))
    # R: the plain call on the track resampled to 50 Hz by the host
    resampled, (model_lens, _, _, _) = _host_resampled(tracks, fps)
    R = predict.predict_tracks(model, cfg, resampled, mask_stride=ms, root_relative=False)
    got = predict.predict_tracks(model, cfg, tracks, fps=fps, **kw)
    assert [tuple(g.shape) for g in got] == [(n, 17, 3) for n in lens] and [len(r) for r in R] == list(model_lens)
    for g, r, n in zip(got, R, lens):
        g, r = g.cpu().numpy(), r.cpu().numpy()
        i = np.arange(0, n, src_step)
        assert base._same_bits(g[i], r[i // src_step * model_step])    # source frame src_step m IS model frame model_step m
        # the others: the direct plan rounds once to float32; the two-step route rounds R's two frames (0.5 ulp each) and nothing more in
        # float64 -- at most 1.5 ulp apart at the track's largest coordinate, the bound of 4 leaves more than a factor of two
        every = np.arange(n)
        want = _bracket(r, every * 50, np.full(n, fps))
        ulp = float(np.spacing(np.float32(np.abs(r).max())))
        err = float(np.abs(g.astype(np.float64) - want).max()) / ulp
        print(f"{cfgname} fps {fps}, {n} frames: direct vs two-step {err:.2f} ulp (bound 4)")
        assert err <= 4.0


def test_root_relative_out_fps_and_flags_on_the_model_grid():
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    ms, root = MASK_STRIDE["h36m_81"], cfg.ROOT_KEYTPOINT
    lens = [60, 23]
    tracks = base._pixel_tracks(lens, seed=24)
    kw = dict(resolutions=_res(2), mask_stride=ms)
    un = predict.predict_tracks(model, cfg, tracks, fps=20, root_relative=False, **kw)
    rel = predict.predict_tracks(model, cfg, tracks, fps=20, **kw)
    for u, r in zip(un, rel):
        u, r = u.cpu().numpy(), r.cpu().numpy()
        assert not r[:, root].any() and base._same_bits(r, u - u[:, root:root + 1])
    # the detector ran on every third frame of a 60 fps video: 3 (T - 1) + 1 poses, every third is the 20 fps call's
    dense = predict.predict_tracks(model, cfg, tracks, fps=20, out_fps=60, **kw)
    assert [len(d) for d in dense] == [3 * (n - 1) + 1 for n in lens]
    assert all(base._same_bits(d[::3], r) for d, r in zip(dense, rel)) and all(bool(torch.isfinite(d).all()) for d in dense)
    # return_valid with fps: the flags of the model's frames, (T'_i,)
    holes = [t.copy() for t in tracks]
    holes[0][7] = np.nan
    poses, flags = predict.predict_tracks(model, cfg, holes, fps=25, valid="finite", return_valid=True, **kw)
    model_lens, left, right, _ = predict.resample_plan(lens, 25)
    assert [tuple(f.shape) for f in flags] == [(int(n),) for n in model_lens] and all(f.dtype == torch.bool for f in flags)
    assert np.array_equal(torch.cat(flags).cpu().numpy(), ~((left == 7) | (right == 7)))
    assert [len(p) for p in poses] == lens and all(bool(torch.isfinite(p).all()) for p in poses)
    with pytest.raises(ValueError, match="out_fps"):
        predict.predict_tracks(model, cfg, [t[::ms] for t in tracks], fps=25, keyframes_only=True, lengths=lens, **kw)


def test_fps_24_against_the_oracle():
    """24 fps is the one common rate whose keyframes are interpolated on the input side.  The oracle pipeline of test_predict_tracks_gpu on the
    host-resampled track, then the output read at the source frames' times on the host; the bar is that test's own (util.TOL_MAX_ABS)."""
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    ms = MASK_STRIDE["h36m_81"]
    n = 50
    tracks = base._pixel_tracks([n], seed=25)
    resampled, (model_lens, left, right, weight) = _host_resampled(tracks, 24)
    assert (weight[::ms] > 0).sum() > 10                               # keyframes that are mixed from two source frames
    dense = base._oracle_tracks(cfg, arch, w, resampled, ms)           # (T', J, 3) float64, root-relative
    want = _bracket(dense, np.arange(n) * 50, np.full(n, 24))
    got = predict.predict_tracks(model, cfg, tracks, resolutions=_res(1), mask_stride=ms, flip=True, fps=24)
    assert len(got) == 1 and tuple(got[0].shape) == (n, 17, 3)
    err = float(np.abs(got[0].cpu().numpy() - want).max())
    print(f"h36m_81 at 24 fps: predict_tracks vs oracle pipeline max-abs {err:.3e} (bar {util.TOL_MAX_ABS})")
    assert err <= util.TOL_MAX_ABS


def test_the_resampling_front_never_waits_for_the_device():
    from uplift_upsample_3dhpe_amd import predict
    lens = [50, 64]
    tracks = [torch.from_numpy(t).cuda() for t in base._pixel_tracks(lens, seed=26)]
    flags = [torch.ones(n, dtype=torch.uint8, device="cuda") for n in lens]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        table, model_lens, _ = predict.resampled_pose_table(tracks, "cuda", [30, (30000, 1001)], resolutions=RES[:2])
        tablev, _, _ = predict.resampled_pose_table(tracks, "cuda", 29.97, resolutions=RES[:2], valid=flags)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert tuple(table.kp2d.shape) == (int(model_lens.sum()), 17, 2) and bool(torch.isfinite(table.kp2d).all())
    assert bool(tablev.valid.all()) and bool(torch.isfinite(tablev.kp2d).all())
