"""GPU: per-joint missed detections -- uu3d_repair_joints (csrc/uu3d_repair.h) and predict.predict_tracks(valid=..., repair_joints=G)
(include/uu3d.h, PER-JOINT MISSED DETECTIONS).  The reference is predict.repair_joints_host, the rule in numpy; every comparison is exact.
The scan of the plan kernel works on chunks of 256 frames: tracks of 255, 256, 257 and 600 frames are the smallest that end just before,
on and just behind a chunk boundary and that carry across two of them."""
import numpy as np
import pytest

from tests.tracks_util import RES, _model, _pixel_tracks, _same_bits

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
C = 256                                                                 # kRepairChunk
LENS = [1, 2, 7, C - 1, C, C + 1, 2 * C + 88]
MS = 4                                                                  # h36m_81


def _runs(T, n):
    """Unobserved runs of n frames at the start, in the interior and at the end of a track of T frames, where they fit."""
    f = np.ones(T, bool)
    if 3 * n + 8 <= T:
        f[:n] = False
        f[T // 2:T // 2 + n] = False
        f[T - n:] = False
    return f


def _patterns(lens, J, G, seed):
    """Per track (T, J) flags: joint 0 all observed, 1 never observed in the tracks of 2, 255 and 257 frames, 2 a run over the chunk boundary (frames C - 6 .. C + 6), 3 runs of
    G, 4 runs of G + 1, the others 30 % random; frame 3 of the 7- and 257-frame tracks has no observed joint at all."""
    rng = np.random.default_rng(seed)
    flags = []
    for T in lens:
        f = rng.random((T, J)) >= 0.3
        f[:, 0] = True
        if T in (2, C - 1, C + 1):
            f[:, 1] = False
        f[:, 2] = True
        f[C - 6:C + 7, 2] = False
        f[:, 3] = _runs(T, G)
        f[:, 4] = _runs(T, G + 1)
        if T in (7, C + 1):
            f[3, :] = False
        flags.append(f)
    return flags


def _poison(tracks, flags, observed_nan=True):
    """NaN, +Inf and 1e30 in the coordinates of unobserved joints (every fourth one keeps its finite value) and, with ``observed_nan``, NaN
    in ONE coordinate of a few joints whose flag is set (joints 5 and up: the random ones): those are unobserved by the finite test."""
    out = []
    for t, f in zip(tracks, flags):
        t = t.copy()
        idx = np.argwhere(~f)
        for k, (r, j) in enumerate(idx):
            if k % 4 < 3:
                t[r, j, k % 2] = (np.nan, np.inf, 1e30)[k % 4]
        on = np.argwhere(f)
        for r, j in on[on[:, 1] >= 5][::37] if observed_nan else ():
            t[r, j, 1] = np.nan
        out.append(t)
    return out


def _device_repair(tracks, flags, G):
    from uplift_upsample_3dhpe_amd import predict
    lens = [len(t) for t in tracks]
    host = np.concatenate(tracks, 0)
    src = torch.from_numpy(host).cuda()
    jf = None if flags is None else torch.from_numpy(np.concatenate(flags, 0).view(np.uint8)).cuda()
    first = predict.repair_joints(src, lens, G, jf)
    again = predict.repair_joints(src, lens, G, jf)
    assert all(np.array_equal(a.cpu().numpy().view(np.uint8).reshape(-1), b.cpu().numpy().view(np.uint8).reshape(-1)) for a, b in zip(first, again))
    assert _same_bits(src, host)                                        # the caller's tensor is only read
    assert first[0].data_ptr() != src.data_ptr()
    return first


@pytest.mark.parametrize("J,G", [(17, 1), (17, 3), (17, 1000), (5, 3), (128, 3)])
def test_kernel_equals_the_host_mirror_bitwise(J, G):
    from uplift_upsample_3dhpe_amd import predict
    flags = _patterns(LENS, J, G, seed=3)
    tracks = _poison(_pixel_tracks(LENS, seed=11, J=J), flags)
    with np.errstate(invalid="ignore", over="ignore"):
        want, want_frames, want_state = predict.repair_joints_host(tracks, flags, G)
    out, frames, state = _device_repair(tracks, flags, G)
    assert out.dtype == torch.float32 and frames.dtype == torch.uint8 and state.dtype == torch.uint8
    st = np.concatenate(want_state, 0)
    assert np.array_equal(state.cpu().numpy(), st)
    assert np.array_equal(frames.cpu().numpy(), np.concatenate(want_frames).astype(np.uint8))
    assert _same_bits(out, np.concatenate(want, 0))
    assert bool(torch.isfinite(out).all())
    # the patterns did what they were made for: every state occurs, the boundary run is filled exactly when G covers its 13 frames
    assert {0, 1, 2} <= set(np.unique(st))
    big = np.concatenate(want_state[-1:], 0)
    assert (big[C - 6:C + 7, 2] == (2 if G >= 13 else 0)).all() and (big[:, 0] == 1).all()
    assert (want_state[-2][:, 1] == 0).all() and not want_frames[-2].any()   # never observed: every frame of that track is missing
    assert 0 < np.concatenate(want_frames).sum() < sum(LENS)
    if 3 * (G + 1) + 8 <= LENS[-1]:
        assert (big[:G, 3] == 2).all() and (big[LENS[-1] // 2:LENS[-1] // 2 + G, 3] == 2).all() and (big[-G:, 3] == 2).all()
        assert (big[LENS[-1] // 2:LENS[-1] // 2 + G + 1, 4] == 0).all()                 # G + 1 between two observations: nothing is filled
        assert big[0, 4] == 0 and (big[1:G + 1, 4] == 2).all() and big[-1, 4] == 0 and (big[-G - 1:-1, 4] == 2).all()   # held up to G frames
    # no flags: the finite test alone
    with np.errstate(invalid="ignore", over="ignore"):
        want, want_frames, want_state = predict.repair_joints_host(tracks, None, G)
    out, frames, state = _device_repair(tracks, None, G)
    assert np.array_equal(state.cpu().numpy(), np.concatenate(want_state, 0))
    assert np.array_equal(frames.cpu().numpy(), np.concatenate(want_frames).astype(np.uint8))
    assert _same_bits(out, np.concatenate(want, 0))


def test_rows_no_track_covers_give_nan_not_a_read_out_of_bounds():
    """The plan launch writes the scratch of the rows track_start covers; whatever the rest of the scratch holds, an unobserved joint there
    comes out NaN with state 0 and its frame missing.  A track end behind the last row is clamped."""
    import ctypes as ct
    from uplift_upsample_3dhpe_amd import _capi, predict
    lib = _capi.load_library()
    J, rows, covered = 17, 20, 7
    track = _pixel_tracks([rows], seed=2)[0]
    flags = np.random.default_rng(2).random((rows, J)) >= 0.3
    flags[:, 0] = True
    src, jf = torch.from_numpy(track).cuda(), torch.from_numpy(flags.view(np.uint8)).cuda()
    want, want_frames, want_state = predict.repair_joints_host([track[:covered]], [flags[:covered]], 3)
    p = lambda t: ct.c_void_p(t.data_ptr())
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    for junk in (0x7F7F7F7F, -5, 3, 12):                                # no row; below -1; a row, but not on both sides of any frame
        start = torch.tensor([0, covered], dtype=torch.int64, device="cuda")
        scratch = torch.full((2 * rows * J,), junk, dtype=torch.int32, device="cuda")
        out, frames, state = torch.full((rows, J, 2), 7.0, device="cuda"), torch.full((rows,), 9, dtype=torch.uint8, device="cuda"), \
            torch.full((rows, J), 9, dtype=torch.uint8, device="cuda")
        _capi.check(lib, lib.uu3d_repair_joints(p(src), rows, J, p(jf), p(start), 1, 3, p(out), p(frames), p(state), p(scratch), scratch.numel() * 4, stream))
        o, f, s_ = out.cpu().numpy(), frames.cpu().numpy(), state.cpu().numpy()
        assert _same_bits(o[:covered], want[0]) and np.array_equal(s_[:covered], want_state[0]) and np.array_equal(f[:covered], want_frames[0])
        rest = flags[covered:]
        assert np.array_equal(s_[covered:], rest.astype(np.uint8)), junk
        assert _same_bits(o[covered:][rest], track[covered:][rest]) and np.isnan(o[covered:][~rest]).all(), junk
        assert np.array_equal(f[covered:], rest.all(axis=1).astype(np.uint8)), junk
    start = torch.tensor([0, 1000], dtype=torch.int64, device="cuda")
    scratch = torch.zeros((2 * rows * J,), dtype=torch.int32, device="cuda")
    _capi.check(lib, lib.uu3d_repair_joints(p(src), rows, J, p(jf), p(start), 1, 3, p(out), p(frames), p(state), p(scratch), scratch.numel() * 4, stream))
    want, want_frames, want_state = predict.repair_joints_host([track], [flags], 3)
    assert _same_bits(out, want[0]) and np.array_equal(state.cpu().numpy(), want_state[0])


# ---- end to end: h36m_81, tracks of 50 and 203 frames, flip ----------------------------------------------------------------------------
E2E_LENS = [50, 203]


def _e2e_case(seed=5):
    """(tracks with NaN / 1e30 in unobserved joints, clean tracks, (T, J) flags): 15 % of the joints lost at random, a run of 3 and a run of
    4 frames of one joint, one frame where nobody was found."""
    rng = np.random.default_rng(seed)
    clean = _pixel_tracks(E2E_LENS, seed=seed)
    flags = [rng.random((n, 17)) >= 0.15 for n in E2E_LENS]
    for f in flags:
        f[8:11, 9] = False
        f[8:11, [8, 10]] = True
        f[20:24, 13] = False
        f[19, 13] = f[24, 13] = True
        f[30, :] = False
    return _poison(clean, flags, observed_nan=False), clean, flags


@pytest.fixture(scope="module")
def e2e():
    from uplift_upsample_3dhpe_amd import predict
    tracks, clean, flags = _e2e_case()
    with np.errstate(invalid="ignore", over="ignore"):
        rep, fr, st = predict.repair_joints_host(tracks, flags, 3)
    assert all((~f).any() and f.any() for f in fr) and all((s == 2).any() and (s == 0).any() for s in st)
    return dict(tracks=tracks, clean=clean, flags=flags, repaired=rep, frame_flags=fr, state=st)


def _run(tracks, **kw):
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    return predict.predict_tracks(model, cfg, tracks, resolutions=RES[:len(tracks)], mask_stride=MS, flip=True, **kw)


@pytest.mark.parametrize("how", ["plain", "fps30", "keyframes_only"])
def test_predict_tracks_equals_the_call_on_host_repaired_tracks_bitwise(e2e, how):
    cut = (lambda a: a[::MS]) if how == "keyframes_only" else (lambda a: a)
    kw = {"plain": {}, "fps30": {"fps": 30}, "keyframes_only": {"keyframes_only": True, "lengths": E2E_LENS}}[how]
    tracks, flags = [cut(t) for t in e2e["tracks"]], [cut(f) for f in e2e["flags"]]
    if how == "keyframes_only":                                         # rows are the given keyframes: the mirror runs on them
        from uplift_upsample_3dhpe_amd import predict
        with np.errstate(invalid="ignore", over="ignore"):
            rep, fr, st = predict.repair_joints_host(tracks, flags, 3)
    else:
        rep, fr, st = e2e["repaired"], e2e["frame_flags"], e2e["state"]
    got, got_flags, got_state = _run(tracks, valid=flags, repair_joints=3, return_valid=True, **kw)
    want, want_flags = _run(rep, valid=fr, return_valid=True, **kw)
    assert len(got) == len(want) == 2 and all(_same_bits(g, w) for g, w in zip(got, want))
    assert all(np.array_equal(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(got_flags, want_flags))
    assert all(s.is_cuda and s.dtype == torch.uint8 and np.array_equal(s.cpu().numpy(), h) for s, h in zip(got_state, st))
    assert all(bool(torch.isfinite(g).all()) for g in got)
    # the repair matters: giving up every frame with a lost joint gives other poses
    dropped = _run(tracks, valid=flags, **kw)
    assert not all(_same_bits(g, d) for g, d in zip(got, dropped))


def test_invariants(e2e):
    tracks, clean, flags = e2e["tracks"], e2e["clean"], e2e["flags"]
    # per-frame flags: nothing to fill, the bits of the call without repair_joints
    per_frame = [f.all(axis=1) for f in flags]
    assert all(_same_bits(a, b) for a, b in zip(_run(clean, valid=per_frame, repair_joints=3), _run(clean, valid=per_frame)))
    # whatever the coordinates of an unobserved joint are, they change no bit
    base = _run(tracks, valid=flags, repair_joints=3)
    for junk in (np.nan, 1e30):
        other = [np.where(f[:, :, None], t, np.float32(junk)).astype(np.float32) for t, f in zip(clean, flags)]
        assert all(_same_bits(a, b) for a, b in zip(base, _run(other, valid=flags, repair_joints=3))), junk
    # host and device flags, mixed in one list, are the same call
    mixed = [torch.from_numpy(flags[0]).cuda(), flags[1]]
    assert all(_same_bits(a, b) for a, b in zip(base, _run([torch.from_numpy(tracks[0]).cuda(), tracks[1]], valid=mixed, repair_joints=3)))
    # "finite": the finite test per joint
    nan_tracks = [np.where(f[:, :, None], t, np.float32(np.nan)).astype(np.float32) for t, f in zip(clean, flags)]
    assert all(_same_bits(a, b) for a, b in zip(base, _run(nan_tracks, valid="finite", repair_joints=3)))
    # repair_joints=None with per-joint flags is today's path on the flags reduced per frame
    got, got_flags = _run(clean, valid=flags, return_valid=True)
    want, want_flags = _run(clean, valid=per_frame, return_valid=True)
    assert all(_same_bits(a, b) for a, b in zip(got, want))
    assert all(np.array_equal(a.cpu().numpy(), b.cpu().numpy()) and np.array_equal(a.cpu().numpy(), p) for a, b, p in zip(got_flags, want_flags, per_frame))
