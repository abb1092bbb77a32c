"""GPU: missed detections -- frame validity in predict.predict_tracks and stream.StreamSession (include/uu3d.h, MISSED DETECTIONS).

The rule: token n of a window reads source frame src (its own frame, or under copy padding the nearest sampled in-range frame); with a
validity table its stride-mask bit becomes  sm' = sm && (!have || valid[video_start + src]).  ``_np_windows`` below restates it in numpy
(``eval.window_frames``' index arithmetic plus the AND); the kernels are compared with it exactly.  Tracks of 1, 7, 50 and 203 frames:
shorter than a window, a window reaching past both ends, and 4k, 4k + 1, 4k + 3 frames for the edge rule of h36m_81 (N = 41, S = 2, copy
padding, s_in = 4 > S)."""
import ctypes as C

import numpy as np
import pytest

from tests import tracks_util, util
from tests.tracks_util import RES, _bits, _host_normalised, _model, _pixel_tracks, _same_bits

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
MASK_STRIDE = {"h36m_351": 5, "h36m_81": 4}
LENS = [1, 7, 50, 203]
PATTERNS = ("all_valid", "all_missing", "first_missing", "edge_missing", "random30")


def _pattern(name, L, S, seed=0):
    v = np.ones(L, bool)
    if name == "all_missing":
        v[:] = False
    elif name == "first_missing":
        v[0] = False
    elif name == "edge_missing":
        v[(L - 1) // S * S] = False                                     # the newest multiple of SEQUENCE_STRIDE: what copy padding repeats
    elif name == "random30":
        v = np.random.default_rng(seed).random(L) >= 0.3
    return v


# ---- the numpy restatement of the rule ---------------------------------------------------------------------------------------------
def _np_windows(desc, N, starts, lens, pad_edge, valid):
    """(W, 6) descriptors -> (src, inside, have, sm'), each (W, N): window_frame of csrc/uu3d_misc.h plus the validity AND.  ``valid``:
    (F,) flags indexed like the pose table, or None."""
    d = np.asarray(desc, np.int64).reshape(-1, 6)
    v, c, s, ms, sh = (d[:, k:k + 1] for k in range(5))
    n = np.arange(N, dtype=np.int64)[None, :]
    f = c - ((N - 1) * s) // 2 + n * s
    ln = np.asarray(lens, np.int64)[v]
    src = np.where(f < 0, f + ((-f + s - 1) // s) * s, np.where(f >= ln, f - ((f - ln + s) // s) * s, f))
    inside = (f >= 0) & (f < ln)
    have = inside | (bool(pad_edge) & (src >= 0) & (src < ln))
    sm = np.mod((n - N // 2) * s + sh, ms) == 0
    if valid is not None:
        g = np.asarray(starts, np.int64)[v] + np.clip(src, 0, ln - 1)
        sm = sm & (~have | (np.asarray(valid).reshape(-1)[g] != 0))
    return src, inside, have, sm


def _np_gather(table, desc, N, starts, lens, pad_edge, zero_masked, valid, order):
    """uu3d_gather_windows_valid: (out (W, N, J, 2), stride_mask, pad_mask)."""
    src, inside, have, sm = _np_windows(desc, N, starts, lens, pad_edge, valid)
    d = np.asarray(desc, np.int64).reshape(-1, 6)
    g = np.asarray(starts, np.int64)[d[:, :1]] + np.where(have, src, 0)
    out = table[g]                                                      # (W, N, J, 2)
    fl = d[:, 5] != 0
    out[fl] = out[fl][:, :, np.asarray(order)]
    out[fl, :, :, 0] = -out[fl, :, :, 0]
    keep = have & (sm | (not zero_masked))
    out = np.where(keep[:, :, None, None], out, np.float32(0.0))
    flip_zero = (~keep) & fl[:, None]                                   # (the kernel negates x of a flipped window after the select: -0.0)
    out[..., 0] = np.where(flip_zero[:, :, None], np.float32(-0.0), out[..., 0])
    return out.astype(np.float32), sm.astype(np.uint8), inside.astype(np.uint8)


def _np_rows(desc, N, starts, lens, pad_edge, zero_masked, valid, frame_base, zero_row):
    """uu3d_gather_window_frames_valid: (rows, stride_mask, pad_mask)."""
    src, inside, have, sm = _np_windows(desc, N, starts, lens, pad_edge, valid)
    d = np.asarray(desc, np.int64).reshape(-1, 6)
    r = np.asarray(starts, np.int64)[d[:, :1]] + src + np.where(d[:, 5:6] != 0, frame_base, 0)
    r = np.where(have, r, zero_row)
    if zero_masked:
        r = np.where(sm, r, -1)
    return r.astype(np.int32), sm.astype(np.uint8), inside.astype(np.uint8)


def _descriptors(cfg, lens, ms, flip):
    """One window per frame eval.needed_windows keeps, the stride mask aligned globally -- plain, then (``flip``) the mirrored twins."""
    S = cfg.SEQUENCE_STRIDE
    rows = [(v, c, S, ms, c, 0) for v, n in enumerate(lens) for c in range(0, n, S)]
    d = np.array(rows, np.int32)
    if flip:
        f = d.copy(); f[:, 5] = 1
        d = np.concatenate([d, f], 0)
    return d


# ---- 1. the front kernel -------------------------------------------------------------------------------------------------------------
def _broken_tracks(lens, seed):
    """Pixel tracks with a NaN in ONE coordinate of one joint, a +Inf, and a finite frame the caller's flags call missing -> (tracks,
    the caller's flags per track, the effective flags per track)."""
    tracks = _pixel_tracks(lens, seed)
    given = [np.ones(n, bool) for n in lens]
    tracks[1][3, 5, 1] = np.nan
    tracks[1][17, 0, 0] = np.inf
    tracks[0][12, 16, 0] = -np.inf
    given[1][8] = False
    given[0][0] = False
    eff = [g & np.isfinite(t).reshape(len(t), -1).all(1) for g, t in zip(given, tracks)]
    return tracks, given, eff


def test_normalize_tracks_valid_flags_and_zeroes_missing_frames():
    from uplift_upsample_3dhpe_amd import predict
    lens = [13, 40, 1]
    tracks, given, eff = _broken_tracks(lens, seed=1)
    res = [RES[i % len(RES)] for i in range(len(lens))]
    flags = np.concatenate(eff)
    assert flags.sum() == len(flags) - 5
    with np.errstate(invalid="ignore"):
        want = np.concatenate(_host_normalised(tracks), 0)
    want[~flags] = 0.0
    src = torch.from_numpy(np.concatenate(tracks, 0)).cuda()
    vin = torch.from_numpy(np.concatenate(given).view(np.uint8)).cuda()
    # a fresh table; the caller's flags ANDed with the finite test
    table, vout = torch.full_like(src, 7.0), torch.full((len(flags),), 9, dtype=torch.uint8, device="cuda")
    predict.normalize_tracks(src, table, lens, res, valid_in=vin, valid_out=vout)
    assert np.array_equal(vout.cpu().numpy(), flags.astype(np.uint8)) and _same_bits(table, want)
    assert _same_bits(src, np.concatenate(tracks, 0))                   # the source is not written
    # no flags from the caller: the finite test alone
    fin = np.concatenate([np.isfinite(t).reshape(len(t), -1).all(1) for t in tracks])
    with np.errstate(invalid="ignore"):
        want_fin = np.concatenate(_host_normalised(tracks), 0)
    want_fin[~fin] = 0.0
    predict.normalize_tracks(src, table, lens, res, valid_out=vout)
    assert np.array_equal(vout.cpu().numpy(), fin.astype(np.uint8)) and _same_bits(table, want_fin)
    # no resolution: the valid rows are copied bit for bit
    raw = np.concatenate(tracks, 0).copy(); raw[~flags] = 0.0
    predict.normalize_tracks(src, table, lens, None, valid_in=vin, valid_out=vout)
    assert np.array_equal(vout.cpu().numpy(), flags.astype(np.uint8)) and _same_bits(table, raw)
    # in place: the flags are taken from the caller's coordinates before any row is rewritten
    inplace = src.clone()
    predict.normalize_tracks(inplace, inplace, lens, res, valid_in=vin, valid_out=vout)
    assert np.array_equal(vout.cpu().numpy(), flags.astype(np.uint8)) and _same_bits(inplace, want)
    # the pose table of predict_tracks carries the flags; the caller's device tensors are not written
    dev_tracks = [torch.from_numpy(t).cuda() for t in tracks]
    pt, _ = predict.pose_table(dev_tracks, "cuda", resolutions=res, valid=given)
    assert _same_bits(pt.kp2d, want) and np.array_equal(pt.valid.cpu().numpy(), flags.astype(np.uint8))
    assert all(_same_bits(d, t) for d, t in zip(dev_tracks, tracks))
    # keyframes only: the flags are the keyframes'; rows that are not given keep 1 and zeros
    for s in (4, 5):
        keys, kgiven = [t[::s] for t in tracks], [g[::s] for g in given]
        kvin = torch.from_numpy(np.concatenate(kgiven).view(np.uint8)).cuda()
        ksrc = torch.from_numpy(np.concatenate(keys, 0)).cuda()
        dense_flags = np.concatenate([np.where(np.arange(len(e)) % s == 0, e, True) for e in eff])
        with np.errstate(invalid="ignore"):
            dense = np.concatenate([np.where((np.arange(len(w_)) % s == 0)[:, None, None], w_, 0.0).astype(np.float32)
                                    for w_ in _host_normalised(tracks)], 0)
        dense[~dense_flags] = 0.0
        table.fill_(7.0); vout.fill_(9)
        predict.normalize_tracks(ksrc, table, lens, res, key_stride=s, src_lens=[len(k) for k in keys], valid_in=kvin, valid_out=vout)
        assert np.array_equal(vout.cpu().numpy(), dense_flags.astype(np.uint8)), s
        assert _same_bits(table, dense), s


# ---- 2. both gathers against the numpy helper, exactly -------------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname", ["h36m_81", "h36m_351"])
@pytest.mark.parametrize("padding", ["copy", "zeros"])
def test_gathers_equal_the_rule_exactly(cfgname, padding):
    from uplift_upsample_3dhpe_amd import _capi
    from uplift_upsample_3dhpe_amd.data import PoseTable, SequenceGenerator
    cfg = util.load_config(cfgname)
    N, S, ms, J = cfg.SEQUENCE_LENGTH, cfg.SEQUENCE_STRIDE, MASK_STRIDE[cfgname], 17
    order = np.asarray(cfg.AUGM_FLIP_KEYPOINT_ORDER)
    lens = LENS
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    F = int(np.sum(lens))
    desc = _descriptors(cfg, lens, ms, flip=True)
    W = len(desc)
    lib = _capi.load_library()
    p = lambda t: C.c_void_p(t.data_ptr())
    d_desc = torch.from_numpy(desc).cuda()
    frame_base, zero_row = F, 2 * F
    rng = np.random.default_rng(5)
    coords = rng.normal(size=(F, J, 2)).astype(np.float32)
    changed = 0
    for name in PATTERNS:
        valid = np.concatenate([_pattern(name, n, S, seed=10 + i) for i, n in enumerate(lens)])
        kp = coords.copy(); kp[~valid] = 0.0                            # (missing frames are zeros in the pose table)
        table = PoseTable.from_device(torch.from_numpy(kp).cuda(), lens, valid=torch.from_numpy(valid.view(np.uint8)).cuda())
        plain = PoseTable.from_device(table.kp2d, lens)
        mk = lambda t: SequenceGenerator(t, seq_len=N, subsample=1, stride=S, padding_type=padding, flip_augment=False, flip_lr_indices=order,
                                         mask_stride=ms, stride_mask_align_global=True, shuffle=False)
        gen, gen_plain = mk(table), mk(plain)
        for zm in (0, 1):
            b = gen.gather(desc, zero_masked=bool(zm), with_3d=False)
            out, sm, pm = _np_gather(kp, desc, N, starts, lens, padding == "copy", zm, valid, order)
            assert np.array_equal(b["stride_mask"].cpu().numpy(), sm), (name, zm)
            assert np.array_equal(b["mask"].cpu().numpy(), pm), (name, zm)
            assert _same_bits(b["kp2d"], out), (name, zm)
            # the table without its flags: the old entry point, and the rule with no table
            b0 = gen_plain.gather(desc, zero_masked=bool(zm), with_3d=False)
            out0, sm0, pm0 = _np_gather(kp, desc, N, starts, lens, padding == "copy", zm, None, order)
            assert np.array_equal(b0["stride_mask"].cpu().numpy(), sm0) and np.array_equal(pm0, pm) and _same_bits(b0["kp2d"], out0)
            # a NULL validity pointer gives the bits of the old entry point
            x = torch.empty((W, N, J, 2), dtype=torch.float32, device="cuda")
            m1, m2 = torch.empty((W, N), dtype=torch.uint8, device="cuda"), torch.empty((W, N), dtype=torch.uint8, device="cuda")
            assert lib.uu3d_gather_windows_valid(p(plain.kp2d), p(plain.d_starts), p(plain.d_lens), p(d_desc), p(gen._d_flip), W, N, J, 2,
                                                 int(padding == "copy"), zm, None, p(x), p(m1), p(m2), None) == 0
            assert _same_bits(x, b0["kp2d"]) and torch.equal(m1, b0["stride_mask"]) and torch.equal(m2, b0["mask"])
            # the frames form
            rows = torch.empty((W, N), dtype=torch.int32, device="cuda")
            for vptr, vnp in ((p(table.valid), valid), (None, None)):
                assert lib.uu3d_gather_window_frames_valid(p(table.d_starts), p(table.d_lens), p(d_desc), W, N, int(padding == "copy"), zm,
                                                           frame_base, zero_row, vptr, p(rows), p(m1), p(m2), None) == 0
                r, sm_r, pm_r = _np_rows(desc, N, starts, lens, padding == "copy", zm, vnp, frame_base, zero_row)
                assert np.array_equal(rows.cpu().numpy(), r), (name, zm)
                assert np.array_equal(m1.cpu().numpy(), sm_r) and np.array_equal(m2.cpu().numpy(), pm_r), (name, zm)
            rows_old = torch.empty_like(rows)
            assert lib.uu3d_gather_window_frames(p(table.d_starts), p(table.d_lens), p(d_desc), W, N, int(padding == "copy"), zm, frame_base,
                                                 zero_row, p(rows_old), p(m1), p(m2), None) == 0
            assert torch.equal(rows_old, rows)
            if zm:
                changed += int((sm != sm0).sum())
                half = W // 2                                           # a flipped window uses the validity entry of its plain twin
                assert np.array_equal(sm[:half], sm[half:])
        if name == "all_valid":
            assert changed == 0
        if name == "all_missing":
            src, inside, have, _ = _np_windows(desc, N, starts, lens, padding == "copy", None)
            assert not sm[have].any()                                   # nothing that reads a frame is real; zero padding keeps its bit
            assert np.array_equal(sm[~have], sm0[~have])
    assert changed > 0


# ---- 3. predict_tracks against the oracle --------------------------------------------------------------------------------------------
def _oracle_tracks(cfg, arch, w, norm_tracks, ms, valid):
    """tracks_util._oracle_tracks with the host mask ANDed with validity and the missing frames zeroed."""
    zeroed = [np.where(v[:, None, None], t, np.float32(0.0)).astype(np.float32) for t, v in zip(norm_tracks, valid)]
    return tracks_util._oracle_tracks(cfg, arch, w, zeroed, ms, window_valid=lambda desc, c, table: _np_windows(
        desc, c.SEQUENCE_LENGTH, table.starts, table.lens, c.PADDING_TYPE == "copy", np.concatenate(valid))[3])


def _missing_30(lens, seed):
    valid = [_pattern("random30", n, 1, seed=seed + i) for i, n in enumerate(lens)]
    valid[-1][0] = valid[-1][-1] = False                                # the first and the last frame of one track
    return valid


@pytest.mark.parametrize("cfgname", ["h36m_351", "h36m_81"])
def test_predict_tracks_with_missing_frames_against_the_oracle(cfgname):
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model(cfgname)
    ms = MASK_STRIDE[cfgname]
    lens = LENS
    tracks = _pixel_tracks(lens, seed=4)
    res = [RES[i % len(RES)] for i in range(len(lens))]
    valid = _missing_30(lens, seed=20)
    want = _oracle_tracks(cfg, arch, w, _host_normalised(tracks), ms, valid)
    got, flags = predict.predict_tracks(model, cfg, tracks, resolutions=res, mask_stride=ms, flip=True, valid=valid, return_valid=True)
    assert [tuple(g.shape) for g in got] == [(n, 17, 3) for n in lens] and all(g.is_cuda and g.dtype == torch.float32 for g in got)
    assert all(f.dtype == torch.bool and f.is_cuda and np.array_equal(f.cpu().numpy(), v) for f, v in zip(flags, valid))
    assert model.check_range() is False
    a = torch.cat(got, 0).cpu().numpy()
    err = float(np.abs(a - want).max())
    print(f"{cfgname}: predict_tracks(valid) vs oracle pipeline max-abs {err:.3e} (bar {util.TOL_MAX_ABS})")
    assert err <= util.TOL_MAX_ABS
    assert not a[:, cfg.ROOT_KEYTPOINT].any() and float(np.abs(a).max()) > 1e-3
    b = torch.cat(predict.predict_tracks(model, cfg, tracks, resolutions=res, mask_stride=ms, flip=True, valid=valid, reuse_frames=False), 0).cpu().numpy()
    d = float(np.abs(a - b).max())
    print(f"{cfgname}: reuse_frames True vs False max-abs {d:.3e} (bar 3e-5)")
    assert d <= 3e-5
    assert float(np.abs(b - want).max()) <= util.TOL_MAX_ABS
    assert model.check_range() is False
    # the missing frames matter: the same tracks with every frame an observation give other poses
    full = torch.cat(predict.predict_tracks(model, cfg, tracks, resolutions=res, mask_stride=ms, flip=True), 0).cpu().numpy()
    assert float(np.abs(full - a).max()) > util.TOL_MAX_ABS


# ---- 4. identities, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname", ["h36m_351", "h36m_81"])
@pytest.mark.parametrize("reuse", [True, False])
def test_identities_bit_for_bit(cfgname, reuse):
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model(cfgname)
    ms = MASK_STRIDE[cfgname]
    lens = LENS
    tracks = _pixel_tracks(lens, seed=6)
    res = [RES[i % len(RES)] for i in range(len(lens))]
    run = lambda tr, **kw: predict.predict_tracks(model, cfg, tr, resolutions=res, mask_stride=ms, flip=True, reuse_frames=reuse, **kw)
    # valid all true equals valid=None (device flags, host flags, "finite" on finite tracks)
    base = torch.cat(run(tracks), 0)
    for v in ([np.ones(n, bool) for n in lens], [torch.ones(n, dtype=torch.bool, device="cuda") for n in lens], "finite"):
        assert _same_bits(torch.cat(run(tracks, valid=v), 0), base)
    # "finite" on NaN rows equals an explicit list with those rows holding +Inf, 1e30 and zeros: a missing frame never reaches the network
    valid = _missing_30(lens, seed=30)
    fill = lambda value: [np.where(v[:, None, None], t, np.float32(value)).astype(np.float32) for t, v in zip(tracks, valid)]
    ref, flags = run(fill(np.nan), valid="finite", return_valid=True)
    ref = torch.cat(ref, 0)
    assert all(np.array_equal(f.cpu().numpy(), v) for f, v in zip(flags, valid))
    assert bool(torch.isfinite(ref).all()) and model.check_range() is False
    for value in (np.inf, 1e30, 0.0):
        assert _same_bits(torch.cat(run(fill(value), valid=valid), 0), ref), value
    # flags on the host, on the device, mixed
    mixed = [torch.from_numpy(v).cuda() if i % 2 else v for i, v in enumerate(valid)]
    assert _same_bits(torch.cat(run(tracks, valid=mixed), 0), ref)
    # two calls: the same bits
    assert _same_bits(torch.cat(run(fill(np.nan), valid="finite"), 0), ref)
    # keyframes only with flags per keyframe: the bits of the full track where the padding source is a keyframe (length 4k + 1)
    if reuse:
        from uplift_upsample_3dhpe_amd.predict import padding_source_is_keyframe
        klens = [n for n in (1, 201) if padding_source_is_keyframe(n, cfg, ms)]
        ktracks = _pixel_tracks(klens, seed=8)
        kvalid = [_pattern("random30", n, 1, seed=40 + i) for i, n in enumerate(klens)]
        kres = res[:len(klens)]
        full = predict.predict_tracks(model, cfg, ktracks, resolutions=kres, mask_stride=ms, valid=kvalid)
        keys = predict.predict_tracks(model, cfg, [t[::ms] for t in ktracks], resolutions=kres, mask_stride=ms, keyframes_only=True, lengths=klens,
                                      valid=[v[::ms] for v in kvalid])
        assert all(_same_bits(f, k) for f, k in zip(full, keys))


# ---- 5. windows with nothing real --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname", ["h36m_351", "h36m_81"])
def test_a_track_of_missing_frames_only_stays_finite(cfgname):
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model(cfgname)
    ms = MASK_STRIDE[cfgname]
    lens = [50, 7]
    tracks = [np.full((n, 17, 2), np.nan, np.float32) for n in lens]
    assert model.check_range() is False
    for reuse in (True, False):
        got, flags = predict.predict_tracks(model, cfg, tracks, resolutions=RES[:2], mask_stride=ms, valid="finite", reuse_frames=reuse,
                                            return_valid=True)
        assert all(bool(torch.isfinite(g).all()) for g in got) and not any(bool(f.any()) for f in flags)
        assert model.check_range() is False                             # the range word stays down


# ---- 6. StreamSession: the truncation identity with missing frames ------------------------------------------------------------------
T = 3


def _run(session, tracks, valid, ticks, active=None):
    """Push ``tracks[i][k]`` (NaN where the pattern of slot i says missing and ``valid[i]`` is None, else the flag) -> host arrays."""
    poses = torch.zeros((ticks, T, 17, 3), dtype=torch.float32, device="cuda")
    fresh = torch.zeros((ticks, T), dtype=torch.bool, device="cuda")
    for k in range(ticks):
        kp = np.stack([tracks[i][k] for i in range(T)])
        v = None if valid is None else np.array([valid[i][k] for i in range(T)])
        p, f = session.push(kp, None if active is None else active(k), valid=v)
        poses[k].copy_(p)
        fresh[k].copy_(f)
    return poses.cpu().numpy(), fresh.cpu().numpy()


def _stream_valid(L, S, s_in):
    """Slot 0: a missing keyframe, a missing edge frame (a multiple of S that is no multiple of s_in), a run longer than s_in, the first
    frame; slot 1: a seeded 30 %; slot 2: every frame valid."""
    v0 = np.ones(L, bool)
    edge = 3 * S if (3 * S) % s_in else 3 * S + S
    assert edge % S == 0 and (s_in == S or edge % s_in != 0)
    v0[[0, 2 * s_in, edge]] = False
    v0[5 * s_in + 1:5 * s_in + 1 + s_in + 3] = False
    v0[L // 2:L // 2 + 2 * s_in + 1] = False
    return [v0, _pattern("random30", L, S, seed=3), np.ones(L, bool)], edge


@pytest.mark.parametrize("cfgname,ms,a", [("h36m_81", 4, 0), ("h36m_81", 4, 7), ("h36m_351", 10, 0), ("h36m_351", 10, 13)])
def test_truncation_identity_with_missing_frames(cfgname, ms, a):
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg, arch, w, model = _model(cfgname)
    S, N = cfg.SEQUENCE_STRIDE, cfg.SEQUENCE_LENGTH
    L = 2 * ((N - 1) * S + 1) + 3                                       # about two window spans
    tracks = _pixel_tracks([L] * T, seed=11)
    valid, edge = _stream_valid(L, S, ms)
    runs = []
    for graph, by_flag in ((True, True), (False, True), (True, False)):
        s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=a, graph=graph, missed_detections=True)
        # by_flag: the caller's flags beside finite coordinates; otherwise NaN rows and no flags
        pushed = tracks if by_flag else [np.where(v[:, None, None], t, np.float32(np.nan)).astype(np.float32) for t, v in zip(tracks, valid)]
        runs.append(_run(s, pushed, valid if by_flag else None, L))
        assert s.check_range() is False
        assert s.frames.cpu().tolist() == [L] * T and s.captures == (1 if graph else 0)      # a missing frame moves the counter
        s.close()
    poses, fresh = runs[0]
    for p, f in runs[1:]:                                               # graph on / off, flags / NaN rows: the same bits
        assert np.array_equal(f, fresh) and np.array_equal(_bits(p), _bits(poses))
    rule = np.array([stream.emits(t + 1, a, cfg, ms) for t in range(L)])
    assert np.array_equal(fresh, np.repeat(rule[:, None], T, 1))         # fresh is unchanged by validity
    assert np.isfinite(poses).all() and not poses[:, :, cfg.ROOT_KEYTPOINT].any()
    # slot 2 (every frame valid) has the bits of a session without missed_detections
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=a)
    old, _ = _run(s, tracks, None, L)
    s.close()
    assert np.array_equal(_bits(old[:, 2]), _bits(poses[:, 2])) and not np.array_equal(_bits(old[:, 0]), _bits(poses[:, 0]))
    # the checked ticks: the newest frame is the missing edge frame / the missing keyframe / inside the missing run, the ring has wrapped, the end
    fr = [t for t in range(L) if rule[t]]
    after = lambda f: next(t for t in fr if t >= f)
    cap = stream.ring_capacity(cfg, ms, a)
    ticks = sorted({fr[0], after(edge), after(edge + 1), after(2 * ms), after(5 * ms + 2), after(6 * ms + 3), after(L // 2 + ms),
                    after(cap * ms + 1), fr[len(fr) // 2], fr[-2], fr[-1]})
    assert after(edge) // S * S == edge and len(ticks) >= 8              # (at that tick the missing edge frame is what copy padding repeats)
    cut = [tracks[i][:t + 1] for t in ticks for i in range(T)]
    cut_valid = [valid[i][:t + 1] for t in ticks for i in range(T)]
    res = [RES[i] for t in ticks for i in range(T)]
    centres = np.array([t - a for t in ticks for i in range(T)])
    got = np.stack([poses[t, i] for t in ticks for i in range(T)])
    full = predict.predict_tracks(model, cfg, cut, resolutions=res, mask_stride=ms, flip=True, valid=cut_valid)
    want = np.stack([full[k][c].cpu().numpy() for k, c in enumerate(centres)])
    d = np.abs(got - want).reshape(len(ticks), -1).max(1)
    print(f"{cfgname} s_in {ms} lookahead {a}: ticks {ticks}")
    print(f"  max-abs to predict_tracks(valid) on the truncated track {d.max():.3e} (bar {util.TOL_MAX_ABS})")
    assert d.max() <= util.TOL_MAX_ABS
    assert float(np.abs(want).max()) > 1e-3


def test_slots_do_not_talk_and_inactive_differs_from_missing():
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    L = 60
    tracks = _pixel_tracks([L] * T, seed=21)
    new = lambda: stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=4, flip=True, lookahead=3, missed_detections=True)
    all_valid = [np.ones(L, bool)] * T
    miss0 = [np.ones(L, bool) for _ in range(T)]
    miss0[0][[4, 8, 9, 10, 11, 12, 13, 30]] = False
    s = new(); pa, fa = _run(s, tracks, all_valid, L); s.close()
    s = new(); pb, fb = _run(s, tracks, miss0, L)
    assert s.frames.cpu().tolist() == [L] * T                            # valid = 0 moves the counter
    s.close()
    assert np.array_equal(fa, fb)
    assert np.array_equal(_bits(pa[:, 1]), _bits(pb[:, 1])) and np.array_equal(_bits(pa[:, 2]), _bits(pb[:, 2]))
    assert not np.array_equal(_bits(pa[:, 0]), _bits(pb[:, 0]))
    # active = 0 with a NaN row: ignored, the counter does not move, and the track continues as if the tick had not happened
    s = new()
    gap = {10, 11, 25}
    poses, used = [], [0] * T
    for k in range(L + len(gap)):
        act = np.array([k not in gap, True, True])
        kp = np.stack([tracks[i][min(used[i], L - 1)] for i in range(T)])
        if not act[0]:
            kp[0] = np.nan
        live = act & np.array([u < L for u in used])
        p, f = s.push(kp, live, valid=np.array([True] * T))
        poses.append((p.clone(), f.clone(), live.copy(), list(used)))
        used = [u + int(l) for u, l in zip(used, live)]
        if k == 11:
            assert s.frames.cpu().tolist() == [10, 12, 12]
    assert s.frames.cpu().tolist() == [L] * T and s.check_range() is False
    s.close()
    prev = np.zeros((17, 3), np.float32)
    for p, f, live, u in poses:
        p0 = p[0].cpu().numpy()
        if live[0]:                                                     # the track goes on as if the ignored ticks had not happened
            assert bool(f[0]) == bool(fa[u[0], 0])
            assert float(np.abs(p0 - pa[u[0], 0]).max()) <= util.TOL_MAX_ABS
        else:                                                           # an ignored tick: not fresh, the held pose bit for bit
            assert not bool(f[0]) and np.array_equal(_bits(p0), _bits(prev))
        prev = p0


# ---- 7. push never waits -------------------------------------------------------------------------------------------------------------
def test_push_with_flags_never_waits_for_the_device():
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    tracks = _pixel_tracks([12] * T, seed=51)
    host = np.stack([t[0] for t in tracks])
    nan_row = host.copy(); nan_row[2] = np.nan
    for graph in (True, False):
        s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=4, flip=True, graph=graph, missed_detections=True)
        dev_flags = torch.tensor([True, True, False], device="cuda")
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            s.push(host, valid=np.array([True, False, True]))
            s.push(host, valid=[1, 1, 0])
            s.push(torch.from_numpy(host), active=[True, False, True], valid=torch.tensor([True, True, False]))
            s.push(nan_row, valid=dev_flags)
            poses, fresh = s.push(host)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert poses.is_cuda and tuple(poses.shape) == (T, 17, 3) and bool(torch.isfinite(poses).all())
        assert s.frames.cpu().tolist() == [5, 4, 5] and s.check_range() is False
        s.close()
    with pytest.raises(ValueError, match="missed_detections=True"):
        s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=4)
        try:
            s.push(host, valid=[1, 1, 1])
        finally:
            s.close()
