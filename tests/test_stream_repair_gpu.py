"""Live per-joint missed detections on the device: StreamSession(repair_joints=G).
  1. uu3d_stream_repair_stage alone, tick by tick, bit for bit against stream.LiveRepairHost
  2. the truncation identity: the pose of frame t - lookahead is predict_tracks(repair_joints=G)'s on the track cut at t
  3. graph on / off and flags / NaN coordinates give the same bits
  4. slots do not talk, reset starts a slot clean, an inactive slot keeps its state
  5. push with device-side per-joint flags never waits
  6. replay_tracks(repair_joints=G) equals the pushes by hand"""
import ctypes as C

import numpy as np
import pytest

from tests import util
from tests.tracks_util import RES, _bits, _host_normalised, _model, _pixel_tracks

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
T, J = 3, 17


def _random_flags(L, seed, share=0.10):
    return np.random.default_rng(seed).uniform(size=(L, J)) >= share


def _hand_flags(L, G, s_in, cap):
    """Slot 0 of the truncation test -> ((L, J) flags, the ticks at which its runs close)."""
    f = np.ones((L, J), bool)
    k1, k2, f0, k3 = 3 * s_in, 6 * s_in, 9 * s_in + 1, 12 * s_in
    f[k1 - 1:k1 - 1 + G, 3] = False                                     # G frames over keyframe k1: interpolated once frame k1 - 1 + G is in
    f[k2:k2 + G + 1, 5] = False                                         # G + 1 frames: keyframe k2 is held, then turns missing at k2 + G + 1
    f[:G, 7] = False                                                    # a leading gap of G frames: held from frame G
    f[:G + 1, 8] = False                                                # ... of G + 1: frame 0 stays missing
    f[f0 - 1:f0 + 2, 1:3] = False                                       # a short run with a frame that has no observed joint inside
    f[f0] = False
    long_run = cap * s_in + 6                                           # longer than the ring reaches back
    f[k3:k3 + long_run, 12] = False
    f[L - 20:, 10] = False                                              # never seen again
    assert k3 + long_run < L - 25
    return f, [k1 - 1 + G, k2 + G + 1, G, G + 1, f0 + 2, k3 + long_run]


def _push_all(s, tracks, flags, ticks, active=None, nan=False, collect_state=False):
    """Push tracks[i][k] with flags[i][k] (J,) into slot i at tick k -> poses (ticks, T, J, 3), fresh (ticks, T) [, joint states (ticks, T, J)]
    as host arrays; ``nan``: no flags, NaN coordinates in their place."""
    poses = torch.zeros((ticks, T, J, 3), dtype=torch.float32, device="cuda")
    fresh = torch.zeros((ticks, T), dtype=torch.bool, device="cuda")
    states = torch.zeros((ticks, T, J), dtype=torch.uint8, device="cuda")
    for k in range(ticks):
        kp = np.stack([tracks[i][k] for i in range(T)])
        v = np.stack([flags[i][k] for i in range(T)])
        if nan:
            kp = np.where(v[:, :, None], kp, np.float32(np.nan)).astype(np.float32)
        p, f = s.push(kp, None if active is None else active(k), valid=None if nan else v)
        poses[k].copy_(p)
        fresh[k].copy_(f)
        states[k].copy_(s.joint_state)
    out = poses.cpu().numpy(), fresh.cpu().numpy()
    return out + ((states.cpu().numpy(),) if collect_state else ())


# ---- 1. the stage alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [3, 6])
def test_stage_alone_bit_for_bit(G):
    from uplift_upsample_3dhpe_amd import _capi, stream
    from uplift_upsample_3dhpe_amd._capi import ptr
    cfg, arch, w, model = _model("h36m_81")
    lib, h = _capi.load_library(), model._h
    S, s_in, L = cfg.SEQUENCE_STRIDE, 4, 40
    K = stream.staged_frames(G, s_in)
    scfg = _capi.Uu3dStreamConfig(T, S, s_in, S, 0, 1, 1, 0)
    lay = _capi.Uu3dStreamLayout()
    _capi.check(lib, lib.uu3d_stream_state_layout(h, C.byref(scfg), C.byref(lay)), h)
    play = _capi.Uu3dStreamRepairLayout()
    _capi.check(lib, lib.uu3d_stream_repair_layout(h, C.byref(scfg), G, C.byref(play)), h)
    assert int(play.staged_frames) == K and int(play.window) == G + 1 and int(play.bytes) == lib.uu3d_stream_repair_bytes(h, C.byref(scfg), G)
    dev = model.device
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    state, repair = z(int(lay.bytes), torch.uint8), z(int(play.bytes), torch.uint8)
    counters = state[int(lay.frames_offset):int(lay.frames_offset) + 4 * T].view(torch.int32)
    kp, flags_dev, active = z((T, J, 2), torch.float32), z((T, J), torch.uint8), z((T,), torch.uint8)
    res = torch.tensor(RES, dtype=torch.float64, device=dev)
    order_host = np.ascontiguousarray(cfg.AUGM_FLIP_KEYPOINT_ORDER, np.int32)
    order = torch.from_numpy(order_host).to(dev)
    staged = torch.full((2 * T * K, J, 2), 7.0, dtype=torch.float32, device=dev)
    stage_frame, stage_valid = torch.full((T, K), 99, dtype=torch.int32, device=dev), torch.full((T, K), 9, dtype=torch.uint8, device=dev)
    far, joint_state = torch.full((T, G), 99, dtype=torch.int32, device=dev), torch.full((T, J), 9, dtype=torch.uint8, device=dev)
    tracks = _pixel_tracks([L] * T, seed=5)
    flags = [_random_flags(L, seed=i, share=0.25) for i in range(T)]
    flags[0][3:3 + G, 2] = False; flags[0][2, 2] = flags[0][3 + G, 2] = True            # a run of G: closes
    flags[1][8:8 + G + 2, 4] = False; flags[1][7, 4] = flags[1][8 + G + 2, 4] = True    # a run of G + 2: a far list
    flags[2][:G, 6] = False                                                              # a leading gap
    tracks[1][20, 3] = np.nan                                                            # a non-finite coordinate is an unobserved joint
    hosts = [stream.LiveRepairHost(J, G, s_in, S) for _ in range(T)]
    used, far_seen, revised = [0] * T, 0, 0
    stream_ptr = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for k in range(L + 2):
        act = np.array([u < L for u in used]) & np.array([k not in (11, 12), True, True])  # slot 0 sits out two ticks
        kp.copy_(torch.from_numpy(np.stack([tracks[i][min(used[i], L - 1)] for i in range(T)])))
        flags_dev.copy_(torch.from_numpy(np.stack([flags[i][min(used[i], L - 1)] for i in range(T)]).view(np.uint8)))
        active.copy_(torch.from_numpy(act.view(np.uint8)))
        before_state = joint_state.cpu().numpy().copy()
        _capi.check(lib, lib.uu3d_stream_repair_stage(h, C.byref(scfg), G, ptr(state), ptr(repair), ptr(kp), ptr(res), ptr(active), ptr(order),
                                                     ptr(flags_dev), ptr(staged), ptr(stage_frame), ptr(stage_valid), ptr(far), ptr(joint_state),
                                                     stream_ptr), h)
        counters.add_(active.to(torch.int32))                           # what the commit does
        got_staged = staged.cpu().numpy().reshape(2, T, K, J, 2)
        got_frame, got_valid, got_far, got_state = stage_frame.cpu().numpy(), stage_valid.cpu().numpy(), far.cpu().numpy(), joint_state.cpu().numpy()
        want = [None] * T
        for i in range(T):
            if act[i]:
                want[i] = hosts[i].step(tracks[i][used[i]], flags[i][used[i]])
                used[i] += 1
        norm = _host_normalised([np.stack([xy for _, xy, _, _ in want[i][0]]) if want[i] else np.zeros((0, J, 2), np.float32) for i in range(T)])
        for i in range(T):
            if not act[i]:                                              # nothing staged, nothing far, the state kept
                assert (got_frame[i] == -1).all() and not got_valid[i].any() and (got_far[i] == -1).all() and not got_staged[:, i].any()
                assert np.array_equal(got_state[i], before_state[i])
                continue
            entries, far_want = want[i]
            assert got_frame[i].tolist() == [f for f, _, _, _ in entries] + [-1] * (K - len(entries)), (k, i)
            assert got_valid[i].tolist() == [int(ok) for _, _, ok, _ in entries] + [0] * (K - len(entries)), (k, i)
            assert sorted(f for f in got_far[i].tolist() if f >= 0) == far_want, (k, i)
            assert np.array_equal(got_state[i], hosts[i].newest_state()), (k, i)
            for e in range(K):
                ok = e < len(entries) and entries[e][2]
                plain = norm[i][e] if ok else np.zeros((J, 2), np.float32)
                mirrored = plain[order_host] * np.array([-1.0, 1.0], np.float32) if ok else plain
                assert np.array_equal(_bits(got_staged[0, i, e]), _bits(plain)), (k, i, e)
                assert np.array_equal(_bits(got_staged[1, i, e]), _bits(mirrored)), (k, i, e)
            far_seen += len(far_want)
            revised += sum(1 for f, _, ok, st in entries if ok and f < used[i] - 1 and (st == 2).any())
    assert far_seen >= 1 and revised >= 3 and used == [L] * T


# ---- 2. the truncation identity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname,ms,a,G", [("h36m_81", 4, 0, 3), ("h36m_81", 4, 0, 6), ("h36m_81", 4, 7, 3), ("h36m_81", 4, 7, 6),
                                            ("h36m_351", 10, 0, 6), ("h36m_351", 10, 7, 3)])
def test_truncation_identity_with_missing_joints(cfgname, ms, a, G):
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg, arch, w, model = _model(cfgname)
    S, N = cfg.SEQUENCE_STRIDE, cfg.SEQUENCE_LENGTH
    L = 2 * ((N - 1) * S + 1) + 3                                       # about two window spans
    cap = stream.ring_capacity(cfg, ms, a)
    tracks = _pixel_tracks([L] * T, seed=11)
    hand, closes = _hand_flags(L, G, ms, cap)
    flags = [hand, _random_flags(L, seed=3), np.ones((L, J), bool)]
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=a, repair_joints=G)
    assert s.staged_frames == G // ms + 2 and s.missed_detections
    poses, fresh, states = _push_all(s, tracks, flags, L, collect_state=True)
    assert s.check_range() is False and s.captures == 1 and s.frames.cpu().tolist() == [L] * T
    s.close()
    rule = np.array([stream.emits(t + 1, a, cfg, ms) for t in range(L)])
    assert np.array_equal(fresh, np.repeat(rule[:, None], T, 1))
    assert np.isfinite(poses).all()
    for i in range(T):                                                  # joint_state: the newest frame under the rule on the cut track
        trailing = np.stack([predict.repair_joints_host([tracks[i][:t + 1]], [flags[i][:t + 1]], G)[2][0][t] for t in closes + [L - 1]])
        assert np.array_equal(states[closes + [L - 1], i], trailing), i
    # a session that declares those frames missing as a whole: slot 2 (every joint seen) has its bits, slot 0 does not
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=a, missed_detections=True)
    whole = torch.zeros((L, T, J, 3), dtype=torch.float32, device="cuda")
    for k in range(L):
        p, _ = s.push(np.stack([tracks[i][k] for i in range(T)]), valid=np.array([flags[i][k].all() for i in range(T)]))
        whole[k].copy_(p)
    s.close()
    whole = whole.cpu().numpy()
    assert np.array_equal(_bits(whole[:, 2]), _bits(poses[:, 2])) and not np.array_equal(_bits(whole[:, 0]), _bits(poses[:, 0]))
    # the checked ticks: where each run closes, the tick before, `lookahead` later; after the ring has wrapped; the last
    fr = [t for t in range(L) if rule[t]]
    after = lambda f: next(t for t in fr if t >= f)
    ticks = sorted({after(x) for c in closes for x in (c - 1, c, c + a)} | {after(cap * ms + 1), fr[-1]})
    assert 8 <= len(ticks) <= 20
    cut = [tracks[i][:t + 1] for t in ticks for i in range(T)]
    cut_flags = [flags[i][:t + 1] for t in ticks for i in range(T)]
    res = [RES[i] for t in ticks for i in range(T)]
    centres = np.array([t - a for t in ticks for i in range(T)])
    got = np.stack([poses[t, i] for t in ticks for i in range(T)])
    full = predict.predict_tracks(model, cfg, cut, resolutions=res, mask_stride=ms, flip=True, valid=cut_flags, repair_joints=G)
    want = np.stack([full[k][c].cpu().numpy() for k, c in enumerate(centres)])
    d = np.abs(got - want).reshape(len(ticks), T, -1).max(2)
    print(f"{cfgname} s_in {ms} lookahead {a} G {G}: ticks {ticks}")
    print(f"  max-abs to predict_tracks(repair_joints) on the truncated track, per slot {d.max(0)} (bar {util.TOL_MAX_ABS})")
    assert d.max() <= util.TOL_MAX_ABS
    assert float(np.abs(want).max()) > 1e-3


# ---- 3. graph and input forms ----------------------------------------------------------------------------------------------------------
def test_graph_on_off_and_nan_coordinates_give_the_same_bits():
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    L, a, G = 70, 3, 5
    tracks = _pixel_tracks([L] * T, seed=13)
    flags = [_random_flags(L, seed=20 + i, share=0.15) for i in range(T)]
    flags[0][10:10 + G + 3, 4] = False
    runs = []
    for graph, nan in ((True, False), (False, False), (True, True)):
        s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=4, flip=True, lookahead=a, graph=graph, repair_joints=G)
        runs.append(_push_all(s, tracks, flags, L, nan=nan, collect_state=True))
        assert s.check_range() is False and s.captures == (1 if graph else 0) and s.frames.cpu().tolist() == [L] * T
        s.close()
    poses, fresh, states = runs[0]
    for p, f, st in runs[1:]:
        assert np.array_equal(f, fresh) and np.array_equal(_bits(p), _bits(poses)) and np.array_equal(st, states)
    rule = np.array([stream.emits(t + 1, a, cfg, 4) for t in range(L)])
    assert np.array_equal(fresh, np.repeat(rule[:, None], T, 1))
    assert (states == 2).any() and (states == 0).any() and np.isfinite(poses).all()


# ---- 4. slots, reset, inactive ---------------------------------------------------------------------------------------------------------
def test_slots_do_not_talk_reset_starts_clean_inactive_keeps_state():
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    L, a, G = 60, 3, 4
    tracks = _pixel_tracks([L] * T, seed=21)
    flags = [_random_flags(L, seed=30 + i, share=0.2) for i in range(T)]
    flags[1][25:25 + G + 4, 6] = False                                  # slot 1 is reset inside this gap
    new = lambda res=RES: stream.StreamSession(model, cfg, slots=T, resolutions=res, mask_stride=4, flip=True, lookahead=a, repair_joints=G)
    s = new(); pa, fa, sa = _push_all(s, tracks, flags, L, collect_state=True); s.close()
    # permuting the slots permutes the results (pixel tracks are made for the resolution of their index)
    perm = [2, 0, 1]
    s = new([RES[i] for i in perm])
    pb, fb, sb = _push_all(s, [tracks[i] for i in perm], [flags[i] for i in perm], L, collect_state=True)
    s.close()
    for slot, i in enumerate(perm):
        assert np.array_equal(_bits(pb[:, slot]), _bits(pa[:, i])) and np.array_equal(sb[:, slot], sa[:, i])
    # reset of slot 1 at tick 28, in the middle of its gap: it then runs its track from frame 0 and gives the bits of a fresh slot
    s = new()
    used = [0] * T
    for k in range(28 + 30):
        if k == 28:
            s.reset([1])
            used[1] = 0
        p, f = s.push(np.stack([tracks[i][used[i]] for i in range(T)]), valid=np.stack([flags[i][used[i]] for i in range(T)]))
        for i in range(T):
            assert np.array_equal(_bits(p[i]), _bits(pa[used[i], i])) and bool(f[i]) == bool(fa[used[i], i]), (k, i)
            assert np.array_equal(s.joint_state[i].cpu().numpy(), sa[used[i], i]), (k, i)
        used = [u + 1 for u in used]
    assert s.frames.cpu().tolist() == [58, 30, 58] and s.check_range() is False
    s.close()
    # an inactive slot: its row is ignored, counter and joint states stay, the track goes on as if the tick had not happened
    s = new()
    used, gap = [0] * T, {10, 11, 26}
    for k in range(L + len(gap)):
        act = np.array([k not in gap, True, True]) & np.array([u < L for u in used])
        kp = np.stack([tracks[i][min(used[i], L - 1)] for i in range(T)])
        v = np.stack([flags[i][min(used[i], L - 1)] for i in range(T)])
        if k in gap:
            kp[0], v[0] = np.nan, False
            before = (s.joint_state[0].clone(), s.frames[0].clone())
        p, f = s.push(kp, act, valid=v)
        if k in gap:
            assert torch.equal(s.joint_state[0], before[0]) and torch.equal(s.frames[0], before[1]) and not bool(f[0])
        for i in range(T):
            if act[i]:
                assert bool(f[i]) == bool(fa[used[i], i])
                assert float((p[i].cpu() - torch.from_numpy(pa[used[i], i])).abs().max()) <= util.TOL_MAX_ABS, (k, i)
                assert np.array_equal(s.joint_state[i].cpu().numpy(), sa[used[i], i]), (k, i)
        used = [u + int(x) for u, x in zip(used, act)]
    assert s.frames.cpu().tolist() == [L] * T and s.check_range() is False
    s.close()


# ---- 5. push never waits ---------------------------------------------------------------------------------------------------------------
def test_push_with_device_side_joint_flags_never_waits():
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    tracks = _pixel_tracks([12] * T, seed=51)
    host = np.stack([t[0] for t in tracks])
    nan_joint = host.copy(); nan_joint[2, 5] = np.nan
    for graph in (True, False):
        s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=4, flip=True, graph=graph, repair_joints=3)
        dev_joint = torch.ones((T, J), dtype=torch.bool, device="cuda"); dev_joint[1, 4] = False
        dev_slot = torch.tensor([True, True, False], device="cuda")
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            s.push(host, valid=dev_joint)
            s.push(host, valid=np.ones((T, J), bool))
            s.push(torch.from_numpy(host), active=[True, False, True], valid=torch.ones((T, J), dtype=torch.uint8))
            s.push(nan_joint, valid=dev_slot)
            s.push(host, valid=[1, 0, 1])
            poses, fresh = s.push(host)
            state = s.joint_state
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert poses.is_cuda and tuple(poses.shape) == (T, J, 3) and bool(torch.isfinite(poses).all())
        assert s.frames.cpu().tolist() == [6, 5, 6] and s.check_range() is False
        assert tuple(state.shape) == (T, J) and state.dtype == torch.uint8 and bool((state == 1).all())
        with pytest.raises(ValueError, match=r"valid must be \(3,\) or \(3, 17\)"):
            s.push(host, valid=np.ones((T, 2), bool))
        s.close()
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=4, missed_detections=True)
    try:
        with pytest.raises(ValueError, match=r"valid must be \(3,\)"):
            s.push(host, valid=np.ones((T, J), bool))                   # per-joint flags need repair_joints
        with pytest.raises(AttributeError, match="repair_joints"):
            s.joint_state
    finally:
        s.close()


# ---- 6. replay_tracks ------------------------------------------------------------------------------------------------------------------
def test_replay_tracks_equals_the_pushes_by_hand():
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    lens, a, G = [40, 25, 33], 2, 3
    tracks = _pixel_tracks(lens, seed=61)
    flags = [_random_flags(n, seed=70 + i, share=0.2) for i, n in enumerate(lens)]
    valid = [flags[0], flags[1].all(axis=1), torch.from_numpy(flags[2])]     # (T_i, J), (T_i,) and a tensor
    poses, fresh = stream.replay_tracks(model, cfg, tracks, resolutions=RES, mask_stride=4, flip=True, lookahead=a, valid=valid, repair_joints=G)
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=4, flip=True, lookahead=a, repair_joints=G)
    flags[1] = np.repeat(flags[1].all(axis=1)[:, None], J, axis=1)
    for k in range(max(lens)):
        act = np.array([k < n for n in lens])
        p, f = s.push(np.stack([tracks[i][min(k, lens[i] - 1)] for i in range(T)]), act, valid=np.stack([flags[i][min(k, lens[i] - 1)] for i in range(T)]))
        for i in range(T):
            if act[i]:
                assert np.array_equal(_bits(p[i]), _bits(poses[i][k])) and bool(f[i]) == bool(fresh[i][k]), (k, i)
    s.close()
    assert [p.shape for p in poses] == [(n, J, 3) for n in lens] and sum(int(f.sum()) for f in fresh) > 10
    with pytest.raises(ValueError, match="repair_joints needs valid"):
        stream.replay_tracks(model, cfg, tracks, resolutions=RES, mask_stride=4, repair_joints=G)
