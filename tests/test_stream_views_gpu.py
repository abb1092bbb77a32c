"""GPU: live several views, StreamSession(views=V) (include/uu3d.h, LIVE SEVERAL VIEWS; live_views.py).  Everything is compared bit for bit.
  1. the stage alone, no model: the chain LiveRoot -> LiveWorld -> LiveViews on caller-made buffers, driven by the script of
     tests/stream_views_util.py (a view below min_root_joints, a view inactive, a slot reset alone, every view blind, state 0 after a full
     reset, one view's joints on one pixel): every buffer and the counters equal stream.LiveViewsHost at every push
  2. the session on h36m_81 with seeded weights, V = 2, N = 2: every push equals LiveViewsHost stepped on what the same session without
     views returned, plus the pushed frames; with smooth and rotations the filtered rows and the quaternions equal LiveOneEuroHost and
     joint_rotations_host on the fused rows; captures stays 1; one case with fps=30
  3. the chain to offline: with all slots active and in phase a fresh person's pose is fuse_views_host of predict_tracks' world poses for
     the tracks cut to their first t + 1 frames, at frame t - lookahead, and a state-1 root is solve_view_roots_host there (the offline
     call runs its forwards in batches of the session's V N windows: with predict_tracks' default batches the lifts themselves differ from
     the session's by 3e-6 to 5e-6, one run on an MI355X, as they do without views)"""
import ctypes as C

import numpy as np
import pytest

from tests import stream_views_util as svu
from tests.tracks_util import _model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
J, M, MS = svu.J, svu.M, 4
RES = (1024, 1024)                                                      # (the ring cameras' principal point is near (512, 516))


def _host(t):
    return t.detach().cpu().numpy()


# ---- 1. the stage alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,N,lookahead", [(1, 1, 0), (1, 3, 2), (2, 1, 2), (2, 3, 0), (8, 1, 0), (8, 3, 2)])
def test_stage_alone_equals_the_mirror(V, N, lookahead):
    from uplift_upsample_3dhpe_amd import _capi, stream
    lib = _capi.load_library()
    dev = torch.device("cuda", 0)
    a, T = lookahead, V * N
    cams, pushes = svu.script(V, N, a)
    rows = svu.world_rows(cams, N)
    plain = np.ascontiguousarray(np.stack([np.asarray(c.intrinsics, np.float64) for c in cams for _ in range(N)]))
    frames = torch.zeros(T, dtype=torch.int32, device=dev)
    active, fresh = torch.zeros(T, dtype=torch.uint8, device=dev), torch.zeros(T, dtype=torch.uint8, device=dev)
    poses, kp = torch.zeros((T, J, 3), device=dev), torch.zeros((T, J, 2), device=dev)
    flags = torch.ones((T, J), dtype=torch.uint8, device=dev)
    root = stream.LiveRoot(T, J, a, plain, M, kp, flags, device=dev)
    world = stream.LiveWorld(T, J, rows, device=dev)
    fused = stream.LiveViews(T, J, V, root, cams, device=dev)
    stream.scenes(stream.Scene(poses, fresh, None, None, ()), [("camera", root), ("world", world), ("fused", fused)])
    for t in (fused._state, root._state):                               # (the resets must make the blocks usable whatever they held)
        t.fill_(0xAB)
    tick = [root.launch(active, frames), world.launch(), fused.launch(active, frames)]
    resets = [root.reset_launch(), fused.reset_launch()]
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(steps, *more):
        for fn, args in steps:
            assert fn(*args, *more, st) == 0, fn.__name__

    run(resets, None)
    host = stream.LiveViewsHost(V, N, J, a, cams, M)
    count = np.zeros(T, np.int64)
    ticks = len(pushes)
    got = {name: torch.zeros((ticks,) + tuple(t.shape), dtype=t.dtype, device=dev) for name, t in
           (("poses", fused.poses), ("fresh", fused.fresh), ("roots", fused.roots), ("state", fused.state), ("view_count", fused.view_count),
            ("frames", fused.frames), ("active", fused.active))}
    want = []
    for k, p in enumerate(pushes):
        count += p["active"]
        fr = svu.fresh_of(count, p["active"], a, k, V, N)
        for dst, src in ((frames, count.astype(np.int32)), (active, p["active"].view(np.uint8)), (fresh, fr.view(np.uint8)), (poses, p["poses"]),
                         (kp, p["kp"]), (flags, p["flags"])):
            dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
        run(tick)
        for name, t in got.items():
            t[k].copy_(getattr(fused, name))
        want.append(host.step(p["kp"], p["flags"], p["active"], fr, svu.to_world(p["poses"], rows)) + (host.frames.copy(), host.active.copy()))
        if p["reset"] is not None:
            chosen = None if p["reset"] == "all" else p["reset"]
            mask = None
            if chosen is not None:
                h = np.zeros(T, np.uint8)
                h[chosen] = 1
                mask = torch.from_numpy(h).to(dev)
            run(resets, None if mask is None else C.c_void_p(mask.data_ptr()))
            host.reset(chosen)
            count[slice(None) if chosen is None else chosen] = 0
    got = {name: _host(t) for name, t in got.items()}
    for k, w in enumerate(want):
        for name, ref in zip(("poses", "fresh", "roots", "state", "view_count", "frames", "active"), w):
            ref = np.asarray(ref)
            assert svu.same(got[name][k], ref.astype(got[name].dtype) if ref.dtype != got[name].dtype else ref), (k, name)
    states, counts, fr = np.stack([w[3] for w in want]), np.stack([w[4] for w in want]), np.stack([w[1] for w in want])
    print(f"V {V} N {N} lookahead {a}: states 0 / 1 / 2 {np.bincount(states.ravel(), minlength=3).tolist()}, view_count 0 while fresh "
          f"{int(((counts == 0) & fr).sum())}, not fresh {int((~fr).sum())}")
    assert (states == 1).any() and (states == 0).any() and ((counts == 0) & fr).any() and (V == 1 or (states == 2).any())
    assert counts.max() == V and (V == 1 or (counts[fr] < V).any())


# ---- 2. the session ---------------------------------------------------------------------------------------------------------------------
TICKS = 24


def _expand(cams, N):
    return [c for c in cams for _ in range(N)]


@pytest.mark.parametrize("form", ["lookahead0", "lookahead2", "fps30"])
def test_session_equals_the_mirror_on_the_session_without_views(form):
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg, arch, w, model = _model("h36m_81")
    V, N = 2, 2
    T = V * N
    fps = 30 if form == "fps30" else None
    rate = 50 if fps is None else fps
    a = {"lookahead0": 0, "lookahead2": 2}.get(form)
    if a is None:
        a = max(2, stream.rate_plan(cfg, fps, None, MS).min_lookahead)
    cams, _, kp = svu.person_tracks(V, N, TICKS, 31)
    kp[7, 0, M - 1:] = np.nan                                           # view 0 of person 0 below min_root_joints
    kp[9] = np.nan                                                      # everybody blind
    kp[11, 1] = kp[11, 1, 2]                                            # view 0 of person 1 on one pixel ...
    kp[11, 3] = np.nan                                                  # ... and alone
    common = dict(slots=T, resolutions=RES, mask_stride=MS, flip=True, lookahead=a, missed_detections=True, **({} if fps is None else {"fps": fps}))
    ref = stream.StreamSession(model, cfg, camera=_expand(cams, N), **common)
    s = stream.StreamSession(model, cfg, camera=cams, views=V, **common)
    full = stream.StreamSession(model, cfg, camera=cams, views=V, smooth=True, rotations=True, **common)
    table = lambda t: [fn.__name__ for fn, args in (t._tick_steps if fps is None else t._push_after) if args is not None]
    at = table(ref).index("uu3d_camera_to_world")
    assert table(s) == table(ref)[:at + 1] + ["uu3d_stream_views"] + table(ref)[at + 1:]                            # directly behind "world"
    assert table(full) == table(s) + ["uu3d_stream_one_euro"] * 2 + ["uu3d_joint_rotations"]
    pose_filter, root_filter = predict.check_smooth(True, True)
    hp, hq = stream.LiveOneEuroHost(N, 3 * J, rate, pose_filter, a), stream.LiveOneEuroHost(N, 3, rate, root_filter, a)
    host = stream.LiveViewsHost(V, N, J, a, cams, M)
    rows = []
    try:
        for k in range(TICKS):
            act = np.ones(T, bool)
            act[2] = k != 5                                             # view 1 of person 0 sits one push out
            if k in (15, 18):                                           # person 1 starts again, both slots together; later slot 0 alone: no person is reset
                chosen = [1, 3] if k == 15 else [0]
                for x in (ref, s, full):
                    x.reset(chosen)
                host.reset(chosen)
                if k == 15:
                    hp.reset([1]); hq.reset([1])
            out = [[t.clone() for t in x.push(kp[k], None if act.all() else act)] for x in (ref, s, full)]
            assert ref.captures == s.captures == full.captures == 1
            r, g, f = ([_host(t) for t in o] for o in out)
            view_p, view_r, raw_p, raw_r, full_p, full_r = (_host(t.clone()) for t in (s.view_poses, s.view_roots, s.raw_poses, s.raw_roots,
                                                                                       full.raw_poses, full.raw_roots))
            assert len(r) == 4 and len(g) == 5 and len(f) == 6
            assert g[0].shape == (N, J, 3) and g[1].shape == (N,) and g[2].shape == (N, 3) and g[3].dtype == np.uint8 and g[4].dtype == np.uint8
            want = host.step(kp[k], None, act, r[1], r[0])
            for name, got, ref_ in zip(("poses", "fresh", "roots", "state", "view_count"), g, want):
                assert svu.same(got, np.asarray(ref_).astype(got.dtype)), (form, k, name)
            assert svu.same(view_p, r[0]) and svu.same(view_r, r[2]) and svu.same(raw_p, g[0]) and svu.same(raw_r, g[2]), k
            assert svu.same(full_p, g[0]) and svu.same(full_r, g[2]) and svu.same(f[1], g[1]) and svu.same(f[3], g[3]) and svu.same(f[4], g[4]), k
            assert svu.same(f[0], hp.step(g[0].reshape(N, -1), host.frames, g[1], host.active).reshape(N, J, 3)), (form, k)
            assert svu.same(f[2], hq.step(g[2], host.frames, g[1], host.active, g[3])), (form, k)
            assert svu.same(f[5], predict.joint_rotations_host(f[0])[0]), (form, k)
            rows.append((r, g))
        fresh, states, counts = (np.stack([r[1][i] for r in rows]) for i in (1, 3, 4))
        print(f"{form} lookahead {a}: fresh {int(fresh.sum())} of {fresh.size}, states 0 / 1 / 2 {np.bincount(states.ravel(), minlength=3).tolist()}, "
              f"view_count {np.bincount(counts.ravel(), minlength=V + 1).tolist()}")
        assert fresh.any() and (states == 1).any() and (counts == V).any() and (counts[fresh] < V).any()
        with pytest.raises(ValueError, match="finish in a session with " + ("views" if fps is None else "fps")):     # (the rate is refused first)
            s.finish()
        for x in (ref, s, full):
            assert x.check_range() is False
    finally:
        for x in (ref, s, full):
            x.close()


# ---- 3. the chain to offline ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookahead", [0, 2])
def test_in_phase_the_session_is_the_offline_fusion_of_the_cut_tracks(lookahead):
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg, arch, w, model = _model("h36m_81")
    V, N, ticks, a = 2, 2, 12, lookahead
    cams, _, kp = svu.person_tracks(V, N, ticks, 53)
    views = [[np.ascontiguousarray(kp[:, v * N + i]) for i in range(N)] for v in range(V)]
    poses, fresh, roots, state, count = stream.replay_views(model, cfg, views, cams, resolutions=RES, mask_stride=MS, flip=True, lookahead=a,
                                                            min_root_joints=M)
    checked = solved = 0
    for t in (a, a + 4, a + 8):
        c = t - a
        if not all(f[t] for f in fresh):
            continue
        flat = [tr[:t + 1] for tracks in views for tr in tracks]
        # (batch_size = the session's slots: the forward's bits follow the batch's row count -- tests/test_stream_gpu.py holds the session to
        # predict_tracks' default batches within a tolerance for that reason -- and with the session's own batch shape the lifts are its bits)
        world = predict.predict_tracks(model, cfg, flat, resolutions=RES, mask_stride=MS, flip=True, camera=[x for x in cams for _ in range(N)],
                                       min_root_joints=M, batch_size=V * N)[0]
        vw = np.stack([_host(p[c]) for p in world]).reshape(V, N, J, 3)
        at = kp[c].reshape(V, N, J, 2)
        fused, seen, _ = predict.fuse_views_host(vw, at, None, M)
        want_roots, ok = predict.solve_view_roots_host(fused, at, cams, None, M)
        for i in range(N):
            assert svu.same(poses[i][t], fused[i]) and count[i][t] == seen[i] == V, (t, i)
            assert (state[i][t] == 1) == bool(ok[i]), (t, i)
            if ok[i]:
                assert svu.same(roots[i][t], want_roots[i].astype(np.float32)), (t, i)
                solved += 1
            checked += 1
    print(f"lookahead {a}: {checked} fresh persons checked against the offline rules, {solved} roots solved")
    assert checked >= 2 * N and solved >= 1
