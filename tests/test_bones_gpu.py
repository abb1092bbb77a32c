"""GPU: constant bone lengths on the device (include/uu3d.h, CONSTANT BONE LENGTHS).  The references are the rules in numpy --
predict.bone_lengths_host / fix_bones_host, stream.LiveBonesHost -- and every comparison with them is exact on bits (the same IEEE float64
operations in the same order, no contraction, a correctly rounded square root).
  1. predict.bone_lengths / fix_bones equal the mirrors: tracks of 1, 2, 3, 65 and 130 rows in one call; J = 17 (the preset), 5 (a chain whose
     children have lower indices than their parents) and 64 (a random tree); "track", given and per-track lengths; a NaN sample, a
     zero-length bone, a track that is NaN throughout; the input is only read
  2. predict_tracks(bones=...) on h36m_81 with seeded weights, tracks of 1, 7 and 101 frames: the poses equal fix_bones_host on the call
     without bones, the roots the root rules on the fixed poses, the filtered output one_euro_host on them
  3. StreamSession(bones=...): every tick's poses equal LiveBonesHost on raw_poses, roots LiveRootHost fed with the fixed poses, the
     filtered output LiveOneEuroHost; finish() rows follow the same rule"""
import numpy as np
import pytest

from tests.tracks_util import RES, _bits, _model, _pixel_tracks, _same_bits

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
LENS = [1, 2, 3, 65, 130]


def _bits64(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _tree(J):
    from uplift_upsample_3dhpe_amd import predict
    if J == 17:
        return predict.SKELETONS["h36m17"]
    if J == 5:
        return predict.Skeleton([1, 2, 3, 4, -1])
    rng = np.random.default_rng(64)
    parents = [-1] + [int(rng.integers(0, j)) for j in range(1, 64)]
    perm = rng.permutation(64)
    mixed = [0] * 64
    for j, p in enumerate(parents):
        mixed[perm[j]] = -1 if p < 0 else int(perm[p])
    return predict.Skeleton(mixed)


def _report_lengths(x, sk, lens, got, want):
    """A differing length: print the operands of the first one, the square roots among them (the one open numerical point)."""
    t, j = np.argwhere(_bits64(got) != _bits64(want))[0]
    first = int(np.sum(lens[:t]))
    rows = x[first:first + lens[t]].astype(np.float64)
    d = rows[:, j] - rows[:, sk.parents[j]]
    q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return (f"track {t} joint {j}: device {got[t, j]!r} ({got[t, j].hex()}) mirror {want[t, j]!r} ({want[t, j].hex()}); sqrt operands "
            f"{[v.hex() for v in q[:4]]} -> numpy {[v.hex() for v in np.sqrt(q[:4])]}")


def _report_poses(x, sk, L, got, want):
    """A differing coordinate: print the bones of its path with their sqrt operands, lengths and scales."""
    r, j, c = np.argwhere(_bits(got) != _bits(want))[0]
    row, lines = x[r].astype(np.float64), []
    for a in sk.paths[j]:
        d = row[a] - row[sk.parents[a]]
        q = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        lines.append(f"bone {a}: sqrt operand {q.hex()} -> {np.sqrt(q).hex()}, L {float(L[r, a]).hex()}, d {[v.hex() for v in d]}")
    return f"row {r} joint {j} coordinate {c}: device {got[r, j, c]!r} mirror {want[r, j, c]!r}; " + "; ".join(lines)


# ---- 1. the launches alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [17, 5, 64])
def test_launches_equal_the_mirrors_bit_for_bit(J):
    from uplift_upsample_3dhpe_amd import predict
    sk = _tree(J)
    rng = np.random.default_rng(J)
    G = sum(LENS)
    x = (rng.normal(size=(G, J, 3)) * rng.uniform(0.05, 2.0, size=(1, J, 1)) + rng.uniform(-3, 3, size=(G, 1, 3))).astype(np.float32)
    child = next(j for j in range(J) if j != sk.root)
    x[30, child, 1] = np.nan                                          # one NaN sample, in the 65-row track
    x[100, child] = x[100, sk.parents[child]]                         # one zero-length bone, in the 130-row track
    x[3:6] = np.nan                                                   # the 3-row track is NaN throughout
    dx = torch.from_numpy(x).cuda()
    before = dx.clone()
    # "track": the lengths, their counts, the fix with them
    want_L, want_N = predict.bone_lengths_host(x, LENS, sk, return_counts=True)
    got_L, got_N = predict.bone_lengths(dx, LENS, sk, return_counts=True)
    assert got_L.dtype == torch.float64 and tuple(got_L.shape) == (len(LENS), J) and got_N.dtype == torch.int64
    h_L = got_L.cpu().numpy()
    assert np.array_equal(_bits64(h_L), _bits64(want_L)), _report_lengths(x, sk, LENS, h_L, want_L)
    assert np.array_equal(got_N.cpu().numpy(), want_N)
    assert np.isnan(np.delete(want_L[2], sk.root)).all() and want_L[2, sk.root] == 0.0 and want_N[3, child] == 64 and want_N[4, child] == 129
    want = predict.fix_bones_host(x, LENS, want_L, sk)
    got = predict.fix_bones(dx, LENS, got_L, sk)
    assert got.dtype == torch.float32 and tuple(got.shape) == (G, J, 3) and got.data_ptr() != dx.data_ptr()
    rows_L = np.repeat(want_L, LENS, axis=0)
    assert np.array_equal(_bits(got), _bits(want)), _report_poses(x, sk, rows_L, got.cpu().numpy(), want)
    assert np.isnan(want[3:6]).all() and np.isnan(want[30]).any() and np.array_equal(_bits(want[:, sk.root]), _bits(x[:, sk.root]))
    assert not np.array_equal(_bits(want[6:30]), _bits(x[6:30]))      # (and the fix does something)
    # given lengths: one table for all tracks, one per track (with entries that mean "not corrected"), one track without lens
    one = rng.uniform(0.1, 0.8, J)
    per = rng.uniform(0.1, 0.8, (len(LENS), J))
    per[1, child], per[3, child], per[4, child] = np.nan, 0.0, -2.0
    for lengths, lens in ((one, LENS), (per, LENS), (one, None), (torch.from_numpy(per).cuda(), LENS)):
        host = lengths.cpu().numpy() if isinstance(lengths, torch.Tensor) else lengths
        want = predict.fix_bones_host(x, lens, host, sk)
        got = predict.fix_bones(dx, lens, lengths, sk)
        table = np.repeat(np.broadcast_to(host, (len(LENS) if lens else 1, J)), lens or [G], axis=0)
        assert np.array_equal(_bits(got), _bits(want)), _report_poses(x, sk, table, got.cpu().numpy(), want)
    assert np.array_equal(_bits64(predict.bone_lengths(dx, None, sk)), _bits64(predict.bone_lengths_host(x, None, sk)))
    assert torch.equal(before.view(torch.int32), dx.view(torch.int32))           # only read
    with pytest.raises(ValueError):
        predict.bone_lengths(dx, [G - 1], sk)
    with pytest.raises(ValueError):
        predict.fix_bones(dx, LENS, np.ones(J + 1), sk)
    with pytest.raises(ValueError):
        predict.fix_bones(dx, LENS, torch.ones((len(LENS), J), dtype=torch.float32, device="cuda"), sk)
    with pytest.raises(ValueError):
        predict.fix_bones(dx[:, :, :2], LENS, one, sk)
    with pytest.raises(ValueError, match="Skeleton"):
        predict.bone_lengths(dx[:, :J - 1].contiguous(), LENS, sk)


# ---- 2. predict_tracks -------------------------------------------------------------------------------------------------------------------
TRACK_LENS = [1, 7, 101]
CAMS = [(1145.0, 1143.8, 512.5, 515.5), (1400.0, 1390.0, 960.0, 540.0), (600.0, 610.0, 320.0, 240.0)]


def _far_tracks(lens, seed, J=17):
    """People far from the camera, in pixels (tests/test_smooth_gpu.py): solved and unsolved frames mix whatever the weights."""
    rng = np.random.default_rng(seed)
    tracks = []
    for i, n in enumerate(lens):
        centre = rng.uniform(0.3, 0.7, size=2) * RES[i % len(RES)] + np.arange(n)[:, None] * np.array([1.5, 0.5])
        tracks.append((centre[:, None, :] + rng.uniform(-4.0, 4.0, size=(n, J, 2))).astype(np.float32))
    return tracks


@pytest.mark.parametrize("bones", ["track", "given"])
@pytest.mark.parametrize("name", ["plain", "keyframes", "fps30_out60", "camera", "camera_smooth", "fps30_out60_camera"])
def test_predict_tracks_with_bones(name, bones):
    from fractions import Fraction
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    tracks, kw, rate = _far_tracks(TRACK_LENS, seed=91), {"mask_stride": 4}, 50
    given_frames = tracks
    if name == "keyframes":
        given_frames = tracks = [t[::4] for t in tracks]
        kw.update(keyframes_only=True, lengths=TRACK_LENS)
    elif name.startswith("fps30_out60"):
        kw.update(fps=30, out_fps=60)
        rate = 60
    placed = "camera" in name
    kw["resolutions"] = [RES[i % len(RES)] for i in range(len(tracks))]
    if placed:
        kw["camera"] = CAMS
    P, R = predict.OneEuro(1.2, 0.8, 1.0), predict.OneEuro(0.4, 0.3, 2.0)
    if name == "camera_smooth":
        kw["smooth"] = (P, R)
    rng = np.random.default_rng(92)
    lengths = [rng.uniform(0.1, 0.5, 17) for _ in tracks]
    lengths[1][9], lengths[2][12] = np.nan, 0.0                       # "not corrected"
    raw = predict.predict_tracks(model, cfg, tracks, **{k: v for k, v in kw.items() if k != "smooth"})
    got = predict.predict_tracks(model, cfg, tracks, bones="track" if bones == "track" else lengths, **kw)
    raw_poses, got_poses = (raw[0], got[0]) if placed else (raw, got)
    lens = [int(p.shape[0]) for p in raw_poses]
    assert [int(p.shape[0]) for p in got_poses] == lens
    flat = torch.cat(raw_poses, 0).cpu().numpy()
    L = predict.bone_lengths_host(flat, lens) if bones == "track" else np.stack(lengths)
    fixed = predict.fix_bones_host(flat, lens, L)
    assert not np.array_equal(_bits(fixed), _bits(flat)) and not fixed[:, int(cfg.ROOT_KEYTPOINT)].any()
    want = predict.one_euro_host(fixed, lens, rate, P) if name == "camera_smooth" else fixed
    assert np.array_equal(_bits(torch.cat(got_poses, 0)), _bits(want)), np.argwhere(_bits(torch.cat(got_poses, 0)) != _bits(want))[:5]
    if placed:
        given = [len(t) for t in given_frames]
        kp2d = np.concatenate(given_frames)
        at_given, where = fixed, None
        if name == "fps30_out60_camera":                              # the motion read at the given frames' times: the call with fps alone
            at30 = predict.predict_tracks(model, cfg, tracks, mask_stride=4, fps=30, resolutions=kw["resolutions"])
            at_given = predict.fix_bones_host(torch.cat(at30, 0).cpu().numpy(), given, L)
            where = predict.given_positions(lens, [Fraction(30, 60)] * len(given))
        roots64, solved = predict.solve_roots_host(at_given, kp2d, CAMS, lens=given)
        want_roots, want_state = predict.root_trajectory_host(roots64, solved, given, where)
        assert np.array_equal(torch.cat(got[2], 0).cpu().numpy(), want_state) and (want_state != 0).sum() > 20
        if name == "camera_smooth":
            want_roots = predict.one_euro_host(want_roots, lens, rate, R, state=want_state)
        assert np.array_equal(_bits(torch.cat(got[1], 0)), _bits(want_roots))
        assert not np.array_equal(_bits(torch.cat(got[1], 0)), _bits(torch.cat(raw[1], 0)))     # the depth follows the bones
    if name == "plain":
        again = predict.predict_tracks(model, cfg, tracks, bones=None, **kw)
        assert all(_same_bits(a, b) for a, b in zip(again, raw_poses))
        if bones == "given":                                          # one (J,) table for every track; another tree through Bones
            one = predict.predict_tracks(model, cfg, tracks, bones=lengths[0], **kw)
            assert np.array_equal(_bits(torch.cat(one, 0)), _bits(predict.fix_bones_host(flat, lens, lengths[0])))
            star = predict.Skeleton([6] * 6 + [-1] + [6] * 10)
            other = predict.predict_tracks(model, cfg, tracks, bones=predict.Bones(lengths[0], star), **kw)
            assert np.array_equal(_bits(torch.cat(other, 0)), _bits(predict.fix_bones_host(flat, lens, lengths[0], star)))
            with pytest.raises(ValueError, match="ROOT_KEYTPOINT"):
                predict.predict_tracks(model, cfg, tracks, bones=predict.Bones("track", predict.Skeleton([-1] + [0] * 16)), **kw)


def test_predict_detections_hands_bones_on():
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    rng = np.random.default_rng(93)
    body = rng.uniform(-60.0, 60.0, size=(17, 2))
    T = 9
    dets = np.zeros((T, 2, 17, 2), np.float32)
    for k in range(T):
        rows = [body + np.array([300.0 + 3 * k, 300.0]) + rng.uniform(-2, 2, (17, 2)), body + np.array([1400.0, 700.0 - 2 * k]) + rng.uniform(-2, 2, (17, 2))]
        dets[k] = rows[::-1] if k % 2 else rows
    kw = dict(slots=2, resolutions=(1920, 1080), mask_stride=4)
    plain = predict.predict_detections(model, cfg, [dets], **kw)
    got = predict.predict_detections(model, cfg, [dets], bones="track", **kw)
    assert len(got[0]) == len(plain[0]) == 2
    for (tid, first, p), (tid2, first2, q) in zip(plain[0], got[0]):
        assert (tid, first) == (tid2, first2)
        flat = p.cpu().numpy()
        assert np.array_equal(_bits(q), _bits(predict.fix_bones_host(flat, None, predict.bone_lengths_host(flat))))


# ---- 3. sessions ---------------------------------------------------------------------------------------------------------------------------
S, J17, MS, TICKS = 3, 17, 4, 12
CAMERAS = [(8.0 * w, 8.0 * w, 0.5 * w, 0.5 * h) for w, h in RES]


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("bones", ["track", "given"])
@pytest.mark.parametrize("lookahead", [0, 2])
def test_session_with_bones(lookahead, bones, smooth):
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg, arch, w, model = _model("h36m_81")
    P, R = predict.OneEuro(1.2, 0.8, 1.0), predict.OneEuro(0.4, 0.3, 2.0)
    rng = np.random.default_rng(94)
    lengths = rng.uniform(0.1, 0.5, (S, J17))
    lengths[0, 9], lengths[2, 12] = np.nan, 0.0
    tracks = _pixel_tracks([TICKS] * S, seed=95)
    common = dict(slots=S, resolutions=RES, mask_stride=MS, flip=True, lookahead=lookahead, camera=CAMERAS)
    s = stream.StreamSession(model, cfg, **common)
    steps = [fn.__name__ for fn, a in s._tick_steps if a is not None]
    s.close()
    option = "track" if bones == "track" else list(lengths)
    s = stream.StreamSession(model, cfg, bones=option, **(dict(smooth=(P, R)) if smooth else {}), **common)
    names = [fn.__name__ for fn, a in s._tick_steps if a is not None]
    assert names == steps[:-1] + ["uu3d_stream_bones", "uu3d_stream_root"] + ["uu3d_stream_one_euro"] * (2 * smooth)
    dev = model.device
    grab = {k: torch.zeros((TICKS, S) + shape, dtype=dt, device=dev) for k, shape, dt in (
        ("out", (J17, 3), torch.float32), ("raw", (J17, 3), torch.float32), ("fixed", (J17, 3), torch.float32), ("fresh", (), torch.bool),
        ("roots", (3,), torch.float32), ("state", (), torch.uint8), ("raw_roots", (3,), torch.float32), ("frames", (), torch.int32),
        ("L", (J17,), torch.float64))}
    active = [np.array([True, True, not 4 <= k < 7]) for k in range(TICKS)]           # slot 2 pauses for three ticks
    for k in range(TICKS):
        if k == 6:
            s.reset([1])
        out = s.push(np.stack([tracks[i][k] for i in range(S)]), active[k])
        assert len(out) == 4 and s.captures == 1
        for key, t in (("out", out[0]), ("raw", s.raw_poses), ("fixed", s.fixed_poses), ("fresh", out[1]), ("roots", out[2]), ("state", out[3]),
                       ("raw_roots", s.raw_roots), ("frames", s.source_frames), ("L", s.bone_lengths)):
            grab[key][k].copy_(t)
    assert s.captures == 1 and (smooth or out[0] is s.fixed_poses) and s.raw_poses is not s.fixed_poses
    chosen = [0, 2]
    tail = [t.clone() for t in s.finish(chosen)]
    tail_raw, tail_fixed, tail_raw_roots = s.drain_raw_poses.clone(), s.drain_fixed_poses.clone(), s.drain_raw_roots.clone()
    assert s.check_range() is False and s.captures == (2 if lookahead else 1)
    s.close()
    g = {k: v.cpu().numpy() for k, v in grab.items()}
    tail = [t.cpu().numpy() for t in tail]
    tail_raw, tail_fixed, tail_raw_roots = tail_raw.cpu().numpy(), tail_fixed.cpu().numpy(), tail_raw_roots.cpu().numpy()
    assert (g["fresh"].sum(axis=0) >= 3).all()                        # (12 ticks, every 2nd frame predicted, lookahead <= 2, a pause or a reset)
    # the mirrors, tick by tick
    hb = stream.LiveBonesHost(S, lengths=None if bones == "track" else lengths)
    hr = [stream.LiveRootHost(J17, lookahead, CAMERAS[i]) for i in range(S)]
    hp, hq = stream.LiveOneEuroHost(S, 3 * J17, 50, P, lookahead), stream.LiveOneEuroHost(S, 3, 50, R, lookahead)
    for k in range(TICKS):
        if k == 6:
            hb.reset([1]), hr[1].reset(), hp.reset([1]), hq.reset([1])
        fixed = hb.step(g["raw"][k], g["fresh"][k], active[k])
        assert np.array_equal(_bits(g["fixed"][k]), _bits(fixed)), (k, np.argwhere(_bits(g["fixed"][k]) != _bits(fixed))[:3])
        assert np.array_equal(_bits64(g["L"][k]), _bits64(hb.lengths)), k
        for i in range(S):
            if active[k][i]:
                root, state = hr[i].step(tracks[i][k], None, fixed[i] if g["fresh"][k, i] else None)
            else:
                root, state = hr[i].root, hr[i].state
            assert np.array_equal(_bits(g["raw_roots"][k, i]), _bits(root)) and g["state"][k, i] == state, (k, i)
        if smooth:
            assert np.array_equal(_bits(g["out"][k]), _bits(hp.step(fixed.reshape(S, -1), g["frames"][k], g["fresh"][k], active[k]).reshape(S, J17, 3))), k
            assert np.array_equal(_bits(g["roots"][k]), _bits(hq.step(g["raw_roots"][k], g["frames"][k], g["fresh"][k], active[k], g["state"][k]))), k
        else:
            assert np.array_equal(_bits(g["out"][k]), _bits(fixed)) and np.array_equal(_bits(g["roots"][k]), _bits(g["raw_roots"][k]))
    assert (g["state"] == 1).any() and not np.array_equal(_bits(g["fixed"]), _bits(g["raw"]))
    # finish(): the same step in every drain tick, the chosen slots as `active`
    assert tail[0].shape == (S, lookahead, J17, 3) and not tail[0][1].any() and not tail[1][1].any()
    mask = np.zeros(S, bool)
    mask[chosen] = True
    for r in range(lookahead):
        fresh = tail[1][:, r]
        fixed = hb.drain(tail_raw[:, r], fresh, mask)
        for i in chosen:
            assert np.array_equal(_bits(tail_fixed[i, r]), _bits(fixed[i])), (r, i)
            root, state = hr[i].drain(fixed[i] if fresh[i] else None)
            assert np.array_equal(_bits(tail_raw_roots[i, r]), _bits(root)) and tail[3][i, r] == state
        if smooth:
            values = np.where(mask[:, None, None], tail_fixed[:, r], g["fixed"][-1])
            want = hp.drain(values.reshape(S, -1), g["frames"][-1], np.where(mask, r + 1, 0), fresh, mask).reshape(S, J17, 3)
            roots_in = np.where(mask[:, None], tail_raw_roots[:, r], g["raw_roots"][-1])
            want_r = hq.drain(roots_in, g["frames"][-1], np.where(mask, r + 1, 0), fresh, mask, np.where(mask, tail[3][:, r], g["state"][-1]))
            for i in chosen:
                assert np.array_equal(_bits(tail[0][i, r]), _bits(want[i])) and np.array_equal(_bits(tail[2][i, r]), _bits(want_r[i])), (r, i)
        else:
            for i in chosen:
                assert np.array_equal(_bits(tail[0][i, r]), _bits(fixed[i])) and np.array_equal(_bits(tail[2][i, r]), _bits(tail_raw_roots[i, r]))
    if lookahead:
        assert tail[1][chosen].any()


def test_session_refusals_and_without_bones():
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    with pytest.raises(ValueError, match="bones together with out_fps"):
        stream.StreamSession(model, cfg, slots=S, mask_stride=MS, lookahead=40, fps=25, out_fps=50, bones="track")
    s = stream.StreamSession(model, cfg, slots=S, resolutions=RES, mask_stride=MS, flip=True, bones=None)
    try:
        out = s.push(np.zeros((S, J17, 2), np.float32))
        assert len(out) == 2 and len(s._tick_steps) == 5 and s._push_after == [] and s._reset_more == [] and out[0] is s.raw_poses
        for name in ("bone_lengths", "fixed_poses"):
            with pytest.raises(AttributeError):
                getattr(s, name)
    finally:
        s.close()


def test_replay_tracks_hands_bones_on():
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg, arch, w, model = _model("h36m_81")
    tracks = _pixel_tracks([9, 6], seed=96)
    kw = dict(resolutions=RES[:2], mask_stride=MS, lookahead=1, drain=True)
    plain_p, plain_f = stream.replay_tracks(model, cfg, tracks, **kw)
    got_p, got_f = stream.replay_tracks(model, cfg, tracks, bones="track", **kw)
    for i in range(2):
        assert np.array_equal(plain_f[i], got_f[i])
        h = stream.LiveBonesHost(1)
        for k in range(len(plain_p[i])):
            want = h.step(plain_p[i][k][None], plain_f[i][k:k + 1])[0]
            assert np.array_equal(_bits(got_p[i][k]), _bits(want)), (i, k)
