"""GPU: stream.StreamSession on models with generic dims (the frames form of csrc/uu3d_spatial_generic.h + the generic forward's second
stage inside the captured tick) against the session's one rule, the truncation identity of tests/test_stream_gpu.py, at the project's
bar util.TOL_MAX_ABS: predict_tracks on the truncated tracks (the window forward) and the CPU oracle pipeline."""
import numpy as np
import pytest

import uplift_upsample_3dhpe_amd as pkg
from tests import util
from tests.tracks_util import RES, _bits, _oracle_poses, _pixel_tracks, _run

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
T = 3
_MODELS = {}


def _involution(J):
    """Joint 0 stays, the others swap in pairs (an odd joint out stays too): a permutation of range(J) that is its own inverse."""
    order = list(range(J))
    for i in range(1, J - 1, 2):
        order[i], order[i + 1] = i + 1, i
    return order


def _model(name):
    """(config, arch, weights, model, session mask stride) of the test's two generic models, built once."""
    if name not in _MODELS:
        # name: (J, d_s, d_t, heads, the config's mask strides, the session's input stride)
        J, d_s, d_t, heads, ms_cfg, s_in = {"j13": (13, 24, 96, 3, None, None), "j25": (25, 16, 64, 4, [3, 9, 2], 4)}[name]
        cfg = util.load_config("h36m_81")
        cfg.NUM_KEYPOINTS, cfg.SPATIAL_EMBED_DIM, cfg.TEMPORAL_EMBED_DIM, cfg.NUM_HEADS = J, d_s, d_t, heads
        cfg.SEQUENCE_LENGTH, cfg.STRIDES, cfg.PADDINGS, cfg.MLP_RATIO = 27, [3, 3, 3], None, 2.0
        cfg.SPATIAL_TRANSFORMER_BLOCKS, cfg.TEMPORAL_TRANSFORMER_BLOCKS = 2, 2
        cfg.MASK_STRIDE = ms_cfg
        cfg.ROOT_KEYTPOINT = min(int(cfg.ROOT_KEYTPOINT), J - 1)
        cfg.AUGM_FLIP_KEYPOINT_ORDER = _involution(J)
        cfg.BATCH_SIZE = 64
        arch = pkg.arch_from_config(cfg)
        assert not arch.compiled_dims and arch.has_strided_input == (ms_cfg is not None)
        w = pkg.init_weights(arch, seed=2, perturb=0.1)
        _MODELS[name] = (cfg, arch, w, pkg.build_uplift_upsample_transformer(cfg, weights=w), s_in)
    cfg, arch, w, model, s_in = _MODELS[name]
    return cfg.copy(), arch, w, model, s_in


def _checked_ticks(L, a, S, cap, s_in):
    """About a dozen fresh ticks (tests/test_stream_gpu.py): the first ones, the ticks right after the ring wrapped once and twice, some in
    the middle, the last ones."""
    fresh = [t for t in range(L) if t - a >= 0 and (t - a) % S == 0]
    after = lambda f: next(t for t in fresh if t >= f)
    pick = {fresh[0], fresh[1], fresh[4], fresh[len(fresh) // 4], after(cap * s_in), after(cap * s_in + 1), after(2 * cap * s_in),
            after(2 * cap * s_in + s_in), fresh[len(fresh) // 2], fresh[-7], fresh[-2], fresh[-1]}
    return sorted(pick)


@pytest.mark.parametrize("name,a", [("j13", 0), ("j13", 7), ("j25", 0), ("j25", 7)])
def test_truncation_identity(name, a):
    from uplift_upsample_3dhpe_amd import h36m, predict, stream
    cfg, arch, w, model, ms = _model(name)
    assert model.has_frames_form
    S, s_in, pred = stream.session_strides(cfg, ms)
    J, L = arch.num_keypoints, 200
    assert a == 0 or a % S != 0                                         # (a lookahead that is no multiple of the sequence stride)
    tracks = _pixel_tracks([L] * T, seed=11, J=J)
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=a)
    assert s.ring_capacity * s_in < L // 2                              # the ring wraps at least twice
    poses, fresh = _run(s, tracks, L)
    assert s.check_range() is False
    assert s.frames.cpu().tolist() == [L] * T and s.captures == 1
    rule = np.array([stream.emits(t + 1, a, cfg, ms) for t in range(L)])
    assert np.array_equal(rule, np.array([t - a >= 0 and (t - a) % pred == 0 for t in range(L)]))
    assert np.array_equal(fresh, np.repeat(rule[:, None], T, 1))
    prev = np.concatenate([np.zeros_like(poses[:1]), poses[:-1]], 0)
    assert np.array_equal(_bits(poses[~rule]), _bits(prev[~rule])) and not poses[:a].any()
    assert np.isfinite(poses).all() and not poses[:, :, cfg.ROOT_KEYTPOINT].any()
    ticks = _checked_ticks(L, a, pred, s.ring_capacity, s_in)
    assert 9 <= len(ticks) <= 12
    cut = [tracks[i][:t + 1] for t in ticks for i in range(T)]
    res = [RES[i] for t in ticks for i in range(T)]
    centres = np.array([t - a for t in ticks for i in range(T)])
    got = np.stack([poses[t, i] for t in ticks for i in range(T)])
    full = predict.predict_tracks(model, cfg, cut, resolutions=res, mask_stride=ms, flip=True)
    want = np.stack([full[k][c].cpu().numpy() for k, c in enumerate(centres)])
    norm = [h36m.normalize_screen_coordinates(t_, w=r[0], h=r[1]).astype(np.float32) for t_, r in zip(cut, res)]
    orc = _oracle_poses(cfg, arch, w, norm, centres, ms)
    d_pred, d_orc = np.abs(got - want).reshape(len(ticks), -1).max(1), np.abs(got - orc).reshape(len(ticks), -1).max(1)
    print(f"{name} s_in {s_in} lookahead {a}: ticks {ticks}")
    print(f"  max-abs to predict_tracks on the truncated track {d_pred.max():.3e}, to the oracle pipeline {d_orc.max():.3e} (bar {util.TOL_MAX_ABS})")
    assert d_pred.max() <= util.TOL_MAX_ABS and d_orc.max() <= util.TOL_MAX_ABS
    assert float(np.abs(want).max()) > 1e-3                             # (poses, not zeros)
    s.close()


def test_no_cross_talk_between_slots():
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model, ms = _model("j25")
    L, J = 80, arch.num_keypoints
    a_tracks, b_tracks = _pixel_tracks([L] * T, seed=21, J=J), _pixel_tracks([L] * T, seed=22, J=J)
    b_tracks[1] = a_tracks[1]
    out = []
    for tr in (a_tracks, b_tracks):
        s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=3)
        out.append(_run(s, tr, L))
        s.close()
    (pa, fa), (pb, fb) = out
    assert np.array_equal(fa, fb) and fa.any()
    assert np.array_equal(_bits(pa[:, 1]), _bits(pb[:, 1]))              # slot 1: the same bits at every tick
    assert not np.array_equal(_bits(pa[:, 0]), _bits(pb[:, 0])) and not np.array_equal(_bits(pa[:, 2]), _bits(pb[:, 2]))


def test_missed_detections_and_finish_against_the_whole_track():
    """One session on the J = 25 model with missed_detections=True, then finish(): the last push and every drained row are poses of the
    WHOLE track (tests/test_stream_drain_gpu.py: nothing is cut there), so predict_tracks(valid=...) decides them."""
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg, arch, w, model, ms = _model("j25")
    S, s_in, pred = stream.session_strides(cfg, ms)
    L, a, J = 61, 7, arch.num_keypoints
    tracks = _pixel_tracks([L] * T, seed=31, J=J)
    rng = np.random.default_rng(5)
    valid = [rng.random(L) > 0.25 for _ in range(T)]
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=a, missed_detections=True)
    poses, fresh = _run(s, tracks, L, valid=valid)
    rows, rfresh = [o.cpu().numpy() for o in s.finish()]
    assert s.check_range() is False and s.frames.cpu().tolist() == [0] * T
    s.close()
    assert rows.shape == (T, a, J, 3) and rfresh.shape == (T, a)
    whole = predict.predict_tracks(model, cfg, tracks, resolutions=RES, mask_stride=ms, flip=True, valid=valid)
    worst, compared = 0.0, 0
    for i in range(T):
        want = whole[i].cpu().numpy()
        if (L - 1 - a) % pred == 0:
            assert fresh[L - 1, i]
            worst, compared = max(worst, float(np.abs(poses[L - 1, i] - want[L - 1 - a]).max())), compared + 1
        for k in range(1, a + 1):
            c = L - 1 - a + k
            assert bool(rfresh[i, k - 1]) == (c % pred == 0)
            if c % pred == 0:
                worst, compared = max(worst, float(np.abs(rows[i, k - 1] - want[c]).max())), compared + 1
                assert float(np.abs(want[c]).max()) > 1e-3
    print(f"missed detections + finish on the J = 25 model: {compared} rows, max-abs to predict_tracks on the whole track {worst:.3e} (bar {util.TOL_MAX_ABS})")
    assert compared >= T and worst <= util.TOL_MAX_ABS


def _tree25():
    """A tree of 25 joints whose root is the config's ROOT_KEYTPOINT 6: joints 0 .. 5 a chain down from it, the others chains of three."""
    return [j + 1 for j in range(6)] + [-1] + [6 if j % 3 == 1 else j - 1 for j in range(7, 25)]


CAMERAS = [(8.0 * w, 8.0 * w, 0.5 * w, 0.5 * h) for w, h in RES]      # a long lens: solved and held roots mix (tests/test_stream_root_gpu.py)


def test_one_session_with_missed_detections_camera_and_bones():
    """The J = 25 model in one session with missed_detections=True, camera=(...), bones=Bones("track", a tree of 25 joints), then finish().
    Compared as the live tests of those options compare (tests/test_stream_root_gpu.py, tests/test_bones_gpu.py): the live root and the
    "track" mean are CAUSAL, so the references are the rules in numpy, exact on bits -- every tick's raw poses are those of the session
    without the two options, the rebuilt poses stream.LiveBonesHost on them, the roots and states stream.LiveRootHost fed the pushed frames,
    their flags and the rebuilt poses; the rows of finish() follow the same rules.  Where the live rule IS the whole track's -- the raw pose
    of the last push and of every drained row -- predict_tracks(valid=...) decides within TOL_MAX_ABS.  The offline call with the same
    options runs the offline root and bone stages on 25 joints against their host rules."""
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg, arch, w, model, ms = _model("j25")
    S, s_in, pred = stream.session_strides(cfg, ms)
    L, a, J = 61, 7, arch.num_keypoints
    sk = predict.Skeleton(_tree25())
    assert sk.root == int(cfg.ROOT_KEYTPOINT)
    option = predict.Bones("track", sk)
    tracks = _pixel_tracks([L] * T, seed=41, J=J)
    rng = np.random.default_rng(6)
    valid = [rng.random(L) > 0.2 for _ in range(T)]
    common = dict(slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=a, missed_detections=True)
    s = stream.StreamSession(model, cfg, **common)
    plain, plain_fresh = _run(s, tracks, L, valid=valid)
    plain_tail = [o.cpu().numpy() for o in s.finish()]
    s.close()
    s = stream.StreamSession(model, cfg, camera=CAMERAS, bones=option, **common)
    dev = model.device
    grab = {k: torch.zeros((L, T) + shape, dtype=dt, device=dev) for k, shape, dt in (
        ("out", (J, 3), torch.float32), ("raw", (J, 3), torch.float32), ("fresh", (), torch.bool), ("roots", (3,), torch.float32),
        ("state", (), torch.uint8), ("L", (J,), torch.float64))}
    for k in range(L):
        out = s.push(np.stack([t[k] for t in tracks]), valid=np.array([v[k] for v in valid]))
        assert len(out) == 4 and s.captures == 1 and out[0] is s.fixed_poses
        for key, t in (("out", out[0]), ("raw", s.raw_poses), ("fresh", out[1]), ("roots", out[2]), ("state", out[3]), ("L", s.bone_lengths)):
            grab[key][k].copy_(t)
    tail = [t.clone().cpu().numpy() for t in s.finish()]
    tail_raw = s.drain_raw_poses.clone().cpu().numpy()
    assert s.check_range() is False and s.frames.cpu().tolist() == [0] * T
    s.close()
    g = {k: v.cpu().numpy() for k, v in grab.items()}
    # the pushes: raw poses of the plain session; bones and roots by the mirrors, tick by tick
    assert np.array_equal(g["fresh"], plain_fresh) and np.array_equal(_bits(g["raw"]), _bits(plain))
    hb = stream.LiveBonesHost(T, skeleton=sk)
    hr = [stream.LiveRootHost(J, a, CAMERAS[i]) for i in range(T)]
    for k in range(L):
        fixed = hb.step(g["raw"][k], g["fresh"][k])
        assert np.array_equal(_bits(g["out"][k]), _bits(fixed)), (k, np.argwhere(_bits(g["out"][k]) != _bits(fixed))[:3])
        assert np.array_equal(np.ascontiguousarray(g["L"][k]).view(np.uint64), np.ascontiguousarray(hb.lengths).view(np.uint64)), k
        for i in range(T):
            root, state = hr[i].step(tracks[i][k], valid[i][k], fixed[i] if g["fresh"][k, i] else None)
            assert np.array_equal(_bits(g["roots"][k, i]), _bits(root)) and g["state"][k, i] == state, (k, i)
    counts = [int((g["state"] == v).sum()) for v in (0, 1, 2)]
    print(f"J = 25, missed detections + camera + bones: states 0 / 1 / 2 seen {counts}, fresh {int(g['fresh'].sum())} of {g['fresh'].size}")
    assert counts[1] >= 5 and counts[2] >= 5 and not np.array_equal(_bits(g["out"]), _bits(g["raw"]))
    assert not g["out"][:, :, sk.root].any() and np.isfinite(g["out"][a + pred:]).all()
    # finish(): the drained raw rows are the plain session's, the rest by the same mirrors
    assert tail[0].shape == (T, a, J, 3) and np.array_equal(tail[1], plain_tail[1]) and np.array_equal(_bits(tail_raw), _bits(plain_tail[0]))
    for r in range(a):
        fresh = tail[1][:, r]
        fixed = hb.drain(tail_raw[:, r], fresh)
        assert np.array_equal(_bits(tail[0][:, r]), _bits(fixed)), r
        for i in range(T):
            root, state = hr[i].drain(fixed[i] if fresh[i] else None)
            assert np.array_equal(_bits(tail[2][i, r]), _bits(root)) and tail[3][i, r] == state, (r, i)
    assert tail[1].any()
    # where the live rule is the whole track's: the raw pose of the last push and of every fresh drained row
    whole = predict.predict_tracks(model, cfg, tracks, resolutions=RES, mask_stride=ms, flip=True, valid=valid)
    worst, compared = 0.0, 0
    for i in range(T):
        want = whole[i].cpu().numpy()
        rows = [(g["raw"][L - 1, i], L - 1 - a)] if g["fresh"][L - 1, i] else []
        rows += [(tail_raw[i, k - 1], L - 1 - a + k) for k in range(1, a + 1) if tail[1][i, k - 1]]
        for got, c in rows:
            worst, compared = max(worst, float(np.abs(got - want[c]).max())), compared + 1
    print(f"  {compared} whole-track rows: max-abs of the raw poses to predict_tracks {worst:.3e} (bar {util.TOL_MAX_ABS})")
    assert compared >= T and worst <= util.TOL_MAX_ABS
    # the offline call with the same options: bones and roots by the host rules on the call without them
    placed = predict.predict_tracks(model, cfg, tracks, resolutions=RES, mask_stride=ms, flip=True, valid=valid, camera=CAMERAS, bones=option)
    lens = [L] * T
    flat = torch.cat(whole, 0).cpu().numpy()
    fixed = predict.fix_bones_host(flat, lens, predict.bone_lengths_host(flat, lens, sk), sk)
    assert np.array_equal(_bits(torch.cat(placed[0], 0)), _bits(fixed)) and not np.array_equal(_bits(fixed), _bits(flat))
    flags = np.repeat(np.concatenate(valid)[:, None], J, 1)
    roots64, solved = predict.solve_roots_host(fixed, np.concatenate(tracks), CAMERAS, flags=flags, lens=lens)
    want_roots, want_state = predict.root_trajectory_host(roots64, solved, lens, None)
    assert np.array_equal(torch.cat(placed[2], 0).cpu().numpy(), want_state) and (want_state == 1).sum() >= 20
    assert np.array_equal(_bits(torch.cat(placed[1], 0)), _bits(want_roots))


def test_flip_needs_a_permutation_of_the_models_joints():
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model, ms = _model("j25")
    cfg.AUGM_FLIP_KEYPOINT_ORDER = list(util.load_config("h36m_81").AUGM_FLIP_KEYPOINT_ORDER)      # the 17-entry table
    with pytest.raises(ValueError, match=r"permutation of range\(25\)"):
        stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True)
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=False)     # without flip the table is not read
    s.close()
