"""GPU: joint rotations (include/uu3d.h, JOINT ROTATIONS) -- uu3d_joint_rotations equals rotations.joint_rotations_host bit for bit
(local, global, flags) on every tree shape and on the degenerate rows; predict_tracks(rotations=...) and StreamSession(rotations=...)
return joint_rotations of the poses they return, bit for bit, and everything else they return is what the call without the keyword
returns; one generic-dims model (J = 13) with a tree and a rest pose of its own."""
import numpy as np
import pytest

from tests.test_rotations_cpu import degenerate_rows
from tests.tracks_util import RES, _bits, _model, _pixel_tracks, _same_bits

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
CAMS = [(1145.0, 1143.5, 512.25, 515.75), (1500.0, 1490.0, 960.0, 540.0)]
ONE = np.array([1.0, 0.0, 0.0, 0.0], np.float32)


def _trees():
    """name -> (Rotations, frame counts): h36m17 at counts that leave the last workgroup (four frames) partial and need several; a
    two-joint tree; a chain of depth 4; the deepest and the widest tree of 64 joints."""
    from uplift_upsample_3dhpe_amd import predict
    rng = np.random.default_rng(20)
    rest = lambda J: rng.normal(size=(J, 3))
    star = [-1] + [0] * 63
    return {"h36m17": (predict.Rotations("h36m17", return_global=True), [1, 3, 65, 130]),
            "two": (predict.Rotations(rest(2), predict.Skeleton([-1, 0])), [7]),
            "chain5": (predict.Rotations(rest(5), predict.Skeleton([-1, 0, 1, 2, 3])), [9]),
            "chain64": (predict.Rotations(rest(64), predict.Skeleton([-1] + list(range(63)))), [6]),
            "star64": (predict.Rotations(rest(64), predict.Skeleton(star), primary={0: 40}, secondary={0: 7}), [6])}


def _equal(got, want, what):
    for name, g, w in zip(("local", "flags", "global"), got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        same = np.array_equal(g, w) if g.dtype == np.uint8 else np.array_equal(_bits(g), _bits(w))
        if not same:
            bad = np.argwhere(g != w)
            print(f"{what} {name}: {len(bad)} elements differ, first at {bad[0].tolist()}: device {g[tuple(bad[0])]!r}, mirror {w[tuple(bad[0])]!r}")
        assert same, (what, name)


@pytest.mark.parametrize("name", ["h36m17", "two", "chain5", "chain64", "star64"])
def test_launch_equals_the_mirror_bit_for_bit(name):
    from uplift_upsample_3dhpe_amd import rotations
    R, counts = _trees()[name]
    J = R.skeleton.joints
    rng = np.random.default_rng(21)
    for G in counts:
        X = rng.normal(size=(G, J, 3)).astype(np.float32)
        got = rotations.joint_rotations(torch.from_numpy(X).cuda(), R, return_global=True)
        assert len(got) == 3
        _equal(got, rotations.joint_rotations_host(X, R, return_global=True), f"{name} G={G}")
    if name == "h36m17":                                              # two outputs without the global ones, the same bits
        two = rotations.joint_rotations(torch.from_numpy(X).cuda(), "h36m17")
        assert len(two) == 2 and _same_bits(two[0], got[0])


def test_degenerate_rows_in_a_batch_and_no_rows():
    from uplift_upsample_3dhpe_amd import rotations
    R, rows = degenerate_rows()
    rng = np.random.default_rng(22)
    X = rng.normal(size=(23, 5, 3)).astype(np.float32)
    X[[1, 4, 5, 9, 13, 17, 22]] = rows                                # among plain rows, across workgroups
    got = rotations.joint_rotations(torch.from_numpy(X).cuda(), R)
    _equal(got, rotations.joint_rotations_host(X, R), "degenerate")
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[2]).all()
    # a row mask leaves the rows it clears as they are
    keep = torch.from_numpy((np.arange(23) % 3 != 0).astype(np.uint8)).cuda()
    out = (torch.full((23, 5, 4), 7.0, device="cuda"), torch.full((23, 5), 9, dtype=torch.uint8, device="cuda"), torch.full((23, 5, 4), 7.0, device="cuda"))
    rotations.joint_rotations(torch.from_numpy(X).cuda(), R, row_mask=keep, out=out)
    k = keep.bool()
    assert _same_bits(out[0][k], got[0][k]) and _same_bits(out[2][k], got[2][k]) and torch.equal(out[1][k], got[1][k])
    assert (out[0][~k] == 7.0).all() and (out[1][~k] == 9).all() and (out[2][~k] == 7.0).all()
    # no rows: nothing is launched
    none = rotations.joint_rotations(torch.zeros((0, 5, 3), device="cuda"), R)
    assert tuple(none[0].shape) == (0, 5, 4) and tuple(none[1].shape) == (0, 5) and tuple(none[2].shape) == (0, 5, 4)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["plain", "bones_smooth_camera"])
def test_predict_tracks_with_rotations(name):
    from uplift_upsample_3dhpe_amd import predict, rotations
    cfg, arch, w, model = _model("h36m_81")
    lens = [60, 45]
    tracks = _pixel_tracks(lens, seed=23)
    kw = dict(mask_stride=4, resolutions=RES[:2])
    if name != "plain":
        kw.update(bones="track", smooth=True, camera=CAMS)
    before = predict.predict_tracks(model, cfg, tracks, **kw)
    got = predict.predict_tracks(model, cfg, tracks, rotations=True, **kw)
    before = before if isinstance(before, tuple) else (before,)
    assert isinstance(got, tuple) and len(got) == len(before) + 1
    for a, b in zip(before, got):                                     # poses (and roots and states): the call without the keyword
        assert len(a) == len(b) == 2 and all(_same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x, y) for x, y in zip(a, b))
    poses, turned = got[0], got[-1]
    assert [tuple(t.shape) for t in turned] == [(n, 17, 4) for n in lens] and all(t.dtype == torch.float32 and t.is_cuda for t in turned)
    for p, t in zip(poses, turned):
        assert _same_bits(t, rotations.joint_rotations(p.contiguous(), "h36m17")[0])
        assert _same_bits(t, rotations.joint_rotations_host(p.cpu().numpy())[0])
    both = predict.predict_tracks(model, cfg, tracks, rotations=predict.Rotations("h36m17", return_global=True), **kw)
    assert len(both) == len(before) + 2 and all(_same_bits(a, b) for a, b in zip(both[-2], turned))
    for p, g in zip(poses, both[-1]):
        assert _same_bits(g, rotations.joint_rotations(p.contiguous(), "h36m17", return_global=True)[2])


def _session_run(model, cfg, ticks, tracks, **kw):
    """Push ``ticks`` frames, reset slot 1 in front of push 30 -> the returned buffers of every push, the buffers right after the reset,
    the rows of finish(), the captures."""
    from uplift_upsample_3dhpe_amd import stream
    s = stream.StreamSession(model, cfg, slots=len(tracks), mask_stride=4, flip=True, graph=True, **kw)
    names = [fn.__name__ for fn, a in s._tick_steps if a is not None]
    per_push, after_reset = [], None
    for k in range(ticks):
        if k == 30:
            s.reset([1])
            after_reset = [t.clone() for t in s._result]
        out = s.push(np.stack([t[k] for t in tracks]))
        assert s.captures == 1
        per_push.append([t.clone() for t in out])
    tail = [t.clone() for t in s.finish()]
    captures = s.captures
    assert s.check_range() is False
    s.close()
    return names, per_push, after_reset, tail, captures


def test_session_with_rotations():
    from uplift_upsample_3dhpe_amd import rotations
    cfg, arch, w, model = _model("h36m_81")
    ticks, a = 50, 4
    tracks = _pixel_tracks([ticks] * 2, seed=24)
    kw = dict(resolutions=RES[:2], lookahead=a)
    names0, plain, _, tail0, captures0 = _session_run(model, cfg, ticks, tracks, **kw)
    names, got, after_reset, tail, captures = _session_run(model, cfg, ticks, tracks, rotations=True, **kw)
    assert names == names0 + ["uu3d_joint_rotations"] and captures == captures0 == 2      # (the tick, and the drain tick of finish)
    previous = np.tile(ONE, (2, 17, 1))
    fresh_seen = np.zeros(2, bool)
    for k, (p, g) in enumerate(zip(plain, got)):
        assert len(g) == len(p) + 1 and all(_same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x, y) for x, y in zip(p, g))
        poses, fresh, turned = g[0], g[1].cpu().numpy(), g[2]
        assert tuple(turned.shape) == (2, 17, 4) and _same_bits(turned, rotations.joint_rotations(poses, "h36m17")[0])
        if k == 30:                                                   # the reset: identities for slot 1 only, on the device
            assert _same_bits(after_reset[2][1], previous[1] * 0 + ONE) and _same_bits(after_reset[2][0], previous[0])
            previous[1] = ONE
        now = turned.cpu().numpy()
        for i in range(2):
            if not fresh[i]:                                          # a row that is not fresh repeats the previous row
                assert _same_bits(now[i], previous[i]), (k, i)
        fresh_seen |= fresh
        previous = now
    assert fresh_seen.all() and not (previous == ONE).all()
    # finish(): the same step in every drain tick
    assert len(tail) == len(tail0) + 1 and all(_same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x, y) for x, y in zip(tail0, tail))
    rows, fresh, turned = tail[0], tail[1].cpu().numpy(), tail[2]
    assert tuple(turned.shape) == (2, a, 17, 4) and fresh.any()
    want = rotations.joint_rotations(rows.reshape(2 * a, 17, 3).contiguous(), "h36m17")[0].reshape(2, a, 17, 4)
    assert _same_bits(turned, want)


def test_generic_model_with_a_tree_of_its_own():
    from tests.test_generic_stream_gpu import _model as generic
    from uplift_upsample_3dhpe_amd import predict, rotations, stream
    cfg, arch, w, model, ms = generic("j13")
    parents = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 8, 10, 8]             # the model's 13 joints: two legs, a spine that forks at joint 8
    R = predict.Rotations(np.random.default_rng(25).normal(size=(13, 3)), predict.Skeleton(parents), primary={0: 7}, secondary={0: 4})
    X = np.random.default_rng(26).normal(size=(10, 13, 3)).astype(np.float32)
    _equal(rotations.joint_rotations(torch.from_numpy(X).cuda(), R), rotations.joint_rotations_host(X, R), "j13")
    with pytest.raises(ValueError, match="Skeleton"):                 # the default skeleton has 17 joints
        stream.StreamSession(model, cfg, slots=2, mask_stride=ms, rotations=True)
    tracks = _pixel_tracks([20] * 2, seed=27, J=13)
    s = stream.StreamSession(model, cfg, slots=2, resolutions=RES[:2], mask_stride=ms, flip=False, lookahead=2, rotations=R)
    seen = 0
    for k in range(20):
        poses, fresh, turned = s.push(np.stack([t[k] for t in tracks]))
        assert s.captures == 1 and _same_bits(turned, rotations.joint_rotations(poses, R)[0])
        seen += int(fresh.sum())
    assert seen > 0 and s.check_range() is False and s.rotation_flags.shape == (2, 13)
    s.close()
