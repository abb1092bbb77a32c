"""CPU: per-joint missed detections (predict.predict_tracks(valid=..., repair_joints=G); include/uu3d.h, PER-JOINT MISSED DETECTIONS) without a
GPU -- the host mirror predict.repair_joints_host against cases worked out by hand, the argument checks, the command line, the C ABI."""
import inspect
import os
import re
import types

import numpy as np
import pytest

from tests import util

J = 3


def _track(T, joints=J, seed=0):
    """Distinct finite float32 coordinates."""
    return np.random.default_rng(seed).uniform(1.0, 1000.0, size=(T, joints, 2)).astype(np.float32)


def _repair(track, flags, G):
    from uplift_upsample_3dhpe_amd import predict
    rep, fr, st = predict.repair_joints_host([track], None if flags is None else [flags], G)
    assert rep[0].dtype == np.float32 and rep[0].shape == track.shape and fr[0].dtype == bool and fr[0].shape == track.shape[:1]
    assert st[0].dtype == np.uint8 and st[0].shape == track.shape[:2]
    return rep[0], fr[0], st[0]


def _mix(a, b, w):
    return (a.astype(np.float64) * (1.0 - np.float64(w)) + b.astype(np.float64) * np.float64(w)).astype(np.float32)


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def test_a_run_of_G_is_filled_and_a_run_of_G_plus_one_is_not():
    G = 3
    t = _track(12)
    f = np.ones((12, J), bool)
    f[2:5, 0] = False                                                   # a run of exactly G: frames 2, 3, 4 between 1 and 5
    f[6:10, 1] = False                                                  # a run of G + 1: frames 6 .. 9 between 5 and 10
    rep, fr, st = _repair(t, f, G)
    assert list(st[:, 0]) == [1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1]
    assert list(st[:, 1]) == [1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1]
    assert (st[:, 2] == 1).all()
    for k, w in zip((2, 3, 4), (0.25, 0.5, 0.75)):                      # the weights of a 3-frame run, exact in float64
        assert np.float64(k - 1) / np.float64(5 - 1) == w
        assert _bits_equal(rep[k, 0], _mix(t[1, 0], t[5, 0], w))
    assert (rep[6:10, 1] == 0).all()                                    # unrepairable: zeros
    assert _bits_equal(rep[f], t[f])                                    # observed joints keep their bits
    assert list(fr) == [True] * 6 + [False] * 4 + [True] * 2            # a frame with an unrepairable joint is missing


def test_hold_at_the_start_and_at_the_end_within_and_beyond_G():
    G = 2
    t = _track(12)
    f = np.ones((12, J), bool)
    f[:2, 0] = False                                                    # first seen at frame 2: frames 0, 1 held (r - t = 2, 1)
    f[:3, 1] = False                                                    # first seen at frame 3: frame 0 is beyond G, frames 1, 2 held
    f[10:, 0] = False                                                   # last seen at frame 9: frames 10, 11 held
    f[8:, 2] = False                                                    # last seen at frame 7: frames 8, 9 held, 10, 11 beyond G
    rep, fr, st = _repair(t, f, G)
    assert list(st[:, 0]) == [2, 2] + [1] * 8 + [2, 2]
    assert list(st[:, 1]) == [0, 2, 2] + [1] * 9
    assert list(st[:, 2]) == [1] * 8 + [2, 2, 0, 0]
    assert _bits_equal(rep[0, 0], t[2, 0]) and _bits_equal(rep[1, 0], t[2, 0])
    assert _bits_equal(rep[1, 1], t[3, 1]) and _bits_equal(rep[2, 1], t[3, 1]) and (rep[0, 1] == 0).all()
    assert _bits_equal(rep[10, 0], t[9, 0]) and _bits_equal(rep[11, 0], t[9, 0])
    assert _bits_equal(rep[8, 2], t[7, 2]) and _bits_equal(rep[9, 2], t[7, 2]) and (rep[10:, 2] == 0).all()
    assert list(fr) == [False] + [True] * 9 + [False] * 2


def test_a_joint_that_is_never_observed_makes_every_frame_missing():
    t = _track(6)
    f = np.ones((6, J), bool)
    f[:, 1] = False
    f[3, :] = False                                                     # (and one frame with no observed joint at all)
    rep, fr, st = _repair(t, f, 1000)
    assert (st[:, 1] == 0).all() and (rep[:, 1] == 0).all()
    assert not fr.any()
    assert list(st[:, 0]) == [1, 1, 1, 2, 1, 1]                         # the other joints are still repaired


def test_a_frame_without_an_observed_joint_stays_missing_while_fills_span_over_it():
    t = _track(5)
    f = np.ones((5, J), bool)
    f[2, :] = False                                                     # frame 2: nobody found
    f[1, 0] = False                                                     # joint 0 is lost on frames 1 and 2: filled between 0 and 3
    rep, fr, st = _repair(t, f, 2)
    assert list(fr) == [True, True, False, True, True]
    assert list(st[2]) == [2, 2, 2]                                     # every joint of frame 2 has a value ...
    assert list(st[:, 0]) == [1, 2, 2, 1, 1]
    assert _bits_equal(rep[1, 0], _mix(t[0, 0], t[3, 0], 1.0 / 3.0))    # ... and frame 1's fill spans over it
    assert _bits_equal(rep[2, 0], _mix(t[0, 0], t[3, 0], np.float64(2) / np.float64(3)))
    assert _bits_equal(rep[2, 1], _mix(t[1, 1], t[3, 1], 0.5))
    # per-frame flags say the same thing
    rep2, fr2, st2 = _repair(t, f.all(axis=1) | np.array([0, 1, 0, 0, 0], bool), 2)
    assert list(fr2) == [True, True, False, True, True] and list(st2[2]) == [2, 2, 2] and (st2[[0, 1, 3, 4]] == 1).all()


def test_nan_in_one_coordinate_only_and_no_flags():
    t = _track(5)
    src = t.copy()
    src[2, 1, 1] = np.nan                                               # y only
    src[4, 0, 0] = np.inf
    rep, fr, st = _repair(src, None, 1)
    assert st[2, 1] == 2 and st[4, 0] == 2 and (np.delete(st.reshape(-1), [2 * J + 1, 4 * J + 0]) == 1).all()
    assert _bits_equal(rep[2, 1], _mix(t[1, 1], t[3, 1], 0.5))          # both coordinates are replaced, x too
    assert _bits_equal(rep[4, 0], t[3, 0])
    assert np.isfinite(rep).all() and fr.all()


def test_two_tracks_back_to_back_do_not_see_each_other():
    from uplift_upsample_3dhpe_amd import predict
    a, b = _track(4, seed=1), _track(4, seed=2)
    fa, fb = np.ones((4, J), bool), np.ones((4, J), bool)
    fa[2:, 0] = False                                                   # lost at the end of a ...
    fb[:2, 0] = False                                                   # ... and at the start of b: held, never mixed across the boundary
    rep, fr, st = predict.repair_joints_host([a, b], [fa, fb], 1)
    assert list(st[0][:, 0]) == [1, 1, 2, 0] and list(st[1][:, 0]) == [0, 2, 1, 1]
    assert _bits_equal(rep[0][2, 0], a[1, 0]) and _bits_equal(rep[1][1, 0], b[2, 0])
    one, _, st1 = predict.repair_joints_host([np.concatenate([a, b])], [np.concatenate([fa, fb])], 1)
    assert list(st1[0][:, 0]) == [1, 1, 0, 0, 0, 0, 1, 1]               # (as one track the run of 4 is too long for G = 1)
    with pytest.raises(ValueError):
        predict.repair_joints_host([a], [fa], 0)


def test_check_valid_shapes():
    from uplift_upsample_3dhpe_amd import predict
    torch = pytest.importorskip("torch")
    predict.check_valid([np.ones(9, bool), np.ones((5, 17), bool)], [9, 5], joints=17)
    predict.check_valid([torch.ones(9), torch.ones((5, 17), dtype=torch.uint8)], [9, 5], joints=17)
    predict.check_valid("finite", [9, 5], joints=17)
    for bad in (np.ones((5, 16), bool), np.ones((5, 17, 1), bool), np.ones((5, 1), bool), np.ones((6, 17), bool), np.ones((17, 5), bool), np.ones((), bool)):
        with pytest.raises(ValueError, match=r"valid\[1\]"):
            predict.check_valid([np.ones(9, bool), bad], [9, 5], joints=17)
    with pytest.raises(ValueError, match=r"valid\[1\]"):                # without the joint count (a session): per frame only
        predict.check_valid([np.ones(9, bool), np.ones((5, 17), bool)], [9, 5])


def _stub_model(strided=True):
    return types.SimpleNamespace(arch=types.SimpleNamespace(compiled_dims=True), device="cpu", has_strided_input=strided)


def test_repair_joints_argument():
    from uplift_upsample_3dhpe_amd import predict, stream
    p = inspect.signature(predict.predict_tracks).parameters
    assert p["repair_joints"].default is None
    assert "repair_joints" not in inspect.signature(stream.StreamSession.__init__).parameters
    assert "repair_joints" not in inspect.signature(stream.replay_tracks).parameters
    cfg = util.load_config("h36m_81")
    tracks = [np.zeros((9, 17, 2), np.float32), np.zeros((5, 17, 2), np.float32)]
    flags = [np.ones((9, 17), bool), np.ones(5, bool)]
    with pytest.raises(ValueError, match="repair_joints needs valid"):
        predict.predict_tracks(_stub_model(), cfg, tracks, repair_joints=3)
    for bad in (0, -1, 2.0, "3", True):
        with pytest.raises(ValueError, match="repair_joints must be"):
            predict.predict_tracks(_stub_model(), cfg, tracks, valid=flags, repair_joints=bad)
    with pytest.raises(ValueError, match="strided input"):
        predict.predict_tracks(_stub_model(strided=False), cfg, tracks, valid=flags, repair_joints=3)
    with pytest.raises(ValueError, match=r"valid\[0\]"):
        predict.predict_tracks(_stub_model(), cfg, tracks, valid=[np.ones((9, 16), bool), np.ones(5, bool)], repair_joints=3)
    # a session keeps refusing per-joint flags
    with pytest.raises(ValueError, match=r"valid\[0\]"):
        stream.replay_tracks(_stub_model(), cfg, tracks, valid=flags)


def test_command_line(tmp_path, monkeypatch):
    from uplift_upsample_3dhpe_amd import predict
    torch = pytest.importorskip("torch")
    cfg = os.path.join(util.ROOT, "config", "h36m_351.json")
    base = ["--config", cfg, "--weights", "w.h5", "--input", "in.npz", "--output", "out.npz"]
    a = predict.parse_args(base)
    assert a.repair_joints is None and a.min_score is None
    a = predict.parse_args(base + ["--repair_joints", "4", "--min_score", "0.3"])
    assert a.repair_joints == 4 and a.min_score == 0.3
    rng = np.random.default_rng(0)
    scored = rng.uniform(0.0, 1.0, size=(6, 17, 3)).astype(np.float32)
    scored[2, 5, 2] = np.nan
    plain = rng.uniform(0.0, 1.0, size=(4, 17, 2)).astype(np.float32)
    inp, outp = str(tmp_path / "scored.npz"), str(tmp_path / "out.npz")
    np.savez(inp, a=scored, b=plain)
    seen = {}

    def fake_predict(model, config, trs, **kw):
        seen["kw"], seen["tracks"] = kw, trs
        return [torch.zeros((len(t), 17, 3)) for t in trs]
    monkeypatch.setattr(predict, "_load_model", lambda config, weights: object())
    monkeypatch.setattr(predict, "predict_tracks", fake_predict)
    io = ["--config", cfg, "--weights", "w.h5", "--input", inp, "--output", outp]
    with pytest.raises(SystemExit, match=r"\(6, 17, 3\)"):              # a score channel without --min_score is refused as before
        predict.main(io)
    with pytest.raises(SystemExit, match=r"\(6, 17, 3\)"):
        predict.main(io + ["--repair_joints", "2"])
    assert predict.main(io + ["--repair_joints", "2", "--min_score", "0.3"]) == 0
    assert seen["kw"]["repair_joints"] == 2
    assert [t.shape for t in seen["tracks"]] == [(6, 17, 2), (4, 17, 2)] and np.array_equal(seen["tracks"][0], scored[:, :, :2])
    va, vb = seen["kw"]["valid"]
    assert va.shape == (6, 17) and np.array_equal(va, np.nan_to_num(scored[:, :, 2], nan=-1.0) >= np.float32(0.3)) and not va[2, 5]
    assert vb.shape == (4, 17) and vb.all()
    # --repair_joints alone implies --mask_missing
    np.savez(inp, b=plain)
    assert predict.main(io + ["--repair_joints", "5"]) == 0
    assert seen["kw"]["valid"] == "finite" and seen["kw"]["repair_joints"] == 5
    assert predict.main(io + ["--mask_missing"]) == 0
    assert seen["kw"]["valid"] == "finite" and "repair_joints" not in seen["kw"]


def test_c_abi_declared_exported_and_refusing():
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    for s in ("uu3d_repair_joints", "uu3d_repair_joints_scratch_bytes"):
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert header.index("MISSED DETECTIONS") < header.index("int uu3d_repair_joints(") < header.index("int uu3d_resample_tracks(")
    assert lib.uu3d_repair_joints_scratch_bytes(600, 17) == 600 * 17 * 2 * 4
    assert lib.uu3d_repair_joints_scratch_bytes(0, 17) == 0 and lib.uu3d_repair_joints_scratch_bytes(4, 0) == 0
    assert lib.uu3d_repair_joints_scratch_bytes(1 << 31, 17) == 0
    # arguments are refused before anything is launched (no device needed)
    bad = _capi.UU3D_ERR_INVALID_ARGUMENT
    a, b, p = 4096, 8192, 16384                                         # aligned addresses that are never dereferenced
    big = 1 << 20

    def call(src=a, rows=4, J=17, flags=None, start=p, tracks=1, gap=3, out=b, frame=p, state=p, scratch=p, nbytes=big):
        return lib.uu3d_repair_joints(src, rows, J, flags, start, tracks, gap, out, frame, state, scratch, nbytes, None)
    assert lib.uu3d_repair_joints(None, 1, 17, None, None, 1, 1, None, None, None, None, 0, None) == bad
    for drop in ("src", "start", "out", "frame", "state", "scratch"):
        assert call(**{drop: None}) == bad, drop
    assert call(out=a) == bad                                           # src == out
    assert call(rows=0) == bad and call(J=0) == bad and call(tracks=0) == bad and call(gap=0) == bad and call(gap=-1) == bad
    assert call(out=b + 8) == bad and call(src=a + 4) == bad and call(state=p + 1) == bad and call(scratch=p + 2) == bad
    assert call(nbytes=4 * 17 * 2 * 4 - 1) == bad
    assert call(rows=1 << 62) == bad and call(rows=1 << 31) == bad      # the rows * J overflow guard, rows as int32
    assert call(tracks=(1 << 31) - 1, J=128) == bad


def test_kernels_have_one_writer_and_the_mix_is_shared():
    csrc = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "uu3d_repair.h")).read())
    assert "atomic" not in code.lower()
    assert code.count("resample_mix(") == 2 and "resample_mix(" in open(os.path.join(csrc, "uu3d_tracks.h")).read()
    assert "__shfl_up(" in code and "__shfl_down(" in code and "__shared__" in code
