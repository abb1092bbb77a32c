"""CPU: missed detections (frame validity in predict.predict_tracks and stream.StreamSession) without a GPU -- the six C-ABI symbols, the new
Python parameters and their refusals, the two command lines, and the host mirror of uu3d_stream_commit_valid's row rule swept against a
direct statement of the rule on the truncated track:  mask' = mask and (no frame is read or valid[the frame read])."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

from tests import util

SYMBOLS = ("uu3d_normalize_tracks_valid", "uu3d_gather_windows_valid", "uu3d_gather_window_frames_valid", "uu3d_stream_valid_bytes",
           "uu3d_stream_stage_valid", "uu3d_stream_commit_valid")
# (config, SEQUENCE_STRIDE, mask strides)
CASES = [("h36m_81", 2, (4, 8)), ("h36m_351", 5, (5, 10))]
PATTERNS = ("all_valid", "all_missing", "first_missing", "edge_missing", "random30")


def test_symbols_declared_exported_and_refusing():
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    # each is the old call plus its validity pointers
    for new, old, extra in (("uu3d_normalize_tracks_valid", "uu3d_normalize_tracks", 2), ("uu3d_gather_windows_valid", "uu3d_gather_windows", 1),
                            ("uu3d_gather_window_frames_valid", "uu3d_gather_window_frames", 1), ("uu3d_stream_stage_valid", "uu3d_stream_stage", 2),
                            ("uu3d_stream_commit_valid", "uu3d_stream_commit", 2), ("uu3d_stream_valid_bytes", "uu3d_stream_state_bytes", 0)):
        assert len(getattr(lib, new).argtypes) == len(getattr(lib, old).argtypes) + extra, new
    # the structs existing callers construct are untouched
    assert C.sizeof(_capi.Uu3dStreamConfig) == 32 and C.sizeof(_capi.Uu3dStreamLayout) == 56
    # arguments are refused before anything is launched (no device needed)
    bad = _capi.UU3D_ERR_INVALID_ARGUMENT
    cfg = _capi.Uu3dStreamConfig(3, 5, 5, 5, 0, 1, 1, 6)
    assert lib.uu3d_normalize_tracks_valid(None, 1, None, 1, 17, None, 1, None, None, None, 0, None, None, None) == bad
    assert lib.uu3d_gather_windows_valid(None, None, None, None, None, 1, 1, 17, 2, 0, 0, None, None, None, None, None) == bad
    assert lib.uu3d_gather_window_frames_valid(None, None, None, 1, 1, 0, 0, 0, 0, None, None, None, None, None) == bad
    assert lib.uu3d_stream_valid_bytes(None, C.byref(cfg)) == 0
    assert lib.uu3d_stream_stage_valid(None, C.byref(cfg), None, None, None, None, None, None, None, None) == bad
    assert lib.uu3d_stream_commit_valid(None, C.byref(cfg), None, None, None, None, None, None, None, None, None) == bad


def test_the_rule_is_stated_once_on_the_device():
    csrc = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
    misc = open(os.path.join(csrc, "uu3d_misc.h")).read()
    assert len(re.findall(r"__device__ __forceinline__ bool window_token_real\(", misc)) == 1
    assert misc.index("WindowFrame window_frame(") < misc.index("bool window_token_real(")
    code = re.sub(r"//[^\n]*", "", misc)
    assert code.count("window_token_real(") == 3                        # the definition and the two gather kernels
    stream_h = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "uu3d_stream.h")).read())
    assert "window_token_real(" in stream_h and not re.search(r"__device__[^\n]*window_token_real", stream_h)
    for f in ("uu3d_stream.h", "uu3d_tracks.h"):
        assert "atomic" not in re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read()).lower(), f


def test_new_parameters():
    from uplift_upsample_3dhpe_amd import data, predict, stream
    p = inspect.signature(predict.predict_tracks).parameters
    assert p["valid"].default is None and p["return_valid"].default is False
    assert inspect.signature(stream.StreamSession.__init__).parameters["missed_detections"].default is False
    assert inspect.signature(stream.StreamSession.push).parameters["valid"].default is None
    assert inspect.signature(stream.window_plan).parameters["valid"].default is None
    assert inspect.signature(stream.replay_tracks).parameters["valid"].default is None
    assert inspect.signature(data.PoseTable.from_device).parameters["valid"].default is None
    # the old parameters keep their places
    assert list(inspect.signature(stream.StreamSession.push).parameters)[:3] == ["self", "kp2d", "active"]
    assert list(inspect.signature(stream.window_plan).parameters)[:4] == ["frames", "lookahead", "config", "mask_stride"]


def _stub_model(strided=True):
    return types.SimpleNamespace(arch=types.SimpleNamespace(compiled_dims=True), device="cpu", has_strided_input=strided)


def test_refusals_need_no_device():
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg = util.load_config("h36m_81")
    tracks = [np.zeros((9, 17, 2), np.float32), np.zeros((5, 17, 2), np.float32)]
    ok = [np.ones(9, bool), np.ones(5, bool)]
    # a model without strided input has no masked token
    for v in ("finite", ok):
        with pytest.raises(ValueError, match="strided input"):
            predict.predict_tracks(_stub_model(strided=False), cfg, tracks, valid=v)
    with pytest.raises(ValueError, match="strided input"):
        stream.StreamSession(_stub_model(strided=False), cfg, slots=2, missed_detections=True)
    # the list: one entry per track, one flag per given frame
    with pytest.raises(ValueError, match="one entry per track"):
        predict.predict_tracks(_stub_model(), cfg, tracks, valid=ok[:1])
    with pytest.raises(ValueError, match=r"valid\[1\]"):
        predict.predict_tracks(_stub_model(), cfg, tracks, valid=[np.ones(9, bool), np.ones(6, bool)])
    with pytest.raises(ValueError, match=r"valid\[0\]"):
        predict.predict_tracks(_stub_model(), cfg, tracks, valid=[np.ones((9, 1), bool), np.ones(5, bool)])
    with pytest.raises(ValueError, match="valid must be"):
        predict.predict_tracks(_stub_model(), cfg, tracks, valid="all")
    # keyframes_only: the flags are counted in keyframes -- 33 and 17 frames at stride 4 are 9 and 5 keyframes; dense flags are refused
    with pytest.raises(ValueError, match=r"valid\[0\] must be \(9,\)"):
        predict.predict_tracks(_stub_model(), cfg, tracks, mask_stride=4, keyframes_only=True, lengths=[33, 17],
                               valid=[np.ones(33, bool), np.ones(17, bool)])
    predict.check_valid(ok, [9, 5])                                    # (the keyframe counts themselves pass)
    # push(valid=...) on a session built without missed_detections: refused before anything else is looked at
    s = stream.StreamSession.__new__(stream.StreamSession)
    s._torch, s.model, s.missed_detections, s.slots = None, _stub_model(), False, 2
    with pytest.raises(ValueError, match="missed_detections=True"):
        s.push(np.zeros((2, 17, 2), np.float32), valid=[1, 0])
    s._state = None                                                     # (nothing to close)
    with pytest.raises(ValueError, match="one flag per frame"):
        stream.window_plan(9, 0, cfg, 4, valid=np.ones(8, bool))


def _direct_rule(L, c, N, S, s_in, pad_edge, valid):
    """The window of a video of L frames centred on c from the rule itself: token n stands for frame f = c + (n - N // 2) S and is real input
    iff f % s_in == 0; a frame outside the video is replaced by the nearest sampled frame inside it ("copy") or is not read (src -1).  With
    validity a token that reads a frame is real only if that frame is valid."""
    f = c + (np.arange(N) - N // 2) * S
    sampled = np.arange(c % S, L, S)
    inside = (f >= 0) & (f < L)
    src = np.where(inside, f, np.where(f < 0, sampled[0], sampled[-1]) if pad_edge else -1)
    mask = (f % s_in == 0) & ((src < 0) | valid[np.maximum(src, 0)])
    return src, mask


def _pattern(name, L, S, rand):
    v = np.ones(L, bool)
    if name == "all_missing":
        v[:] = False
    elif name == "first_missing":
        v[0] = False
    elif name == "edge_missing":
        v[(L - 1) // S * S] = False                                     # the newest multiple of SEQUENCE_STRIDE: what copy padding repeats
    elif name == "random30":
        v = rand[:L].copy()
    return v


@pytest.mark.parametrize("cfgname,S,strides", CASES)
@pytest.mark.parametrize("padding", ["copy", "zeros"])
def test_row_rule_with_validity_on_the_truncated_track(cfgname, S, strides, padding):
    from uplift_upsample_3dhpe_amd import stream
    cfg = util.load_config(cfgname)
    cfg.PADDING_TYPE = padding
    N = cfg.SEQUENCE_LENGTH
    assert cfg.SEQUENCE_STRIDE == S
    span = (N - 1) * S + 1
    rand = np.random.default_rng(7).random(2 * span + 1) >= 0.3         # seeded, 30 % missing: ONE track, cut to every length
    assert 0.25 < 1.0 - rand.mean() < 0.35
    changed = {p: 0 for p in PATTERNS}
    for s_in in strides:
        for a in (0, S + 1):
            cap = stream.ring_capacity(cfg, s_in, a)
            for t in range(2 * span + 1):
                L, c = t + 1, t - a
                if not stream.emits(L, a, cfg, s_in):
                    assert stream.window_plan(L, a, cfg, s_in, valid=np.ones(L, bool)) is None
                    continue
                base = stream.window_plan(L, a, cfg, s_in)
                for name in PATTERNS:
                    v = _pattern(name, L, S, rand)
                    plan = stream.window_plan(L, a, cfg, s_in, valid=v)
                    src, mask = _direct_rule(L, c, N, S, s_in, padding == "copy", v)
                    assert np.array_equal(plan["mask"], mask), (name, s_in, a, t)
                    assert np.array_equal(plan["src"], np.where(mask, src, -1)), (name, s_in, a, t)
                    # a masked token points nowhere; zero padding is untouched by validity
                    gone = ~plan["mask"]
                    assert (plan["kind"][gone] == 0).all() and (plan["place"][gone] == -1).all() and (plan["src"][gone] == -1).all()
                    assert np.array_equal(plan["kind"] == 1, base["kind"] == 1)
                    # every real token reads a valid frame, and is where the plan without validity has it
                    real = plan["kind"] >= 2
                    assert v[plan["src"][real]].all()
                    for k in ("kind", "place", "src"):
                        assert np.array_equal(plan[k][real], base[k][real])
                    # ring places still never alias
                    ring = plan["kind"] == 2
                    frames, places = plan["src"][ring], plan["place"][ring]
                    assert ((0 <= places) & (places < cap)).all()
                    assert len(set(zip(frames.tolist(), places.tolist()))) == len(set(frames.tolist())) == len(set(places.tolist()))
                    if name == "all_valid":
                        assert all(np.array_equal(plan[k], base[k]) for k in ("mask", "src", "kind", "place"))
                    elif name == "all_missing":
                        assert not (plan["kind"] >= 2).any()
                    changed[name] += int((plan["mask"] != base["mask"]).sum())
    assert changed["all_valid"] == 0 and all(changed[p] > 0 for p in PATTERNS[1:]), changed


def test_copy_padding_source_that_is_missing_masks_the_padded_tokens():
    """h36m_81 at s_in 4, a track of 7 frames (4k + 3), lookahead 0: behind the end copy padding repeats frame 6, the edge row, which is no
    keyframe.  With frame 6 missing every token that would read it is masked; the keyframes 0 and 4 stay."""
    from uplift_upsample_3dhpe_amd import stream
    cfg = util.load_config("h36m_81")
    assert cfg.PADDING_TYPE == "copy" and cfg.SEQUENCE_STRIDE == 2
    base = stream.window_plan(7, 0, cfg, 4)
    assert (base["kind"] == 3).sum() > 0 and (base["src"][base["kind"] == 3] == 6).all()
    v = np.ones(7, bool); v[6] = False
    plan = stream.window_plan(7, 0, cfg, 4, valid=v)
    assert not (plan["kind"] == 3).any() and (plan["kind"][base["kind"] == 3] == 0).all()
    assert sorted(set(plan["src"][plan["kind"] == 2].tolist())) == [0, 4]


def test_predict_cli_mask_missing(tmp_path, monkeypatch):
    from uplift_upsample_3dhpe_amd import predict
    torch = pytest.importorskip("torch")
    inp, outp = str(tmp_path / "tracks.npz"), str(tmp_path / "out.npz")
    walk = np.zeros((11, 17, 2), np.float32); walk[3] = np.nan
    np.savez(inp, walk=walk)
    seen = {}

    def fake_predict(model, config, trs, **kw):
        seen["kw"], seen["tracks"] = kw, trs
        return [torch.zeros((len(t), 17, 3), dtype=torch.float32) for t in trs]
    monkeypatch.setattr(predict, "_load_model", lambda config, weights: object())
    monkeypatch.setattr(predict, "predict_tracks", fake_predict)
    cfg = os.path.join(util.ROOT, "config", "h36m_351.json")
    assert predict.main(["--config", cfg, "--weights", "w.h5", "--input", inp, "--output", outp, "--mask_missing"]) == 0
    assert seen["kw"]["valid"] == "finite" and np.isnan(seen["tracks"][0][3]).all()      # the NaN rows reach predict_tracks as they are
    assert predict.main(["--config", cfg, "--weights", "w.h5", "--input", inp, "--output", outp]) == 0
    assert "valid" not in seen["kw"]


def test_stream_cli_mask_missing(tmp_path, monkeypatch):
    from uplift_upsample_3dhpe_amd import stream
    inp, outp = str(tmp_path / "tracks.npz"), str(tmp_path / "out.npz")
    walk = np.zeros((11, 17, 2), np.float32); walk[3] = np.nan
    np.savez(inp, walk=walk)
    seen = {}

    def fake_replay(model, config, trs, **kw):
        seen["kw"], seen["tracks"] = kw, trs
        return [np.zeros((len(t), 17, 3), np.float32) for t in trs], [np.ones(len(t), bool) for t in trs]
    monkeypatch.setattr(stream, "_load_model", lambda config, weights: object())
    monkeypatch.setattr(stream, "replay_tracks", fake_replay)
    cfg = os.path.join(util.ROOT, "config", "h36m_351.json")
    assert stream.main(["--config", cfg, "--weights", "w.h5", "--input", inp, "--output", outp, "--mask_missing"]) == 0
    assert seen["kw"] == {"resolutions": None, "lookahead": 0, "valid": "finite"} and np.isnan(seen["tracks"][0][3]).all()
    assert stream.main(["--config", cfg, "--weights", "w.h5", "--input", inp, "--output", outp]) == 0
    assert seen["kw"] == {"resolutions": None, "lookahead": 0}
