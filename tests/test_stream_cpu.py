"""CPU: the parts of stream.StreamSession that need no GPU -- the host mirror of uu3d_stream_commit's row rule against the window rules on
the truncated track (eval.window_frames and a direct restatement), the ring capacity, the C-ABI symbols and the constructor's refusals."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from tests import util

SYMBOLS = ("uu3d_stream_state_bytes", "uu3d_stream_state_layout", "uu3d_stream_stage", "uu3d_stream_commit", "uu3d_stream_emit",
           "uu3d_stream_reset")
# (config, padding types, mask strides: equal to SEQUENCE_STRIDE and greater than it, lookaheads: none, one that is no multiple of the
#  sequence stride, the largest)
CASES = [("h36m_81", 2, (2, 4, 10)), ("h36m_351", 5, (5, 10, 20))]


def _direct_rule(L, c, N, S, s_in, pad_edge):
    """The window of a video of L frames centred on c, token by token, from the rule itself: token n stands for frame f = c + (n - N // 2) S;
    it is real input iff f % s_in == 0; a frame outside the video is replaced by the nearest sampled frame inside it ("copy") or by zeros."""
    sampled = [f for f in range(c % S, L, S)]
    src, mask = [], []
    for n in range(N):
        f = c + (n - N // 2) * S
        mask.append(f % s_in == 0)
        if 0 <= f < L:
            src.append(f)
        elif pad_edge:
            src.append(min(sampled) if f < 0 else max(sampled))
        else:
            src.append(-1)
    return np.array(src), np.array(mask)


@pytest.mark.parametrize("cfgname,S,strides", CASES)
@pytest.mark.parametrize("padding", ["copy", "zeros"])
def test_row_rule_equals_the_window_rules_on_the_truncated_track(cfgname, S, strides, padding):
    from uplift_upsample_3dhpe_amd import eval as ev
    from uplift_upsample_3dhpe_amd import stream
    cfg = util.load_config(cfgname)
    cfg.PADDING_TYPE = padding
    N = cfg.SEQUENCE_LENGTH
    assert cfg.SEQUENCE_STRIDE == S and cfg.TEST_STRIDED_EVAL is True
    span = (N - 1) * S + 1
    amax = stream.max_lookahead(cfg)
    assert amax == (N // 2) * S
    for s_in in strides:
        for a in (0, S + 1, amax):
            cap = stream.ring_capacity(cfg, s_in, a)
            assert cap == (a + amax) // s_in + 1
            emitted = 0
            for t in range(3 * span + 1):
                L = t + 1
                plan = stream.window_plan(L, a, cfg, s_in)
                c = t - a
                assert (plan is not None) == (c >= 0 and c % S == 0) == stream.emits(L, a, cfg, s_in)
                if plan is None:
                    continue
                emitted += 1
                assert plan["centre"] == c
                src, mask = _direct_rule(L, c, N, S, s_in, padding == "copy")
                assert np.array_equal(plan["mask"], mask)
                want = np.where(mask, src, -1)                       # a masked token reads nothing
                assert np.array_equal(plan["src"], want), (s_in, a, t)
                assert np.array_equal(plan["kind"] == 0, ~mask) and np.array_equal(plan["kind"] == 1, mask & (src < 0))
                # the same window by the host restatement of the gather kernels: the set of frames read, and whether the zero row is
                desc = np.array([[0, c, S, s_in, c, 0]])
                read, _, zero = ev.window_frames(desc, N, [0], [L], padding == "copy")
                assert np.array_equal(np.unique(plan["src"][plan["src"] >= 0]), read)
                assert zero == bool((plan["kind"] == 1).any())
                # ring: only keyframes, every place holds one frame of this window, and that frame is the newest keyframe filed there
                ring = plan["kind"] == 2
                frames, places = plan["src"][ring], plan["place"][ring]
                assert (frames % s_in == 0).all() and ((0 <= places) & (places < cap)).all()
                assert len(set(zip(frames.tolist(), places.tolist()))) == len(set(frames.tolist())) == len(set(places.tolist()))
                newest_key = t // s_in * s_in
                for f, p in zip(frames.tolist(), places.tolist()):
                    assert f <= newest_key and f + cap * s_in > newest_key        # not yet overwritten by a later keyframe of the same place
                    assert p == (f // s_in) % cap
                # edge: the frame copy padding repeats behind the end, the newest multiple of the sequence stride
                edge = plan["kind"] == 3
                assert (plan["src"][edge] == t // S * S).all()
                if padding == "zeros":
                    assert not edge.any()
            assert emitted > 2 * (N - 1)
    # s_in > SEQUENCE_STRIDE: the edge frame is not always a keyframe -- the ring alone would not do
    if padding == "copy":
        s_in = strides[1]
        seen = [stream.window_plan(L, 0, cfg, s_in) for L in range(1, 4 * s_in + 2)]
        assert any(p is not None and ((p["kind"] == 3) & (p["src"] % s_in != 0)).any() for p in seen)


def test_symbols_declared_exported_and_refusing():
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert "uu3d_stream.h" in open(os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc", "uu3d_api.hip")).read()
    # the two structs as the header lays them out: 8 int32, 7 int64
    assert C.sizeof(_capi.Uu3dStreamConfig) == 32 and C.sizeof(_capi.Uu3dStreamLayout) == 56
    assert [f for f, _ in _capi.Uu3dStreamConfig._fields_] == re.search(r"typedef struct uu3d_stream_config \{\s*int32_t ([^;]*);", header).group(1) \
        .replace("/* 1 = \"copy\" padding */", "").replace("/* < 0: absolute */", "").replace(" ", "").split(",")
    assert [f for f, _ in _capi.Uu3dStreamLayout._fields_] == re.search(r"typedef struct uu3d_stream_layout \{ int64_t ([^;]*);", header).group(1) \
        .replace(" ", "").split(",")
    assert len(lib.uu3d_stream_stage.argtypes) == 8 and len(lib.uu3d_stream_commit.argtypes) == 9
    assert len(lib.uu3d_stream_emit.argtypes) == 8 and len(lib.uu3d_stream_reset.argtypes) == 5
    # arguments are refused before anything is launched (no device needed)
    cfg = _capi.Uu3dStreamConfig(3, 5, 5, 5, 0, 1, 1, 6)
    lay = _capi.Uu3dStreamLayout()
    assert lib.uu3d_stream_state_bytes(None, C.byref(cfg)) == 0
    assert lib.uu3d_stream_state_layout(None, C.byref(cfg), C.byref(lay)) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_stream_stage(None, C.byref(cfg), None, None, None, None, None, None) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_stream_commit(None, C.byref(cfg), None, None, None, None, None, None, None) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_stream_emit(None, C.byref(cfg), None, None, None, None, None, None) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_stream_reset(None, C.byref(cfg), None, None, None) == _capi.UU3D_ERR_INVALID_ARGUMENT


def test_source_has_no_atomics_and_shares_the_helpers():
    csrc = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
    text = open(os.path.join(csrc, "uu3d_stream.h")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert "atomic" not in code.lower()
    # the frame / mask rules, the normalisation and the un-flip are the shared device helpers, not restated
    assert "window_frame(" in code and "normalize_pair(" in code and "window_prediction(" in code
    for helper, home in (("window_frame", "uu3d_misc.h"), ("normalize_pair", "uu3d_tracks.h"), ("window_prediction", "uu3d_tracks.h")):
        assert re.search(r"__device__ __forceinline__ \w+ " + helper + r"\(", open(os.path.join(csrc, home)).read()), helper
        assert not re.search(r"__device__[^\n]*\b" + helper + r"\(", code), helper


def _stub_model(compiled=True):
    return types.SimpleNamespace(arch=types.SimpleNamespace(compiled_dims=compiled), device="cpu")


def test_constructor_refusals_need_no_device():
    import uplift_upsample_3dhpe_amd as pkg
    from uplift_upsample_3dhpe_amd import stream
    assert pkg.StreamSession is stream.StreamSession
    cfg = util.load_config("h36m_351")
    amax = (cfg.SEQUENCE_LENGTH // 2) * cfg.SEQUENCE_STRIDE
    for a in (-1, amax + 1):
        with pytest.raises(ValueError, match="lookahead"):
            stream.StreamSession(_stub_model(), cfg, slots=2, lookahead=a)
    for res in ((0, 1080), (1920, -1), [(1920, 1080), (640, 0)], [(1920, 1080)] * 3, (float("nan"), 5)):
        with pytest.raises(ValueError, match="resolutions"):
            stream.StreamSession(_stub_model(), cfg, slots=2, resolutions=res)
    with pytest.raises(NotImplementedError, match="generic dims"):
        stream.StreamSession(_stub_model(compiled=False), cfg, slots=2, resolutions=(1920, 1080), lookahead=amax)
    with pytest.raises(ValueError, match="slots"):
        stream.StreamSession(_stub_model(), cfg, slots=0)
    with pytest.raises(ValueError, match="multiple of the sequence stride"):
        stream.StreamSession(_stub_model(), cfg, slots=1, mask_stride=7)


def test_cli_replays_an_npz_tick_by_tick(tmp_path, monkeypatch, capsys):
    from uplift_upsample_3dhpe_amd import stream
    rng = np.random.default_rng(0)
    tracks = {"walk": rng.normal(size=(23, 17, 2)).astype(np.float32), "sit": rng.normal(size=(7, 17, 2)).astype(np.float32)}
    inp, outp = str(tmp_path / "tracks.npz"), str(tmp_path / "out.npz")
    np.savez(inp, **tracks)
    seen = {}

    def fake_replay(model, config, trs, **kw):
        seen["kw"], seen["tracks"] = kw, trs
        return ([np.full((len(t), 17, 3), float(i), np.float32) for i, t in enumerate(trs)],
                [np.arange(len(t)) % 5 == 0 for t in trs])
    monkeypatch.setattr(stream, "_load_model", lambda config, weights: seen.setdefault("weights", weights))
    monkeypatch.setattr(stream, "replay_tracks", fake_replay)
    cfg = os.path.join(util.ROOT, "config", "h36m_351.json")
    assert stream.main(["--config", cfg, "--weights", "w.h5", "--input", inp, "--output", outp, "--lookahead", "7", "--resolution", "1920", "1080"]) == 0
    assert seen["weights"] == "w.h5" and seen["kw"] == {"resolutions": (1920.0, 1080.0), "lookahead": 7}
    with np.load(outp) as z:
        assert sorted(z.files) == ["sit", "sit_fresh", "walk", "walk_fresh"]
        assert z["walk"].shape == (23, 17, 3) and z["walk"].dtype == np.float32 and z["sit_fresh"].dtype == bool and z["sit_fresh"].sum() == 2
    assert "2 tracks, 30 ticks, 7 fresh poses" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        stream.main(["--config", cfg, "--weights", "w.h5", "--input", inp, "--output", outp, "--lookahead", "176"])
