"""CPU: the pieces of predict.predict_tracks that need no GPU -- the two C-ABI symbols, the atomic-free source and gfx950 code of
csrc/uu3d_tracks.h (hipcc cross-compiles without a GPU), the command line and its .npz round trip with a stub model."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import util

CSRC = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
SYMBOLS = ("uu3d_normalize_tracks", "uu3d_assemble_tracks")


def test_symbols_declared_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    # arguments are refused before anything is launched (no device needed)
    assert lib.uu3d_normalize_tracks(None, 1, None, 1, 17, None, 1, None, None, None, 0, None) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_assemble_tracks(None, None, 1, None, None, None, None, 1, 17, 6, None, None) == _capi.UU3D_ERR_INVALID_ARGUMENT


def test_package_exports_predict_tracks():
    import uplift_upsample_3dhpe_amd as pkg
    from uplift_upsample_3dhpe_amd import predict
    assert callable(pkg.predict_tracks) and callable(predict.predict_tracks)
    assert "resampled" in predict.predict_tracks.__doc__ and "never reach the network" in predict.predict_tracks.__doc__


def test_source_has_no_atomics():
    text = open(os.path.join(CSRC, "uu3d_tracks.h")).read()
    code = re.sub(r"//[^\n]*", "", text)                              # (the comments say "no atomics")
    assert "atomic" not in code.lower()
    assert '#include "uu3d_tracks.h"' in open(os.path.join(CSRC, "uu3d_api.hip")).read()


@pytest.fixture(scope="module")
def asm():
    import importlib.util
    spec = importlib.util.spec_from_file_location("uu3d_build_tracks", os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "build.py"))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src_text = '#include "uu3d_tracks.h"\n'
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "k.hip"), os.path.join(d, "k.s")
        open(src, "w").write(src_text)
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", *b.DEVICE_FLAGS, "-I", CSRC, "-S", "--cuda-device-only", "-o", out, src],
                       check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def _kernels(asm):
    return {m.group(1): m.group(0) for m in re.finditer(r"^(_ZN4uu3d\w+):.*?s_endpgm", asm, re.S | re.M)}


def test_code_objects_have_no_atomics_and_store_16_bytes(asm):
    ks = _kernels(asm)
    norm = next(v for k, v in ks.items() if "normalize_tracks_kernel" in k)
    asse = next(v for k, v in ks.items() if "assemble_tracks_kernel" in k)
    for body in (norm, asse):
        assert "global_atomic" not in body and "flat_atomic" not in body and "buffer_atomic" not in body
        assert not re.search(r"ds_\w+_rtn", body) and "ds_add" not in body
        assert "scratch_" not in body
        assert "global_store_dwordx4" in body                         # the 16-byte store of the flattened output
        assert not re.search(r"\bs_(?:buffer_|scratch_)?(?:store|atomic)", body)          # vector stores only
        assert "v_pk_mul_f32" not in body and "v_pk_fma_f32" not in body and "v_pk_add_f32" not in body
    # the interpolation is the host's two float64 products and one sum, each rounded: no fused multiply-add on doubles
    assert "v_fma_f64" not in asse and "v_mul_f64" in asse and "v_add_f64" in asse
    # the normalisation subtracts in float64 (numpy's float32 array minus a float64 list) after a correctly rounded float32 division
    assert "v_add_f64" in norm and "v_div_fixup_f32" in norm


def test_keyframe_count_and_padding_rule():
    from uplift_upsample_3dhpe_amd import predict
    assert [predict.keyframe_count(n, 5) for n in (1, 5, 6, 37)] == [1, 1, 2, 8]
    c351, c81 = util.load_config("h36m_351"), util.load_config("h36m_81")
    assert all(predict.padding_source_is_keyframe(n, c351, 5) for n in range(1, 40))          # mask stride == sequence stride
    # h36m_81: sequence stride 2, mask stride 4 -- the last even frame is a multiple of 4 for lengths 4k + 1 and 4k + 2 only
    assert [predict.padding_source_is_keyframe(n, c81, 4) for n in (201, 202, 203, 204)] == [True, True, False, False]


class _StubModel(object):
    device = "cpu"


def test_cli_arguments_and_npz_round_trip(tmp_path, monkeypatch, capsys):
    from uplift_upsample_3dhpe_amd import predict
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)
    tracks = {"walk": rng.normal(size=(23, 17, 2)).astype(np.float32), "sit": rng.normal(size=(7, 17, 2)).astype(np.float32)}
    inp, outp = str(tmp_path / "tracks.npz"), str(tmp_path / "out.npz")
    np.savez(inp, **tracks)
    seen = {}

    def fake_load(config, weights):
        seen["weights"] = weights
        return _StubModel()

    def fake_predict(model, config, trs, **kw):
        seen["kw"] = kw
        seen["tracks"] = trs
        lens = kw["lengths"] if kw.get("keyframes_only") else [len(t) for t in trs]
        return [torch.full((int(n), 17, 3), float(i), dtype=torch.float32) for i, n in enumerate(lens)]
    monkeypatch.setattr(predict, "_load_model", fake_load)
    monkeypatch.setattr(predict, "predict_tracks", fake_predict)
    cfg = os.path.join(util.ROOT, "config", "h36m_351.json")
    assert predict.main(["--config", cfg, "--weights", "w.h5", "--input", inp, "--output", outp]) == 0
    assert seen["weights"] == "w.h5" and isinstance(seen["kw"].pop("lengths", None), type(None))
    assert seen["kw"] == {"resolutions": None, "mask_stride": 5, "keyframes_only": False}
    assert [t.shape for t in seen["tracks"]] == [(23, 17, 2), (7, 17, 2)] and all(t.dtype == np.float32 for t in seen["tracks"])
    with np.load(outp) as z:
        assert list(z.files) == ["walk", "sit"]
        assert z["walk"].shape == (23, 17, 3) and z["walk"].dtype == np.float32 and (z["walk"] == 0).all()
        assert z["sit"].shape == (7, 17, 3) and (z["sit"] == 1).all()
    assert "2 tracks, 30 frames" in capsys.readouterr().out
    # every option: the resolution reaches predict_tracks as (w, h), keyframe tracks get their dense lengths (K - 1) * s_in + 1
    assert predict.main(["--config", cfg, "--weights", "w.h5", "--input", inp, "--output", outp, "--resolution", "1920", "1080",
                         "--mask_stride", "10", "--keyframes_only"]) == 0
    assert seen["kw"] == {"resolutions": (1920.0, 1080.0), "mask_stride": 10, "keyframes_only": True, "lengths": [221, 61]}
    with np.load(outp) as z:
        assert z["walk"].shape == (221, 17, 3) and z["sit"].shape == (61, 17, 3)
    # refused input: a missing argument, an array of the wrong shape
    with pytest.raises(SystemExit):
        predict.main(["--config", cfg, "--input", inp, "--output", outp])
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, a=np.zeros((5, 16, 2), np.float32))
    with pytest.raises(SystemExit):
        predict.main(["--config", cfg, "--weights", "w.h5", "--input", bad, "--output", outp])


def test_track_checks_need_no_device():
    """The argument checks of pose_table run before anything touches a device."""
    from uplift_upsample_3dhpe_amd import predict
    torch = pytest.importorskip("torch")
    t = torch.zeros((8, 17, 2))
    with pytest.raises(ValueError, match="lengths"):
        predict.pose_table([t], "cpu", key_stride=5)
    with pytest.raises(ValueError, match="keyframes"):
        predict.pose_table([t], "cpu", key_stride=5, lengths=[50])          # 50 frames at stride 5 are 10 keyframes, not 8
    with pytest.raises(ValueError, match="resolutions"):
        predict.pose_table([t, t], "cpu", resolutions=[(1000, 1000)] * 3)
    with pytest.raises(ValueError, match=r"\(T, J, 2\)"):
        predict.pose_table([torch.zeros((8, 17, 3))], "cpu")


@pytest.mark.parametrize("cfgname,ms", [("h36m_351", 5), ("h36m_81", 4)])
def test_windows_read_keyframes_only_where_the_padding_rule_says_so(cfgname, ms):
    """What keyframes_only rests on, by the host restatement of the gather rules (eval.window_frames): the windows that are run read nothing
    but multiples of the mask stride exactly when predict.padding_source_is_keyframe holds; otherwise the one other frame they read is the
    copy-padding source behind the end of the track."""
    from uplift_upsample_3dhpe_amd import eval as ev
    from uplift_upsample_3dhpe_amd import predict
    cfg = util.load_config(cfgname)
    N, s = cfg.SEQUENCE_LENGTH, cfg.SEQUENCE_STRIDE
    for L in (1, 2, 37, 200, 201, 202, 203, 418, 597, 600):
        c = np.arange(0, L, s)
        desc = np.stack([np.zeros_like(c), c, np.full_like(c, s), np.full_like(c, ms), c, np.zeros_like(c)], -1)
        read, _, _ = ev.window_frames(desc, N, [0], [L], True)
        other = read[read % ms != 0]
        if predict.padding_source_is_keyframe(L, cfg, ms):
            assert len(other) == 0, (L, other)
        else:
            assert list(other) == [(L - 1) // s * s], (L, other)
