"""Any skeleton without a GPU: ``predict.KeypointMap`` and its refusals, ``predict.map_keypoints_host`` (the rule of uu3d_map_keypoints in
numpy), the two presets (affine, left-right consistent), affinity against the screen normalisation, the command lines, the C ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import util

# the detectors' own left-right orders, written out: mirrored joint k is joint ORDER[k]
COCO17_FLIP = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
BODY25_FLIP = [0, 1, 5, 6, 7, 2, 3, 4, 8, 12, 13, 14, 9, 10, 11, 16, 15, 18, 17, 22, 23, 24, 19, 20, 21]
FLIPS = {"coco17": COCO17_FLIP, "body25": BODY25_FLIP}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_keypoint_map_refusals():
    from uplift_upsample_3dhpe_amd import predict
    ok = predict.KeypointMap(3, [[0], [1, 2], [2, 0, 1]], [[1.0], [0.5, 0.5], [1.0, 1.0, -1.0]])
    assert (ok.inputs, ok.joints) == (3, 3) and ok.sources[2] == (2, 0, 1) and ok.weights[2] == (1.0, 1.0, -1.0)
    bad = [
        ([[0, 1]], [[0.5, 0.25]], "sum to 1"),                           # weights not summing to 1
        ([[0, 1]], [[0.5, 0.5 + 1e-9]], "sum to 1"),
        ([[0, 1]], [[1.0, 0.0]], "finite and non-zero"),                 # a zero weight
        ([[0, 1]], [[np.nan, 1.0]], "finite and non-zero"),              # a non-finite weight
        ([[0, 1]], [[np.inf, -np.inf]], "finite and non-zero"),
        ([list(range(9))], [[1.0 / 9] * 9], "1 to 8 sources"),           # more than 8 sources
        ([[]], [[]], "1 to 8 sources"),
        ([[0, 0]], [[0.5, 0.5]], "distinct"),                            # a repeated source
        ([[0, 9]], [[0.5, 0.5]], r"\[0, 9\)"),                           # a source out of range
        ([[-1]], [[1.0]], r"\[0, 9\)"),
        ([[0, 1]], [[1.0]], "as many weights"),
        ([[0], [1]], [[1.0]], "one entry per model joint"),
    ]
    for sources, weights, match in bad:
        with pytest.raises(ValueError, match=match):
            predict.KeypointMap(9, sources, weights)
    for inputs in (0, -3, True, 2.5):
        with pytest.raises(ValueError, match="inputs"):
            predict.KeypointMap(inputs, [[0]], [[1.0]])
    # the wrong number of joints: a map onto 3 joints for a model of 17, a preset for a model of 16, an unknown name
    with pytest.raises(ValueError, match="3 joints, the model has 17"):
        predict.keypoint_map(ok, 17)
    with pytest.raises(ValueError, match="17 joints, the model has 16"):
        predict.keypoint_map("coco17", 16)
    with pytest.raises(ValueError, match="body25.*coco17"):
        predict.keypoint_map("coco18", 17)
    assert predict.keypoint_map("body25", 17) is predict.KEYPOINT_PRESETS["body25"] and predict.keypoint_map(ok, 3) is ok
    # a track with the wrong joint count names both numbers
    with pytest.raises(ValueError, match="17 keypoints.*takes 25"):
        predict.map_keypoints_host("body25", [np.zeros((4, 17, 2), np.float32)])


def test_host_rule():
    from uplift_upsample_3dhpe_amd import predict
    rng = np.random.default_rng(0)
    M = predict.KeypointMap(6, [[3], [0, 1], [1, 2, 0], [4, 0]], [[1.0], [0.5, 0.5], [1.0, 1.0, -1.0], [1.5, -0.5]])
    x = (rng.normal(size=(12, 6, 2)) * 300).astype(np.float32)
    x[2, 3] = [-0.0, np.float32(1e-42)]                                  # a negative zero and a denormal keep their bits too
    plain, none = predict.map_keypoints_host(M, [x])
    assert none is None and plain[0].dtype == np.float32 and plain[0].shape == (12, 4, 2)
    # a single-source joint keeps its bits; the others are the float64 expression, summed left to right, rounded once
    assert np.array_equal(_bits(plain[0][:, 0]), _bits(x[:, 3]))
    x64 = x.astype(np.float64)
    assert np.array_equal(_bits(plain[0][:, 2]), _bits(((1.0 * x64[:, 1] + 1.0 * x64[:, 2]) + -1.0 * x64[:, 0]).astype(np.float32)))
    assert np.array_equal(_bits(plain[0][:, 3]), _bits((1.5 * x64[:, 4] + -0.5 * x64[:, 0]).astype(np.float32)))
    # a NaN in an unlisted source (5) changes nothing, with or without flags
    y = x.copy()
    y[:, 5] = np.nan
    flags = rng.uniform(size=(12, 6)) >= 0.2
    assert np.array_equal(_bits(predict.map_keypoints_host(M, [y])[0][0]), _bits(plain[0]))
    a, fa = predict.map_keypoints_host(M, [x], [flags])
    b, fb = predict.map_keypoints_host(M, [y], [flags])
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(fa[0], fb[0])
    # a NaN / Inf or a zero flag in a LISTED source: NaN without flags, an unobserved joint written as zeros with them
    z = x.copy()
    z[4, 1, 0] = np.nan
    z[5, 0, 1] = np.inf
    zp, _ = predict.map_keypoints_host(M, [z])
    assert np.isnan(zp[0][4, 1, 0]) and np.isnan(zp[0][4, 2, 0]) and np.isfinite(zp[0][4, 1, 1]) and np.isfinite(zp[0][4, [0, 3]]).all()
    assert _bits(zp[0][4, 1, 0]) == 0x7fc00000                           # THE quiet NaN
    assert np.isposinf(zp[0][5, 1, 1]) and np.isneginf(zp[0][5, 2, 1]) and np.isneginf(zp[0][5, 3, 1])
    ones = np.ones((12, 6), bool)
    ones[7, 4] = False
    zf, ff = predict.map_keypoints_host(M, [z], [ones])
    want = np.ones((12, 4), bool)
    want[4, [1, 2]] = want[5, [1, 2, 3]] = want[7, 3] = False
    assert ff[0].dtype == bool and np.array_equal(ff[0], want)
    assert (zf[0][~want] == 0).all() and np.array_equal(_bits(zf[0][want]), _bits(zp[0][want]))
    # "finite" is the finite test per source joint: the flags above without the zero flag
    zq, fq = predict.map_keypoints_host(M, [z], "finite")
    want[7, 3] = True
    assert np.array_equal(fq[0], want) and (zq[0][~want] == 0).all()
    # (F,) frame flags pass through unchanged and the coordinates are the expression
    frame = rng.uniform(size=12) >= 0.5
    zr, fr = predict.map_keypoints_host(M, [z, x], [frame, flags])
    assert fr[0] is frame and np.array_equal(_bits(zr[0]), _bits(zp[0])) and np.array_equal(_bits(zr[1]), _bits(a[0])) and np.array_equal(fr[1], fa[0])
    with pytest.raises(ValueError, match=r"valid\[0\] must be \(12,\)"):
        predict.map_keypoints_host(M, [x], [np.ones((12, 4), bool)])      # per-joint flags are per SOURCE joint


@pytest.mark.parametrize("name", ["coco17", "body25"])
def test_presets_are_affine_and_mirror_consistently(name):
    from tests.tracks_util import _pixel_tracks
    from uplift_upsample_3dhpe_amd import predict
    cfg = util.load_config("h36m_81")
    M = predict.KEYPOINT_PRESETS[name]
    assert M.joints == 17 == cfg.NUM_KEYPOINTS and M.inputs == len(FLIPS[name]) and sorted(FLIPS[name]) == list(range(M.inputs))
    for w in M.weights:
        total = 0.0
        for x in w:
            total += x
        assert abs(total - 1.0) <= 1e-12
    counts, src, w = M.planes()
    assert np.array_equal(counts, [len(s) for s in M.sources]) and (src[w == 0] == -1).all() and (src[w != 0] >= 0).all()
    # mirroring commutes: negate x and permute by the detector's own left-right order, then map == map, then negate x and permute by
    # AUGM_FLIP_KEYPOINT_ORDER.  Exact: negation is exact and the two sides sum the same terms (a mirrored pair first: a + b == b + a)
    flip_in, flip_out = np.array(FLIPS[name]), np.array(cfg.AUGM_FLIP_KEYPOINT_ORDER)
    for x in _pixel_tracks([40, 33, 21], seed=5, J=M.inputs):
        x = x - np.float32(500.0)                                        # both signs
        mirrored = x[:, flip_in] * np.array([-1.0, 1.0], np.float32)
        a = predict.map_keypoints_host(M, [mirrored])[0][0]
        b = predict.map_keypoints_host(M, [x])[0][0][:, flip_out] * np.array([-1.0, 1.0], np.float32)
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("name", ["coco17", "body25"])
def test_map_commutes_with_the_normalisation_to_4_ulp(name):
    """normalize(map(x)) against map(normalize(x)).  Each side rounds to float32 twice on the way to a coordinate (the map's one rounding
    and the normalisation's stored result, in either order), each by at most half an ulp of the value it rounds; the values rounded are
    coordinates of the normalised image, so the unit is the ulp of the larger of the two coordinates compared, taken no smaller than the
    ulp of 1: the normalisation subtracts 1 (h / w) from a quotient in [0, 2], so a coordinate near the image centre still carries the
    rounding of a number near 1.  4 ulp = two roundings on each side; printed before it is asserted."""
    from tests.tracks_util import RES, _pixel_tracks
    from uplift_upsample_3dhpe_amd import h36m, predict
    M = predict.KEYPOINT_PRESETS[name]
    worst = 0.0
    for i, x in enumerate(_pixel_tracks([50, 50, 50], seed=9, J=M.inputs)):
        w, h = RES[i % len(RES)]
        norm = lambda t: h36m.normalize_screen_coordinates(t, w=w, h=h).astype(np.float32)
        a = norm(predict.map_keypoints_host(M, [x])[0][0])
        b = predict.map_keypoints_host(M, [norm(x)])[0][0]
        ulp = np.spacing(np.maximum(np.maximum(np.abs(a), np.abs(b)), np.float32(1.0)))
        worst = max(worst, float((np.abs(a.astype(np.float64) - b.astype(np.float64)) / ulp).max()))
    print(f"{name}: normalize(map(x)) and map(normalize(x)) differ by at most {worst:.3f} ulp")
    assert worst <= 4.0


def test_command_lines(tmp_path, monkeypatch):
    from uplift_upsample_3dhpe_amd import predict, stream
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)
    scored = np.concatenate([rng.normal(size=(9, 17, 2)), rng.uniform(size=(9, 17, 1))], axis=2).astype(np.float32)
    inp, outp = str(tmp_path / "tracks.npz"), str(tmp_path / "out.npz")
    np.savez(inp, walk=scored, sit=rng.normal(size=(5, 17, 2)).astype(np.float32))
    seen = {}

    def fake_replay(model, config, trs, **kw):
        seen["kw"], seen["tracks"] = kw, trs
        return [np.zeros((len(t), 17, 3), np.float32) for t in trs], [np.ones(len(t), bool) for t in trs]

    def fake_predict(model, config, trs, **kw):
        seen["kw"], seen["tracks"] = kw, trs
        return [torch.zeros((len(t), 17, 3)) for t in trs]
    monkeypatch.setattr(stream, "_load_model", lambda config, weights: None)
    monkeypatch.setattr(stream, "replay_tracks", fake_replay)
    monkeypatch.setattr(predict, "_load_model", lambda config, weights: object())
    monkeypatch.setattr(predict, "predict_tracks", fake_predict)
    cfg = os.path.join(util.ROOT, "config", "h36m_81.json")
    base = ["--config", cfg, "--weights", "w.h5", "--input", inp, "--output", outp]
    for main, more in ((predict.main, []), (predict.main, ["--repair_joints", "5"]), (stream.main, ["--repair_joints", "5"])):
        seen.clear()
        assert main(base + ["--keypoints", "coco17", "--min_score", "0.5"] + more) == 0
        assert seen["kw"]["keypoints"] == "coco17" and [t.shape for t in seen["tracks"]] == [(9, 17, 2), (5, 17, 2)]
        assert seen["kw"]["valid"][0].shape == (9, 17) and np.array_equal(seen["kw"]["valid"][0], scored[:, :, 2] >= np.float32(0.5))
        assert seen["kw"]["valid"][1].shape == (5, 17) and seen["kw"]["valid"][1].all()
        assert seen["kw"].get("repair_joints") == (5 if more else None)
    # the detector's joint count decides which arrays pass: 25 joints with body25, not 17
    for main in (predict.main, stream.main):
        with pytest.raises(SystemExit, match=r"expected \(T, 25, 2\)"):
            main(base + ["--keypoints", "body25"])
    np.savez(inp, walk=rng.normal(size=(6, 25, 2)).astype(np.float32))
    for main in (predict.main, stream.main):
        seen.clear()
        assert main(base + ["--keypoints", "body25"]) == 0
        assert seen["kw"]["keypoints"] == "body25" and seen["tracks"][0].shape == (6, 25, 2) and "valid" not in seen["kw"]
        with pytest.raises(SystemExit):
            main(base)                                                   # without --keypoints the model's own 17 joints are expected
        with pytest.raises(SystemExit):
            main(base + ["--keypoints", "coco18"])                       # an unknown preset
    # without --keypoints no such keyword is handed on
    np.savez(inp, walk=rng.normal(size=(6, 17, 2)).astype(np.float32))
    for main in (predict.main, stream.main):
        seen.clear()
        assert main(base) == 0 and "keypoints" not in seen["kw"]


def test_live_options_gate_and_plan():
    """``keypoints`` goes through the ``**options`` gate of the live entries next to ``repair_joints``; a wrong joint count is refused
    before any device is touched."""
    import types
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg = util.load_config("h36m_81")
    stub = types.SimpleNamespace(arch=types.SimpleNamespace(compiled_dims=True), device="cpu", has_strided_input=True)
    with pytest.raises(TypeError, match="unexpected keyword argument 'keypoint'"):
        stream.StreamSession(stub, cfg, slots=2, mask_stride=4, keypoint="coco17")
    with pytest.raises(TypeError, match="unexpected keyword argument 'keypoint'"):
        stream.replay_tracks(stub, cfg, [np.zeros((4, 17, 2), np.float32)], keypoint="coco17")
    with pytest.raises(ValueError, match="coco18"):
        stream.StreamSession(stub, cfg, slots=2, mask_stride=4, keypoints="coco18")
    with pytest.raises(ValueError, match="17 keypoints.*takes 25"):
        stream.replay_tracks(stub, cfg, [np.zeros((4, 17, 2), np.float32)], keypoints="body25")
    with pytest.raises(ValueError, match="repair_joints.*re-make model frames"):  # the existing refusals stay
        stream.StreamSession(stub, cfg, slots=2, mask_stride=4, lookahead=40, repair_joints=3, fps=25, keypoints="coco17")
    plans = []
    for kw in ({}, {"keypoints": None}, {"keypoints": "body25"}):
        s = object.__new__(stream.StreamSession)
        s._init_plan(stub, cfg, 3, (1920, 1080), 4, True, 5, True, True, None, 50, None, **kw)
        plans.append({k: v for k, v in vars(s).items() if k not in ("model", "_key")})
    assert plans[0] == plans[1] and plans[0]["keypoints"] is None
    assert plans[2].pop("keypoints") is predict.KEYPOINT_PRESETS["body25"] and plans[0].pop("keypoints") is None and plans[2] == plans[0]
    small = cfg.copy()
    small.NUM_KEYPOINTS = 16
    with pytest.raises(ValueError, match="17 joints, the model has 16"):
        stream.StreamSession(stub, small, slots=2, mask_stride=4, keypoints="coco17")


def test_c_abi_declared_exported_and_refusing():
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi, predict
    lib = _capi.load_library()
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    assert "ANY SKELETON" in header
    for s in ("uu3d_keypoint_map_bytes", "uu3d_keypoint_map_pack", "uu3d_map_keypoints"):
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.uu3d_keypoint_map_bytes(17, 17) == 17 * 100 + 4 and lib.uu3d_keypoint_map_bytes(0, 17) == 0 and lib.uu3d_keypoint_map_bytes(17, 0) == 0
    # the packed table: w (J, 8) f64, src (J, 8) i32 with -1 behind a joint's sources, n (J) i32
    M = predict.KEYPOINT_PRESETS["coco17"]
    counts, src, w = M.planes()
    table = M.packed()
    assert table.dtype == np.uint8 and len(table) == 1704
    assert np.array_equal(table[:17 * 64].view(np.float64).reshape(17, 8), w)
    assert np.array_equal(table[17 * 64:17 * 96].view(np.int32).reshape(17, 8), src)
    assert np.array_equal(table[17 * 96:17 * 100].view(np.int32), counts)

    def pack(inputs, counts, src, w):
        out = np.zeros(len(counts) * 13, np.float64)
        return lib.uu3d_keypoint_map_pack(inputs, len(counts), counts.ctypes.data, src.ctypes.data, w.ctypes.data, out.ctypes.data, out.nbytes)
    assert pack(17, counts, src, w) == _capi.UU3D_OK
    assert pack(12, counts, src, w) == _capi.UU3D_ERR_INVALID_ARGUMENT   # the index range is checked when the table is packed
    for j, k, value in ((8, 1, 5), (8, 0, -1)):                          # a repeated source, a negative one
        bad = src.copy()
        bad[j, k] = value
        assert pack(17, counts, bad, w) == _capi.UU3D_ERR_INVALID_ARGUMENT
    for value in (0.0, np.nan, 0.25 + 1e-9):
        bad = w.copy()
        bad[8, 2] = value
        assert pack(17, counts, src, bad) == _capi.UU3D_ERR_INVALID_ARGUMENT
    for n in (0, 9):
        bad = counts.copy()
        bad[3] = n
        assert pack(17, bad, src, w) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_keypoint_map_pack(17, 17, counts.ctypes.data, src.ctypes.data, w.ctypes.data, np.zeros(8).ctypes.data, 64) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_map_keypoints(None, None, 17, None, None, 0, None, None, None) == _capi.UU3D_ERR_INVALID_ARGUMENT   # no handle


def test_kernel_source_has_no_atomics_and_the_float64_discipline():
    csrc = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "uu3d_keypoints.h")).read())
    assert "atomic" not in code.lower() and "fp contract(off)" in code and "finite_pair(" in code
    assert re.search(r"reinterpret_cast<float2\*>\(out \+ p \* 2\) = ", code)   # the 8-byte store of the coordinate pair
