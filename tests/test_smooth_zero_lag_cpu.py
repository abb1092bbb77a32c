"""CPU: the zero-lag, two-pass One-Euro filter (include/uu3d.h, STEADY OUTPUT, ZERO LAG; predict.OneEuro(zero_lag=True), one_euro_host) --
the flag and what it does to tuple / repr / == / hash, the live refusals that need no device, the definition (per track
reverse(walk(reverse(walk(x)))) with the causal walk, bit for bit), the lag it takes out of a ramp, the C ABI's argument checks and the
BVH command's flags."""
import types

import numpy as np
import pytest

from tests import util
from tests.zero_lag_util import bits, composition, hard_input

CAMERA = (1145.0, 1143.5, 512.25, 515.75)


# ---- the flag ------------------------------------------------------------------------------------------------------------------------------
def test_zero_lag_flag():
    from uplift_upsample_3dhpe_amd import predict
    Z, F = predict.OneEuro(zero_lag=True), predict.OneEuro()
    assert tuple(Z) == (1.0, 0.5, 1.0) and Z.zero_lag is True and F.zero_lag is False
    assert F != Z and Z != F and Z == predict.OneEuro(1, 0.5, 1, zero_lag=True) and F == predict.OneEuro(zero_lag=False)
    assert hash(F) != hash(Z) and hash(Z) == hash(predict.OneEuro(zero_lag=True)) and len({F, Z, predict.OneEuro()}) == 2
    assert repr(F) == "OneEuro(min_cutoff=1.0, beta=0.5, d_cutoff=1.0)"
    assert repr(Z) == "OneEuro(min_cutoff=1.0, beta=0.5, d_cutoff=1.0, zero_lag=True)"
    assert repr(predict.OneEuro(0.25, 0, 3, zero_lag=True)) == "OneEuro(min_cutoff=0.25, beta=0.0, d_cutoff=3.0, zero_lag=True)"
    with pytest.raises(TypeError):
        predict.OneEuro(1.0, 0.5, 1.0, True)                          # keyword only
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="OneEuro"):
            predict.OneEuro(zero_lag=bad)
    with pytest.raises(ValueError, match="OneEuro needs"):
        predict.OneEuro(0, 0.5, 1, zero_lag=True)
    # check_smooth hands such filters through in every form
    R = predict.OneEuro(0.5, 0.0, 1.0)
    assert predict.check_smooth(Z, True) == (Z, Z) and predict.check_smooth(Z, False) == (Z, None)
    assert predict.check_smooth((Z, R), True) == (Z, R) and predict.check_smooth([R, Z], True) == (R, Z)
    assert predict.check_smooth((None, Z), True) == (None, Z) and predict.check_smooth((Z, None), False) == (Z, None)
    assert all(f.zero_lag for f in predict.check_smooth(Z, True)) and predict.check_smooth((Z, R), True)[1].zero_lag is False
    assert predict.check_smooth(True, True) == (F, F)                 # True stays the causal defaults
    with pytest.raises(ValueError, match="root filter needs camera"):
        predict.check_smooth((None, Z), False)


# ---- the live refusals -----------------------------------------------------------------------------------------------------------------------
def _stub_model():
    return types.SimpleNamespace(arch=types.SimpleNamespace(compiled_dims=True), device="cpu", has_strided_input=True)


def test_live_refusals_need_no_device():
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg = util.load_config("h36m_81")
    Z, F = predict.OneEuro(2.0, 0.1, 1.5, zero_lag=True), predict.OneEuro(2.0, 0.1, 1.5)
    words = "live filtering is causal.*zero_lag=True.*predict_tracks"
    tracks = [np.zeros((6, 17, 2), np.float32)] * 2
    for smooth, kw in ((Z, {}), ((Z, None), {}), (Z, {"camera": CAMERA}), ((None, Z), {"camera": CAMERA}), ((F, Z), {"camera": CAMERA}),
                       ((Z, F), {"camera": CAMERA})):
        with pytest.raises(ValueError, match=words):
            stream.StreamSession(_stub_model(), cfg, slots=2, mask_stride=4, smooth=smooth, **kw)
        with pytest.raises(ValueError, match=words):
            stream.replay_tracks(_stub_model(), cfg, tracks, mask_stride=4, smooth=smooth, **kw)
    with pytest.raises(ValueError, match=words):
        stream.replay_detections(_stub_model(), cfg, np.zeros((6, 2, 17, 2), np.float32), mask_stride=4, smooth=Z)
    s = object.__new__(stream.StreamSession)                          # the causal twin still plans
    s._init_plan(_stub_model(), cfg, 3, (1920, 1080), 4, True, 5, True, False, None, 50, None, smooth=F)
    assert s.pose_filter == F
    for live in (stream.LiveOneEuroHost, stream.LiveOneEuro):         # (LiveOneEuro refuses before it loads the library or touches a device)
        with pytest.raises(ValueError, match=words):
            live(2, 3, 50, Z)
    stream.LiveOneEuroHost(2, 3, 50, F)
    # offline the shared check lets it through, for either member
    from uplift_upsample_3dhpe_amd.options import stage_options
    for per, ok in (("track", True), ("slot", False)):
        args = (cfg, 2, per, True, None, CAMERA, 6, (F, Z), None, None, None, None)
        if ok:
            assert stage_options(*args).root_filter == Z
        else:
            with pytest.raises(ValueError, match=words):
                stage_options(*args)


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
LENS = [1, 2, 3, 40, 5]
RATES = [50, 29.97, (30000, 1001), 50, 29.97]


@pytest.mark.parametrize("params", [(1.0, 0.5, 1.0), (0.7, 2.5, 1.3), (1.0, 0.0, 1.0)])
def test_two_pass_is_the_composition_bit_for_bit(params):
    from uplift_upsample_3dhpe_amd import predict
    Z = predict.OneEuro(*params, zero_lag=True)
    x, state = hard_input(LENS, 4, seed=11)
    for st in (None, state):
        got = predict.one_euro_host(x, LENS, RATES, Z, state=st)
        want = composition(x, LENS, RATES, Z, state=st)
        assert got.dtype == np.float32 and got.shape == x.shape
        assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]
        bad = ~np.isfinite(x)
        assert bad.sum() == 4 and np.array_equal(bits(got[bad]), bits(x[bad]))          # passed through by both passes
        causal = predict.one_euro_host(x, LENS, RATES, predict.OneEuro(*params), state=st)
        assert not np.array_equal(bits(got), bits(causal))
        if st is not None:
            assert np.array_equal(bits(got[state == 0]), bits(x[state == 0]))
            assert np.array_equal(bits(got[-LENS[-1]:]), bits(x[-LENS[-1]:]))            # the track with no usable row
        # a track's last usable row comes out as pass 1 left it; a one-row track as given
        assert np.array_equal(bits(got[0]), bits(x[0])) and np.array_equal(bits(got[2]), bits(causal[2]))
        last = sum(LENS[:4]) - 1 - (0 if st is None else 1)           # (with state the long track's last row is passed through)
        usable = np.isfinite(x[last])
        assert usable.sum() >= 3 and np.array_equal(bits(got[last][usable]), bits(causal[last][usable]))
    # any trailing shape, one track, one rate
    z = predict.one_euro_host(x.reshape(-1, 2, 2), None, 50, Z)
    assert z.shape == (len(x), 2, 2) and np.array_equal(bits(z.reshape(len(x), 4)), bits(composition(x, [len(x)], [50], Z)))


# ---- the lag is gone -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [1.0, 0.2])
def test_ramp_has_no_lag(v):
    from uplift_upsample_3dhpe_amd import predict
    x = (v * np.arange(400, dtype=np.float64) / 50).astype(np.float32).reshape(400, 1)
    mid = slice(100, 300)
    two = predict.one_euro_host(x, None, 50, predict.OneEuro(zero_lag=True)).astype(np.float64)
    one = predict.one_euro_host(x, None, 50, predict.OneEuro()).astype(np.float64)
    dev_two, dev_one = np.abs(two - x)[mid].max(), np.abs(one - x)[mid].max()
    print(f"ramp {v} units/s: max deviation two-pass {dev_two:.3g}, causal {dev_one:.3g}")
    assert dev_two <= 2e-6
    assert dev_one >= 1e-2


def test_noisy_ramp_orders_two_pass_raw_causal():
    from uplift_upsample_3dhpe_amd import predict
    clean = (np.arange(400, dtype=np.float64) / 50).reshape(400, 1)
    x = (clean + np.random.default_rng(5).normal(0.0, 0.01, size=clean.shape)).astype(np.float32)
    mid = slice(100, 300)
    rms = lambda y: float(np.sqrt(np.mean((y.astype(np.float64) - clean)[mid] ** 2)))
    two, raw, one = (rms(predict.one_euro_host(x, None, 50, predict.OneEuro(zero_lag=True))), rms(x),
                     rms(predict.one_euro_host(x, None, 50, predict.OneEuro())))
    print(f"rms error against the clean ramp: two-pass {two:.3g}, raw {raw:.3g}, causal {one:.3g}")
    assert two < raw < one


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_declared_and_refusing_like_the_causal_entry():
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(util.ROOT + "/include/uu3d.h").read()
    assert "uu3d_one_euro_tracks_two_pass(" in header and "ZERO LAG" in header
    assert "uu3d_one_euro_tracks_two_pass" in _capi.EXPORTED_SYMBOLS and hasattr(lib, "uu3d_one_euro_tracks_two_pass")
    assert lib.uu3d_one_euro_tracks_two_pass.argtypes == lib.uu3d_one_euro_tracks.argtypes
    block, other = C.c_void_p(256), C.c_void_p(512)                   # (aligned addresses that are never dereferenced: the calls refuse first)
    odd = C.c_void_p(258)
    BAD, UNS, OK = _capi.UU3D_ERR_INVALID_ARGUMENT, _capi.UU3D_ERR_UNSUPPORTED, _capi.UU3D_OK
    calls = {
        "channels beyond the limit": (dict(C_=(1 << 16) + 1), UNS),
        "min_cutoff 0": (dict(mc=0.0), BAD), "min_cutoff nan": (dict(mc=float("nan")), BAD), "beta < 0": (dict(beta=-0.5), BAD),
        "beta inf": (dict(beta=float("inf")), BAD), "d_cutoff 0": (dict(dc=0.0), BAD), "no channels": (dict(C_=0), BAD),
        "rows < 0": (dict(rows=-1), BAD), "tracks < 0": (dict(tracks=-1), BAD), "too many tracks": (dict(tracks=(1 << 20) + 1), BAD),
        "out is in": (dict(out=block), BAD), "in NULL": (dict(inp=None), BAD), "out NULL": (dict(out=None), BAD),
        "track_start NULL": (dict(start=None), BAD), "track_len NULL": (dict(length=None), BAD), "rates NULL": (dict(rates=None), BAD),
        "in misaligned": (dict(inp=odd), BAD), "rates misaligned": (dict(rates=C.c_void_p(260)), BAD),
        "no rows": (dict(rows=0), OK), "no tracks": (dict(tracks=0), OK), "no rows, NULL buffers": (dict(rows=0, inp=None, out=None), OK),
    }
    for name, (kw, want) in calls.items():
        a = dict(inp=block, out=other, rows=4, C_=51, start=block, length=block, rates=block, tracks=1, mc=1.0, beta=0.5, dc=1.0)
        a.update(kw)
        args = (a["inp"], a["out"], a["rows"], a["C_"], a["start"], a["length"], a["rates"], a["tracks"], None, a["mc"], a["beta"], a["dc"], None)
        assert lib.uu3d_one_euro_tracks_two_pass(*args) == want, name
        assert lib.uu3d_one_euro_tracks(*args) == want, name          # the same code as the causal entry for the same bad call


# ---- the BVH command ---------------------------------------------------------------------------------------------------------------------
def test_bvh_command_flags(tmp_path, monkeypatch):
    import torch
    from uplift_upsample_3dhpe_amd import bones, bvh, predict, rotations, smooth
    base = ["--input", "in.npz", "--output", "out"]
    a = bvh.parse_args(base)
    assert a.smooth is None and a.smooth_root is None and a.pose_filter is None and a.root_filter is None
    a = bvh.parse_args(base + ["--smooth", "2", "0.1", "1.5"])
    assert a.pose_filter == predict.OneEuro(2.0, 0.1, 1.5, zero_lag=True) and a.root_filter is None
    a = bvh.parse_args(base + ["--smooth", "2", "0.1", "1.5", "--smooth_root", "0.5", "0", "1"])
    assert a.pose_filter.zero_lag and a.root_filter == predict.OneEuro(0.5, 0.0, 1.0, zero_lag=True)
    for bad in (["--smooth", "1", "2"], ["--smooth_root", "a", "b", "c"]):
        with pytest.raises(SystemExit):
            bvh.parse_args(base + bad)
    for bad in (["--smooth", "0", "0.1", "1.5"], ["--smooth_root", "1", "-1", "1"], ["--smooth", "nan", "0", "1"]):
        with pytest.raises(SystemExit, match="--smooth / --smooth_root: OneEuro needs"):
            bvh.parse_args(base + bad)
    # main: the device calls are stand-ins that keep tensors on the host and say what they were given
    rng = np.random.default_rng(3)
    poses, roots = rng.normal(size=(9, 17, 3)).astype(np.float32), rng.normal(size=(9, 3)).astype(np.float32)
    state = np.array([0, 1, 1, 2, 2, 1, 1, 0, 1], np.uint8)
    inp, plain = str(tmp_path / "in.npz"), str(tmp_path / "plain.npz")
    np.savez(inp, walk=poses, walk__root=roots, walk__root_state=state)
    np.savez(plain, walk=poses, walk__root=roots)
    seen = []
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)

    def fake_one_euro(x, lens, rate, filt, state=None):
        seen.append(("one_euro", tuple(x.shape), lens, rate, filt, None if state is None else state.numpy().copy()))
        return x + 1.0

    def fake_lengths(p, lens, skeleton):
        seen.append(("bone_lengths", p.numpy().copy()))
        return torch.ones((1, 17), dtype=torch.float64)

    def fake_fix(p, lens, lengths, skeleton):
        return p

    def fake_rotations(p, R):
        q = torch.zeros((p.shape[0], 17, 4), dtype=torch.float32)
        q[..., 0] = 1.0
        return (q,)
    monkeypatch.setattr(smooth, "one_euro", fake_one_euro)
    monkeypatch.setattr(bones, "bone_lengths", fake_lengths)
    monkeypatch.setattr(bones, "fix_bones", fake_fix)
    monkeypatch.setattr(rotations, "joint_rotations", fake_rotations)
    moved = lambda path: bvh.read_bvh(path)["translations"] / 100.0
    # without the flags: today's path -- no filter call, the poses and roots as the file has them
    out = str(tmp_path / "a")
    assert bvh.main(["--input", inp, "--output", out]) == 0
    assert [s[0] for s in seen] == ["bone_lengths"] and np.array_equal(seen[0][1], poses)
    assert np.abs(moved(out + "/walk.bvh") - roots).max() <= 1e-6
    # --smooth: the poses go through the zero-lag filter at --fps BEFORE the bone lengths; the roots stay
    del seen[:]
    out = str(tmp_path / "b")
    assert bvh.main(["--input", inp, "--output", out, "--fps", "25", "--smooth", "2", "0.1", "1.5"]) == 0
    assert [s[0] for s in seen] == ["one_euro", "bone_lengths"]
    assert seen[0][1:5] == ((9, 17, 3), None, 25.0, predict.OneEuro(2.0, 0.1, 1.5, zero_lag=True)) and seen[0][5] is None
    assert np.array_equal(seen[1][1], poses + 1.0) and np.abs(moved(out + "/walk.bvh") - roots).max() <= 1e-6
    # --smooth_root: NAME__root with NAME__root_state as its state; a file without the state: none
    for source, want_state in ((inp, state != 0), (plain, None)):
        del seen[:]
        out = str(tmp_path / ("c" if want_state is not None else "d"))
        assert bvh.main(["--input", source, "--output", out, "--smooth_root", "0.5", "0", "1"]) == 0
        assert [s[0] for s in seen] == ["bone_lengths", "one_euro"] and np.array_equal(seen[0][1], poses)
        assert seen[1][1:5] == ((9, 3), None, 50.0, predict.OneEuro(0.5, 0.0, 1.0, zero_lag=True))
        assert (seen[1][5] is None) if want_state is None else np.array_equal(seen[1][5] != 0, want_state)
        assert np.abs(moved(out + "/walk.bvh") - (roots + 1.0)).max() <= 1e-6
