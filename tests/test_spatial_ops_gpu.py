"""The SPATIAL STACK, kernel form by kernel form through uu3d_op_spatial_stack / uu3d_op_compact_frames / uu3d_op_spatial_choice
(include/uu3d_ops.h), against the float64 reference of tests/spatial_util.py (held to the oracle's float64 path by tests/test_spatial_ref_cpu.py).
The operator runs on a committed handle and launches through the helpers the forward's spatial_stage and generic_frame_features launch
through: a case here runs the kernel, grid, LDS size, SpatialParams and weight fragments (uu3d_commit.inc's pack) the forward runs.

Forms: UU3D_SPATIAL_F32 (spatial_stack_mfma_kernel<17, 3>), _H3_TILES (spatial_stack_h3_kernel<17, 3, MT>, inference form), _P16
(spatial_stack_p16_kernel<17, 7, 1>), each x f32 / planes output where it exists, each x no mask / mask; AUTO on generic handles
(spatial_generic_kernel); compact_frames_kernel on its own.

Checks (numbers as in the issue that asked for this file):
  1 against float64.  f16x3 kernels: 2e-5 (tests/test_panel_op_gpu.py's bound for one f16x3 layer at unit scale; max|ref| < 16 asserted)
    + 2 x the max-abs deviation of the float32 oracle from float64 on that case's frames (CPU); the x30 and 1e3 frames: 2e-5 max|ref| + the
    same term on those frames.  Exact-f32 kernel and generic kernel: max(4 x that deviation, 2e-6 max|ref|) (tests/test_bwd_ops_gpu.py's
    measure).  Every allowance asserted <= 1e-4.  No bound comes from a kernel.
  2 plane output = the split (device_split: h3_split in the kernels' conversion form) of the same handle's f32 output, hi and lo of every
    element, bitwise.
  3 slot independence: a probe frame at every index 0 .. 13 of a 14-frame launch and as a launch of 1: the same 544 outputs bitwise; the same
    under a mask that keeps the probe and one other frame.
  4 masks at every frame count (alternating, every 5th kept, only the first, only the last, all masked): kept rows = the unmasked launch's
    rows bitwise, masked rows and the guard frame still NaN, the all-masked launch writes nothing.
  5 every launch is made twice and compared bitwise (_twice).
  6 re-commit: other weights, then back: S follows the weights under the bound of 1, the third launch = the first bitwise.
  7 uu3d_op_spatial_choice = the restatement below on both sides of each boundary of spatial_h3_pays, both precisions, the exact-f32 bit, each
    UU3D_SPATIAL value and UU3D_NO_PLANES; AUTO = the bits of the forced kernel it names.
    (spatial_h3_pays: the f16x3 kernel loses to the exact-f32 one only while ceil(F / 3) is in 1537 .. 1792, F = 4609 .. 5376: two rounds of 68 us
    against one of 133 us.  F = 3 x 1792 + 1 = 5377 is the first count BACK on p16; the large launches here are F = 4609, where AUTO is the f32
    kernel, and F = 5377, where it is p16 over 769 workgroups.)
Every output buffer is NaN-filled and followed by a guard frame; every frame list carries a guard int.

Measured on an MI355X (largest max-abs error of a form over all its cases, next to the smallest bound any of those cases was held to; the
plane and masked forms are tied to the f32 form bit for bit, so these are their errors too):
  spatial_stack_mfma_kernel (f32)      1.59e-6 of 5.46e-6        spatial_generic_kernel (7 configurations)   2.05e-6 of 4.22e-6
  spatial_stack_h3_kernel (h3tiles)    1.31e-6 of 2.19e-5        spatial_stack_p16_kernel (p16)              1.21e-6 of 2.19e-5
127 tests, 2074 checked launches (the rejected calls launch nothing), 10.7 s for the whole file; the slowest tests are the three re-commits
(1.4 s: three uu3d_commit_weights each).

The plane split (check 2): the kernels convert with the wave's f16 denormal mode set to flush, so an f16 result below 2^-14 is a zero of its
sign in either plane, where the numpy h3_split of tests/test_fwd_tiled_gpu.py keeps a denormal lo (3e-8 of value at most, which the MFMA that
reads the plane takes as zero anyway) and writes +0 for a flushed hi.  1 .. 6 elements of a case differ between the two forms; device_split
below states the kernels' form and the check is bitwise on both planes of every element.
Mutations of a scratch copy that check 1 catches (F = 22; error against the bound, p0.1 / p0.5 weights): two elements of p16_kch swapped in the
commit's pack 4.1 / 1.8 of 2.2e-5; the lo plane of one p16 weight fragment (wq, block 1) zeroed 3.3e-4 / 3.2e-5 of 2.2e-5 / 2.4e-5; the GELU
coefficient 4.9867e-2 -> 4.9877e-2 1.2e-4 / 5.5e-5 on both f16x3 kernels.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import uplift_upsample_3dhpe_amd as pkg
from uplift_upsample_3dhpe_amd import _capi
from tests import spatial_util as SU

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

AUTO, F32, H3_TILES, P16 = range(4)
OUT_F32, OUT_PLANES = 0, 1
KNAME = {AUTO: "auto", F32: "f32", H3_TILES: "h3tiles", P16: "p16"}
TOL_H3, TOL_F32_REL, CAP = 2e-5, 2e-6, 1e-4
J, DS, W = 17, 32, 17 * 32
WSETS = {"p0.1": (1, 0.1), "p0.5": (2, 0.5)}           # init_weights (seed, perturb)
F_SWEEP = (1, 2, 3, 4, 6, 7, 8, 13, 14, 15, 22)       # either side of 3 and 7 frames per workgroup, partial last workgroups
LARGE = (3, 5)                                          # indices of the x30 and joint-at-1e3 frames in the pool


# ---- inputs and references: made once, read-only ----
@functools.lru_cache(maxsize=None)
def _pool():
    """22 frames: a uniform frame, the five edge frames (zero, 1e-6, x30, identical joints, one joint at 1e3), 16 more uniform frames."""
    r = SU.make_frames(17, J, 5)
    p = np.concatenate([r[:1], SU.edge_frames(J), r[1:]])
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _reference(name, seed, perturb, frames_key):
    """(float64 S per frame, per-frame max-abs deviation of the float32 oracle from it) for a frame set."""
    _, arch, w = SU.arch_and_weights(name, seed, perturb)
    frames = _frames_of(frames_key)
    ref = SU.spatial_ref64(w, frames, arch.num_heads)
    f32 = SU.spatial_torch(w, frames, arch.num_heads, torch.float32).astype(np.float64)
    dev = np.abs(f32 - ref).max(axis=1)
    ref.setflags(write=False)
    return ref, dev


def _frames_of(key):
    kind, Jn, n, seed = key
    if kind == "pool":
        return _pool()
    if kind == "edges":
        return SU.edge_frames(Jn, seed)
    return SU.make_frames(n, Jn, seed)


def _bounds(ref, dev, idx, large, exact):
    """(bound for the unit-scale frames, bound for the large frames) of the frames idx."""
    out = []
    for grp in ([i for i in idx if i not in large], [i for i in idx if i in large]):
        if not grp:
            out.append(None)
            continue
        scale, d = float(np.abs(ref[grp]).max()), float(dev[grp].max())
        assert scale < 16.0
        b = max(4.0 * d, TOL_F32_REL * scale) if exact else (TOL_H3 * (scale if grp[0] in large else 1.0) + 2.0 * d)
        assert 0.0 < b <= CAP
        out.append(b)
    return out


def _hold(form, got, ref, dev, idx, large, exact):
    """check 1 on rows idx of got (rows of ref with the same numbers)."""
    bu, bl = _bounds(ref, dev, idx, large, exact)
    for grp, b in (([i for i in idx if i not in large], bu), ([i for i in idx if i in large], bl)):
        if not grp:
            continue
        assert np.isfinite(got[grp]).all(), form
        err = float(np.abs(got[grp].astype(np.float64) - ref[grp]).max())
        print(f"{form}: max-abs error {err:.2e} (bound {b:.2e}) on frames {grp[0]} .. {grp[-1]}")
        assert err <= b, (form, err, b, grp)


# ---- handles ----
@functools.lru_cache(maxsize=None)
def _model(name, seed, perturb, precision):
    cfg, arch, w = SU.arch_and_weights(name, seed, perturb)
    return pkg.build_uplift_upsample_transformer(cfg, weights=w, precision=precision, range_guard=False)


def _fresh_model(name, seed, perturb, precision="f16x3"):
    cfg, arch, w = SU.arch_and_weights(name, seed, perturb)
    return pkg.build_uplift_upsample_transformer(cfg, weights=w, precision=precision, range_guard=False)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def device_split(x):
    """The project's split (uu3d_gemm_h3.h; numpy form: h3_split of tests/test_fwd_tiled_gpu.py) as the spatial kernels' conversions give it:
    hi = f16(x), lo = f16((x - hi) * 2048), both round-to-nearest-even, with the wave's f16 denormal mode set to flush
    (h3_flush_f16_denormals): a converted RESULT below the smallest normal half 2^-14 is a zero of its sign.  Against h3_split that changes a
    denormal lo (h3_split keeps it, at most 2^-14 / 2048 = 3e-8 of value; csrc/uu3d_gemm_h3.h: "a denormal lo is read as 0 by the MFMA either
    way: any cvt form will do"), the sign of a flushed hi (h3_split writes +0), and a value just under 2^-14 that rounds up to it (h3_split
    compares the float and writes hi = 0).  Every other element is h3_split's bit for bit."""
    x = np.asarray(x, np.float32)
    tiny = np.float16(2.0 ** -14)

    def cvt(v):
        h = v.astype(np.float16)
        return np.where(np.abs(h) < tiny, np.copysign(np.float16(0), h), h).astype(np.float16)

    hi = cvt(x)
    lo = cvt((x - hi.astype(np.float32)) * np.float32(2048.0))
    return hi, lo


def _launch(model, frames, kernel, layout=OUT_F32, mask=None, width=W, expect=_capi.UU3D_OK):
    """One uu3d_op_spatial_stack call into a NaN-filled buffer with a guard frame.  f32: (S (F, width) f32, guard (width,)); planes:
    (hi (F, width) f16, lo (F, width) f16, guard (width,) f16).  The frame list (mask given) must keep its guard int."""
    F = len(frames)
    ft = torch.from_numpy(np.array(frames)).cuda()
    if layout == OUT_F32:
        out = torch.full(((F + 1) * width,), float("nan"), dtype=torch.float32, device="cuda")
    else:
        out = torch.full(((2 * F + 1) * width,), float("nan"), dtype=torch.float16, device="cuda")
    mt = lt = None
    if mask is not None:
        mt = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).cuda()
        lt = torch.full((F + 2,), -7, dtype=torch.int32, device="cuda")
    st = model._lib.uu3d_op_spatial_stack(model._h, _capi.ptr(ft), F, _capi.ptr(mt), _capi.ptr(lt), kernel, layout, _capi.ptr(out),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == expect, (st, model._lib.uu3d_last_error(model._h).decode())
    o = out.cpu().numpy()
    if st == _capi.UU3D_OK and lt is not None:
        lst = lt.cpu().numpy()
        keep = np.flatnonzero(np.asarray(mask))
        assert lst[F] == len(keep) and np.array_equal(lst[:len(keep)], keep) and lst[F + 1] == -7 and (lst[len(keep):F] == -7).all()
    if layout == OUT_F32:
        return o[:F * width].reshape(F, width), o[F * width:]
    return o[:F * width].reshape(F, width), o[F * width:2 * F * width].reshape(F, width), o[2 * F * width:]


def _twice(model, frames, kernel, layout=OUT_F32, mask=None, width=W):
    """check 5: the launch made twice, the same bits (NaN rows included); the guard still NaN."""
    a, b = _launch(model, frames, kernel, layout, mask, width), _launch(model, frames, kernel, layout, mask, width)
    assert all(_same(x, y) for x, y in zip(a, b)), (KNAME[kernel], layout)
    assert np.isnan(a[-1]).all()
    return a


def _masks(F):
    m = {"alternating": np.arange(F) % 2 == 0, "every5th": np.arange(F) % 5 == 4, "first": np.arange(F) == 0, "last": np.arange(F) == F - 1,
         "none_kept": np.zeros(F, bool)}
    return {k: np.where(v, 255 if k == "every5th" else 1, 0).astype(np.uint8) for k, v in m.items()}       # (any nonzero byte keeps a frame)


def _check_masked(model, frames, kernel, layout, mask, plain):
    got = _twice(model, frames, kernel, layout, mask)
    keep = mask != 0
    for g, p in zip(got[:-1], plain[:-1]):
        assert _same(g[keep], p[keep]) and np.isnan(g[~keep]).all(), (KNAME[kernel], layout, mask)


# ---- checks 1, 2, 4, 5 over the frame sweep ----
@pytest.mark.parametrize("wset", sorted(WSETS))
@pytest.mark.parametrize("F", F_SWEEP)
@pytest.mark.parametrize("kernel", [F32, H3_TILES, P16], ids=lambda k: KNAME[k])
def test_kernel_form_against_float64(kernel, F, wset):
    seed, perturb = WSETS[wset]
    model = _model("h36m_351", seed, perturb, "f16x3")
    ref, dev = _reference("h36m_351", seed, perturb, ("pool", J, 22, 0))
    frames = _pool()[:F]
    plain = _twice(model, frames, kernel)
    _hold(KNAME[kernel], plain[0], ref, dev, list(range(F)), LARGE, exact=kernel == F32)
    planes = None
    if kernel != F32:
        planes = _twice(model, frames, kernel, OUT_PLANES)
        hi, lo = device_split(plain[0])
        bad = np.argwhere((_bits(planes[0]) != _bits(hi)) | (_bits(planes[1]) != _bits(lo)))
        report = [(tuple(i), float(plain[0][tuple(i)]).hex(), float(planes[0][tuple(i)]), float(hi[tuple(i)]),
                   float(planes[1][tuple(i)]), float(lo[tuple(i)])) for i in bad[:6]]
        assert len(bad) == 0, (len(bad), report)                 # check 2: (index, f32, hi, split hi, lo, split lo)
        back = planes[0].astype(np.float64) + planes[1].astype(np.float64) / 2048.0
        assert np.abs(back - plain[0]).max() <= 2.0 ** -20 * max(1.0, np.abs(plain[0]).max())
    masks = _masks(F)
    for name in sorted(masks):                                                           # check 4
        _check_masked(model, frames, kernel, OUT_F32, masks[name], plain)
        if planes is not None:
            _check_masked(model, frames, kernel, OUT_PLANES, masks[name], planes)


def test_exact_f32_kernel_on_a_handle_of_precision_f32():
    """The f32 kernel reads no f16 fragment: a handle of precision f32 gives the bits of the f16x3 handle's forced f32 kernel; AUTO is that kernel."""
    seed, perturb = WSETS["p0.1"]
    frames = _pool()
    a = _twice(_model("h36m_351", seed, perturb, "f32"), frames, AUTO)
    b = _twice(_model("h36m_351", seed, perturb, "f16x3"), frames, F32)
    assert _same(a[0], b[0])
    ref, dev = _reference("h36m_351", seed, perturb, ("pool", J, 22, 0))
    _hold("f32", a[0], ref, dev, list(range(22)), LARGE, exact=True)


# ---- check 3 ----
@pytest.mark.parametrize("kernel", [F32, H3_TILES, P16], ids=lambda k: KNAME[k])
def test_slot_independence(kernel):
    seed, perturb = WSETS["p0.1"]
    model = _model("h36m_351", seed, perturb, "f16x3")
    probe = _pool()[6]
    layouts = [OUT_F32] if kernel == F32 else [OUT_F32, OUT_PLANES]
    alone = {lay: _twice(model, probe[None], kernel, lay) for lay in layouts}
    others = SU.make_frames(14, J, 77)
    for i in range(14):
        frames = others.copy()
        frames[i] = probe
        mask = np.zeros(14, np.uint8)
        mask[[i, (i + 5) % 14]] = 1
        for lay in layouts:
            dense, masked = _twice(model, frames, kernel, lay), _twice(model, frames, kernel, lay, mask)
            for part in range(len(alone[lay]) - 1):
                assert _same(dense[part][i], alone[lay][part][0]), (KNAME[kernel], lay, i)
                assert _same(masked[part][i], alone[lay][part][0]), (KNAME[kernel], lay, i, "masked")
                assert np.isnan(masked[part][mask == 0]).all()


# ---- check 6 ----
@pytest.mark.parametrize("kernel", [F32, H3_TILES, P16], ids=lambda k: KNAME[k])
def test_recommitted_weights_reach_the_kernel(kernel):
    model = _fresh_model("h36m_351", *WSETS["p0.1"])
    frames = _pool()[:8]
    runs = []
    for wset in ("p0.1", "p0.5", "p0.1"):
        seed, perturb = WSETS[wset]
        model.set_weights_dict(SU.arch_and_weights("h36m_351", seed, perturb)[2])
        S = _twice(model, frames, kernel)[0]
        ref, dev = _reference("h36m_351", seed, perturb, ("pool", J, 22, 0))
        _hold(KNAME[kernel], S, ref, dev, list(range(8)), LARGE, exact=kernel == F32)
        runs.append(S)
    assert _same(runs[0], runs[2]) and not _same(runs[0], runs[1])


# ---- check 7 ----
def h3_pays(F):
    """spatial_h3_pays of csrc/uu3d_forward.inc, restated: rounds of resident workgroups (3 frames each) x the time of a round."""
    wgs = (F + 2) // 3
    return -(-wgs // 1536) * 68 <= -(-wgs // 1792) * 133


def choice_rule(F, precision, exact_f32, spatial, no_planes):
    """spatial_stage's decision, restated: (kernel, planes)."""
    h3 = precision == "f16x3" and not exact_f32 and spatial != "f32" and (spatial == "h3" or h3_pays(F))
    kernel = F32 if not h3 else (H3_TILES if spatial == "h3tiles" else P16)
    return kernel, int(h3 and not no_planes and (J * DS) % 32 == 0)


def _choice(model, F, schedule):
    k, p = C.c_int32(-1), C.c_int32(-1)
    assert model._lib.uu3d_op_spatial_choice(model._h, F, schedule, C.byref(k), C.byref(p)) == _capi.UU3D_OK
    return k.value, p.value


BOUNDARY_F = (1, 3 * 1536 - 1, 3 * 1536, 3 * 1536 + 1, 3 * 1792 - 1, 3 * 1792, 3 * 1792 + 1, 3 * 3072, 3 * 3072 + 1, 3 * 3584, 3 * 3584 + 1, 200000)


def test_the_pays_rule_has_the_boundaries_the_docstring_names():
    assert [F for F in range(1, 20000) if not h3_pays(F)] == list(range(4609, 5377))


@pytest.mark.parametrize("no_planes", [False, True], ids=["planes", "no_planes"])
@pytest.mark.parametrize("spatial", ["", "f32", "h3", "h3tiles"])
def test_choice_matches_the_rule_and_auto_runs_what_it_names(spatial, no_planes, monkeypatch):
    if spatial:
        monkeypatch.setenv("UU3D_SPATIAL", spatial)
    else:
        monkeypatch.delenv("UU3D_SPATIAL", raising=False)
    if no_planes:
        monkeypatch.setenv("UU3D_NO_PLANES", "1")
    else:
        monkeypatch.delenv("UU3D_NO_PLANES", raising=False)
    for precision in ("f16x3", "f32"):
        model = _fresh_model("h36m_351", *WSETS["p0.1"], precision=precision)           # (the switches are read by uu3d_create)
        for F in BOUNDARY_F:
            for sched in (0, 1, _capi.UU3D_SCHEDULE_EXACT_F32, 1 | _capi.UU3D_SCHEDULE_EXACT_F32):
                want = choice_rule(F, precision, bool(sched & _capi.UU3D_SCHEDULE_EXACT_F32), spatial, no_planes)
                assert _choice(model, F, sched) == want, (spatial, no_planes, precision, F, sched)
        named = _choice(model, 8, 0)[0]
        a, b = _twice(model, _pool()[:8], AUTO), _twice(model, _pool()[:8], named)
        assert _same(a[0], b[0])
        if precision == "f16x3":
            others = [k for k in (F32, H3_TILES, P16) if k != named]
            assert all(not _same(a[0], _twice(model, _pool()[:8], k)[0]) for k in others)       # the three kernels round differently


@pytest.mark.parametrize("F,named", [(3 * 1536 + 1, F32), (3 * 1792 + 1, P16)])
def test_large_launch(F, named):
    """Hundreds of workgroups: the choice at the boundary, AUTO = the kernel it names bitwise, and six frames -- two each from the first, a middle
    and the last workgroup (the last one partial for every kernel: F = 1 mod 3, F = 1 and 3 mod 7) -- of every kernel against float64."""
    seed, perturb = WSETS["p0.1"]
    model = _model("h36m_351", seed, perturb, "f16x3")
    assert _choice(model, F, 0) == (named, int(named != F32)) and _choice(model, F - 1, 0)[0] != named
    key = ("uniform", J, F, 4242)
    frames = _frames_of(key)
    idx = [0, 1, F // 2, F // 2 + 1, F - 2, F - 1]
    _, arch, w = SU.arch_and_weights("h36m_351", seed, perturb)
    ref = np.zeros((F, W))
    ref[idx] = SU.spatial_ref64(w, frames[idx], 8)
    dev = np.zeros(F)
    dev[idx] = np.abs(SU.spatial_torch(w, frames[idx], 8, torch.float32).astype(np.float64) - ref[idx]).max(axis=1)
    auto = _twice(model, frames, AUTO)
    for kernel in (F32, H3_TILES, P16):
        S = _twice(model, frames, kernel)
        assert np.isfinite(S[0]).all()
        _hold(KNAME[kernel], S[0], ref, dev, idx, (), exact=kernel == F32)
        assert _same(S[0], auto[0]) == (kernel == named)


# ---- rejections: an error before any launch, the output untouched ----
def test_rejections_leave_the_output_untouched():
    lib = _capi.load_library()
    model = _fresh_model("h36m_351", *WSETS["p0.1"])
    m32 = _model("h36m_351", *WSETS["p0.1"], "f32")
    gen = _model("depth1", 11, 0.1, "f16x3")
    frames = _pool()[:4]
    INV, NOT_READY = _capi.UU3D_ERR_INVALID_ARGUMENT, _capi.UU3D_ERR_NOT_READY

    def untouched(res):
        assert all(np.isnan(r).all() for r in res)

    untouched(_launch(model, frames, F32, OUT_PLANES, expect=INV))                        # planes asked of the exact-f32 kernel
    untouched(_launch(model, frames, 4, expect=INV))
    untouched(_launch(model, frames, -1, expect=INV))
    untouched(_launch(model, frames, P16, 2, expect=INV))
    untouched(_launch(m32, frames, P16, expect=INV))                                      # no f16 fragments on a handle of precision f32
    untouched(_launch(m32, frames, H3_TILES, expect=INV))
    untouched(_launch(m32, frames, AUTO, OUT_PLANES, expect=INV))
    gframes = SU.make_frames(4, 17, 1)
    for kernel in (F32, H3_TILES, P16):                                                   # forced kernels on dims that are not the compiled ones
        untouched(_launch(gen, gframes, kernel, width=17 * 16, expect=INV))
    untouched(_launch(gen, gframes, AUTO, OUT_PLANES, width=17 * 16, expect=INV))
    untouched(_launch(gen, gframes, AUTO, mask=np.ones(4, np.uint8), width=17 * 16, expect=INV))
    # null pointers, F < 1, a mask without a list
    ft = torch.from_numpy(np.array(frames)).cuda()
    out = torch.full((5 * W,), float("nan"), device="cuda")
    mt = torch.ones(4, dtype=torch.uint8, device="cuda")
    p, s = _capi.ptr, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.uu3d_op_spatial_stack(None, p(ft), 4, None, None, P16, 0, p(out), s) == INV
    assert lib.uu3d_op_spatial_stack(model._h, None, 4, None, None, P16, 0, p(out), s) == INV
    assert lib.uu3d_op_spatial_stack(model._h, p(ft), 4, None, None, P16, 0, None, s) == INV
    assert lib.uu3d_op_spatial_stack(model._h, p(ft), 0, None, None, P16, 0, p(out), s) == INV
    assert lib.uu3d_op_spatial_stack(model._h, p(ft), -3, None, None, P16, 0, p(out), s) == INV
    assert lib.uu3d_op_spatial_stack(model._h, p(ft), 4, p(mt), None, P16, 0, p(out), s) == INV
    k, pl = C.c_int32(), C.c_int32()
    assert lib.uu3d_op_spatial_choice(model._h, 0, 0, C.byref(k), C.byref(pl)) == INV
    assert lib.uu3d_op_spatial_choice(model._h, 8, 2, C.byref(k), C.byref(pl)) == INV
    assert lib.uu3d_op_spatial_choice(model._h, 8, 0, None, C.byref(pl)) == INV
    assert lib.uu3d_op_spatial_choice(gen._h, 8, 0, C.byref(k), C.byref(pl)) == INV
    assert lib.uu3d_op_compact_frames(None, 4, p(out), s) == INV and lib.uu3d_op_compact_frames(p(mt), 4, None, s) == INV
    assert lib.uu3d_op_compact_frames(p(mt), 0, p(out), s) == INV
    # an uncommitted handle: a weight set since the last commit
    name, shape = model._spec[0]
    a = np.zeros(shape, np.float32)
    assert lib.uu3d_set_weight(model._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size) == _capi.UU3D_OK
    assert lib.uu3d_op_spatial_stack(model._h, p(ft), 4, None, None, P16, 0, p(out), s) == NOT_READY
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ---- the generic kernel ----
def _generic_frames(name, seed):
    Jn = SU.GENERIC[name][0]
    return {1: ("uniform", Jn, 1, seed), 2: ("uniform", Jn, 2, seed + 1), 5: ("edges", Jn, 5, seed)}


@pytest.mark.parametrize("name", sorted(SU.GENERIC))
def test_generic_kernel_against_float64(name):
    Jn, ds = SU.GENERIC[name][0], SU.GENERIC[name][1]
    model = _model(name, 11, 0.1, "f16x3")
    for F, key in _generic_frames(name, 3).items():
        frames = _frames_of(key)
        ref, dev = _reference(name, 11, 0.1, key)
        S = _twice(model, frames, AUTO, width=Jn * ds)[0]
        _hold("generic", S, ref, dev, list(range(F)), (2, 4) if key[0] == "edges" else (), exact=True)
        if F > 1:                                                                        # frame independence: a permutation of the frames, bitwise
            perm = np.roll(np.arange(F), 2)
            Sp = _twice(model, frames[perm], AUTO, width=Jn * ds)[0]
            assert _same(Sp, S[perm])


def test_generic_handle_with_the_compiled_spatial_weights():
    """J 17 / d_s 32 / 8 heads at d_t 256: the compiled spatial function on the generic kernel.  With h36m_351's spatial tensors its S meets that
    model's float64 reference, and the exact-f32 compiled kernel agrees with it inside the two bounds."""
    seed, perturb = WSETS["p0.1"]
    w351 = SU.arch_and_weights("h36m_351", seed, perturb)[2]
    w = dict(SU.arch_and_weights("compiled_dt256", 11, 0.1)[2])
    for k in w:
        if k.startswith(("keypoint_embedding/", "spatial_pe/", "spatial_block_", "spatial_norm/")):
            assert w[k].shape == w351[k].shape
            w[k] = w351[k]
    model = _fresh_model("compiled_dt256", 11, 0.1)
    model.set_weights_dict(w)
    ref, dev = _reference("h36m_351", seed, perturb, ("pool", J, 22, 0))
    S = _twice(model, _pool(), AUTO)[0]
    _hold("generic", S, ref, dev, list(range(22)), LARGE, exact=True)


@pytest.mark.parametrize("name", sorted(SU.GENERIC))
def test_generic_recommit(name):
    Jn, ds = SU.GENERIC[name][0], SU.GENERIC[name][1]
    model = _fresh_model(name, 11, 0.1)
    key = ("uniform", Jn, 2, 9)
    runs = []
    for seed, perturb in ((11, 0.1), (12, 0.5), (11, 0.1)):
        model.set_weights_dict(SU.arch_and_weights(name, seed, perturb)[2])
        S = _twice(model, _frames_of(key), AUTO, width=Jn * ds)[0]
        ref, dev = _reference(name, seed, perturb, key)
        _hold("generic", S, ref, dev, [0, 1], (), exact=True)
        runs.append(S)
    assert _same(runs[0], runs[2]) and not _same(runs[0], runs[1])


# ---- compact_frames_kernel ----
def _compact(mask_np, offset):
    """mask at `offset` bytes past a 16-byte aligned address -> the list (total + 2 ints, sentinel -7)."""
    total = len(mask_np)
    buf = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    base = (-buf.data_ptr()) % 16 + offset
    view = buf[base:base + total]
    assert (view.data_ptr() - offset) % 16 == 0
    view.copy_(torch.from_numpy(mask_np))
    lst = torch.full((total + 2,), -7, dtype=torch.int32, device="cuda")
    st = _capi.load_library().uu3d_op_compact_frames(_capi.ptr(view), total, _capi.ptr(lst), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == _capi.UU3D_OK
    return lst.cpu().numpy()


@pytest.mark.parametrize("offset", [0, 1, 8])
@pytest.mark.parametrize("total", [1, 15, 16, 17, 1023, 16383, 16384, 16385, 32768 + 5])
def test_compact_frames(total, offset):
    """16384 frames = one pass of 1024 threads x 16 bytes; offsets 1 and 8 leave the 16-byte fast path for every thread."""
    rng = np.random.default_rng(total + offset)
    dens = {"ones": np.ones(total, np.uint8), "zeros": np.zeros(total, np.uint8),
            "random": rng.choice(np.array([0, 0, 1, 7, 255], np.uint8), size=total), "last": np.zeros(total, np.uint8)}
    dens["last"][-1] = 255
    for name, mask in dens.items():
        want = np.flatnonzero(mask)
        for _ in range(2):
            lst = _compact(mask, offset)
            n = len(want)
            assert lst[total] == n and np.array_equal(lst[:n], want), (name, total, offset)
            assert (lst[n:total] == -7).all() and lst[total + 1] == -7, (name, total, offset)

