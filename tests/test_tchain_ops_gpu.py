"""GPU: every launch form of the temporal chain (tchain16_kernel<FLAGS>, csrc/uu3d_tchain16.h) on its own through uu3d_op_tchain
(include/uu3d_ops.h), against a float64 restatement of the same stages from the NAMED weights (tests/tchain_util.py: unfolded gamma / beta, the
unscaled wq with q's scale applied at the end).  The operator runs on a committed handle's own weight stream and parameter table, so the
commit's fold and pack (csrc/uu3d_commit.inc) are under test with the kernel, and it launches through launch_tchain (csrc/uu3d_launch.h), as
the forward's Launcher::tchain does.

Handles: config/h36m_81.json (41 tokens: the positional encoding's period wraps inside a tile) with two temporal blocks, precision f16x3;
A with its strided blocks (launches QKV | PROJ MLP QKV | PROJ MLP QKV PE | PROJ FC1_PLANES), B without (its last launch: PROJ MLP).
Every form runs at M in {1, 15, 16, 17, 48, 49, 63, 64, 65, 129, 191}: one live row, wholly dead panel waves (M % 64 <= 48), boundaries on a
16-token panel edge, M < 64, one to three workgroups.

Each block is held on its own -- a stage that follows a stored intermediate is referenced from what the device stored (the kernel stores the
tile before that LayerNorm), so one stage's error is not charged to the next:
  x + projection (XA of the strided form)                 2e-5   from x_in and the attention output
  x_out of an MLP form (projection, fc1, fc2)             6e-5   from x_in and the attention output
  q | k | v (planes as hi + lo / 2048; q on its scaled value)   2e-5   from the float64 LayerNorm of the residual tile the launch stored
  H planes of the strided form                            2e-5   from the XA the launch stored
  stored x + pe tile                                      exact (float32 add) against the stored x
2e-5 is the bound of tests/test_panel_op_gpu.py and tests/test_fwd_ops_gpu.py for one LayerNorm + Dense layer on unit-scale outputs; 6e-5 is
three such layers.  tests/test_tchain_emulation_cpu.py shows on the CPU that a faithful emulation of the arithmetic stays within half of each
and that one dropped cross term in one stage exceeds it 10 to 50 times.
Every buffer is NaN-filled and carries a guard.  Each case prints its measured maxima."""
import ctypes as C
import functools

import numpy as np
import pytest

import uplift_upsample_3dhpe_amd as pkg
from uplift_upsample_3dhpe_amd import _capi
from tests import tchain_util as T
from tests.test_tchain_gpu import _model as _chain_model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K, HT, G = T.K, T.HT, 2          # G: guard rows behind row-major buffers
GUARD = 4096                     # guard elements behind q and the scratch
OK, INV, UNSUP, NOT_READY = _capi.UU3D_OK, _capi.UU3D_ERR_INVALID_ARGUMENT, _capi.UU3D_ERR_UNSUPPORTED, _capi.UU3D_ERR_NOT_READY
# form -> (handle with strided blocks, launch, block whose projection / MLP run, block whose LayerNorm 1 + QKV run)
LAUNCH = {"qkv": (True, 0, None, T.block(False, 0)),
          "proj_mlp_qkv": (True, 1, T.block(False, 0), T.block(False, 1)),
          "proj_mlp_qkv_pe": (True, 2, T.block(False, 1), T.block(True, 0)),
          "proj_fc1_planes": (True, 3, T.block(True, 0), None),
          "proj_mlp": (False, 2, T.block(False, 1), None)}


@functools.lru_cache(maxsize=None)
def _handle(strided):
    model = _chain_model(T.config(strided), T.weights(strided))
    flags = (C.c_int32 * 8)()
    n = model._lib.uu3d_op_tchain_launches(model._h, flags, 8)
    P, Mp, Q, F1, PE = T.TC_PROJ, T.TC_MLP, T.TC_QKV, T.TC_FC1_PLANES, T.TC_PE
    want = [Q, P | Mp | Q, P | Mp | Q | PE, P | F1] if strided else [Q, P | Mp | Q, P | Mp]
    assert n == len(want) and list(flags[:n]) == want, (n, list(flags[:8]))
    return model


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _pad(a, rows):
    """rows past len(a): its last row (what a launch in front of this one leaves in a whole tile)."""
    return np.ascontiguousarray(np.concatenate([a, np.repeat(a[-1:], rows - len(a), axis=0)]))


def _nan(n, dtype):
    return torch.full((n,), float("nan"), dtype=dtype, device="cuda")


def _launch(form, x, o_hi, o_lo, scratch=None, nulls=(), expect=OK, model=None, launch=None, M=None):
    """One uu3d_op_tchain call of `form` on rows x (and the attention-output planes) into NaN-filled buffers with guards.  scratch: a device
    scratch another launch left (else: NaN, with x as the residual tile of a form that reads one).  Returns the host copies."""
    strided, li, _, _ = LAUNCH[form]
    flags = T.FORMS[form]
    model = model or _handle(strided)
    lib = model._lib
    Mx = len(x)                                                                          # the buffers' rows; M: what the call is given
    M = Mx if M is None else M
    R, R128, Rp = (Mx + 63) // 64 * 64, (Mx + 127) // 128 * 128, (Mx + 31) // 32 * 32
    xd = _nan((Mx + G) * K, torch.float32)
    if not flags & T.TC_PROJ:
        xd[:Mx * K] = torch.from_numpy(np.array(x, np.float32).ravel()).cuda()
    xad = _nan((Mx + G) * K, torch.float32)
    hd = _nan((2 * Mx + G) * HT, torch.float16)
    qn = int(lib.uu3d_op_attn_qf_bytes(Mx)) // 2
    qd = _nan(qn + GUARD, torch.float16)
    sn = int(lib.uu3d_op_tchain_scratch_bytes(Mx)) // 4
    in_slot = 1 if flags & T.TC_FC1_PLANES else 0
    if scratch is None:
        sh = np.full(sn + GUARD, np.nan, np.float32)
        if flags & T.TC_PROJ:
            assert lib.uu3d_op_tchain_xs_pack(_p(_pad(np.asarray(x, np.float32), R)), Mx, in_slot, R, _p(sh)) == 0
        scratch = torch.from_numpy(sh).cuda()
    fh = np.full(int(lib.uu3d_op_panel_a_bytes(Mx)) // 2, np.nan, np.float16)
    assert lib.uu3d_op_panel_a_pack(_p(_pad(o_hi.astype(np.float32), Rp)), _p(_pad(o_lo.astype(np.float32), Rp)), Rp, _p(fh)) == 0
    od = torch.from_numpy(fh).cuda()
    before = scratch.cpu().numpy().copy()
    args = {"o": od, "x": xd, "xa": xad, "q": qd, "h": hd, "s": scratch}
    ptr = {k: (None if k in nulls else _capi.ptr(v)) for k, v in args.items()}
    st = lib.uu3d_op_tchain(None if "model" in nulls else model._h, li if launch is None else launch, M, ptr["o"], ptr["x"], ptr["xa"], ptr["q"], ptr["h"],
                            ptr["s"], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == expect, (form, M, st, lib.uu3d_last_error(model._h).decode())
    out = {"X": xd.cpu().numpy().reshape(Mx + G, K), "XA": xad.cpu().numpy().reshape(Mx + G, K), "scratch_dev": scratch, "before": before}
    h = hd.cpu().numpy()
    out["Hh"], out["Hl"], out["Hguard"] = h[:Mx * HT].reshape(Mx, HT), h[Mx * HT:2 * Mx * HT].reshape(Mx, HT), h[2 * Mx * HT:]
    q = qd.cpu().numpy()
    out["Qraw"], out["Qguard"] = q[:qn], q[qn:]
    qh, ql = np.empty((R128, 3 * K), np.float16), np.empty((R128, 3 * K), np.float16)
    assert lib.uu3d_op_attn_qf_unpack(_p(np.ascontiguousarray(q[:qn])), R128, _p(qh), _p(ql)) == 0
    out["Qh"], out["Ql"] = qh, ql
    s = scratch.cpu().numpy()
    out["Sraw"], out["Sguard"] = s[:sn], s[sn:]
    for slot in (0, 1):
        t = np.empty((R, K), np.float32)
        assert lib.uu3d_op_tchain_xs_unpack(_p(np.ascontiguousarray(s[:sn])), Mx, slot, R, _p(t)) == 0
        out["S%d" % slot] = t
    return out


def _untouched(out, x_in=None):
    """Nothing was written: every buffer NaN (x_in: the rows x_dev was given, for a form that reads them), the scratch as it was."""
    for k in ("X", "XA", "Hh", "Hl", "Hguard", "Qraw", "Qguard"):
        if k == "X" and x_in is not None:
            assert _same(out[k][:len(x_in)], x_in) and np.isnan(out[k][len(x_in):]).all()
        else:
            assert np.isnan(out[k]).all(), k
    assert _same(out["Sraw"], out["before"][:len(out["Sraw"])]) and np.isnan(out["Sguard"]).all()


@functools.lru_cache(maxsize=None)
def _case(form, M):
    x, o_hi, o_lo = T.pool()
    return _launch(form, x[:M], o_hi[:M], o_lo[:M])


def _footprint(form, M, out, x):
    flags = T.FORMS[form]
    R = (M + 63) // 64 * 64
    tiles = R // 64
    stores_x = bool(flags & T.TC_MLP) and (not flags & T.TC_QKV or bool(flags & T.TC_PE))
    planes = bool(flags & T.TC_FC1_PLANES)
    assert np.isnan(out["X"][M:]).all() and np.isnan(out["XA"][M:]).all() and np.isnan(out["Hguard"]).all(), "rows >= M of a row-major buffer"
    assert np.isnan(out["Qguard"]).all() and np.isnan(out["Sguard"]).all(), "behind uu3d_op_attn_qf_bytes(M) / uu3d_op_tchain_scratch_bytes(M)"
    if not flags & T.TC_PROJ:
        assert _same(out["X"][:M], x)                                                    # read, not written
    else:
        assert np.isfinite(out["X"][:M]).all() if stores_x else np.isnan(out["X"][:M]).all()
    for k in ("XA", "Hh", "Hl"):
        assert np.isfinite(out[k][:M]).all() if planes else np.isnan(out[k]).all(), k
    if flags & T.TC_QKV:
        for k in ("Qh", "Ql"):
            assert np.isfinite(out[k][:R]).all() and np.isnan(out[k][R:]).all(), k      # whole 64-row tiles, nothing beyond the last one
    else:
        assert np.isnan(out["Qraw"]).all()
    n = tiles * 64 * K
    before = out["before"]
    written = None if not flags & T.TC_QKV and flags & T.TC_PROJ else (1 if flags & T.TC_PE else 0)
    for slot in (0, 1):
        if slot == written:
            assert np.isfinite(out["S%d" % slot]).all(), "the stored residual tiles are whole"
        else:
            assert _same(out["Sraw"][slot * n:(slot + 1) * n], before[slot * n:(slot + 1) * n]), "the other slot is left as it was"
    if form == "qkv" and M < R:                                                          # rows past M: the clamped row's values
        assert _same(out["S0"][M:], np.repeat(x[M - 1:M], R - M, axis=0))
        for k in ("Qh", "Ql"):
            assert _same(out[k][M:R], np.repeat(out[k][M - 1:M], R - M, axis=0)), k


def _errors(form, M, out, x, o_val):
    """{quantity: (max-abs error against float64, bound)} of one case; the exact checks are asserted here."""
    w = T.weights(LAUNCH[form][0])
    _, _, p, p_next = LAUNCH[form]
    flags = T.FORMS[form]
    e = {}
    if form == "qkv":
        assert _same(out["S0"][:M], x)
        ln_in = out["S0"][:M]
    if flags & T.TC_MLP:
        got = out["X"][:M] if (not flags & T.TC_QKV or flags & T.TC_PE) else out["S0"][:M]
        e["x_out"] = (np.abs(T.f64(got) - T.ref_mlp(w, p, T.ref_proj(w, p, x, o_val))).max(), T.TOL_X)
        ln_in = got
        if flags & T.TC_PE:
            pe = np.asarray(w["strided_temporal_pe_1/positional_encoding_weights"])
            ln_in = out["S1"][:M]
            assert _same(ln_in, out["X"][:M] + pe[np.arange(M) % T.PERIOD]), "x + pe[token % period] in float32"
    if flags & T.TC_FC1_PLANES:
        e["xa"] = (np.abs(T.f64(out["XA"][:M]) - T.ref_proj(w, p, x, o_val)).max(), T.TOL)
        e["h"] = (np.abs(T.planes_value(out["Hh"], out["Hl"]) - T.ref_fc1(w, p, out["XA"][:M])).max(), T.TOL)
    if flags & T.TC_QKV:
        e["qkv"] = (np.abs(T.planes_value(out["Qh"][:M], out["Ql"][:M]) - T.ref_qkv(w, p_next, ln_in)).max(), T.TOL)
    return e


@pytest.mark.parametrize("M", T.M_SWEEP)
@pytest.mark.parametrize("form", sorted(LAUNCH))
def test_form_against_float64(form, M):
    x, o_hi, o_lo = T.pool()
    out = _case(form, M)
    _footprint(form, M, out, x[:M])
    e = _errors(form, M, out, x[:M], T.planes_value(o_hi[:M], o_lo[:M]))
    print(f"tchain {form} M={M}: " + ", ".join(f"{k} {v:.2e} of {b:.0e}" for k, (v, b) in e.items()))
    for k, (v, b) in e.items():
        assert v <= b, (form, M, k, v, b)


def _row_outputs(form, out, rows):
    flags = T.FORMS[form]
    keys = []
    if flags & T.TC_QKV:
        keys += ["Qh", "Ql", "S1" if flags & T.TC_PE else "S0"]
    if flags & T.TC_MLP and (not flags & T.TC_QKV or flags & T.TC_PE):
        keys += ["X"]
    if flags & T.TC_FC1_PLANES:
        keys += ["XA", "Hh", "Hl"]
    return {k: out[k][rows] for k in keys}


@pytest.mark.parametrize("form", sorted(LAUNCH))
def test_rows_do_not_depend_on_m_position_or_neighbours(form):
    """Rows of the M = 191 case, permuted, as the M = 129 and the M = 64 case: every output of a row has the same bits.  (A row keeps its token
    index modulo the period, which the positional encoding of the PE form reads; 41 moves it to another lane, panel and tile.)  And the same
    call twice gives the same bits in every buffer (the trash page, which every dead lane writes, aside)."""
    x, o_hi, o_lo = T.pool()
    base = _case(form, T.POOL)
    rng = np.random.default_rng(3)
    for M in (129, 64):
        idx = np.empty(M, np.int64)
        for r in range(T.PERIOD):
            pos = np.arange(r, M, T.PERIOD)
            idx[pos] = rng.permutation(np.arange(r, T.POOL, T.PERIOD))[:len(pos)]
        assert len(np.unique(idx)) == M and (idx != np.arange(M)).sum() > M // 2
        out = _launch(form, x[idx], o_hi[idx], o_lo[idx])
        got, want = _row_outputs(form, out, np.arange(M)), _row_outputs(form, base, idx)
        assert got, form
        for k in got:
            assert _same(got[k], want[k]), (form, M, k)
    again = _launch(form, x[idx], o_hi[idx], o_lo[idx])
    n = 2 * 64 * K                                                                       # M = 64: one tile per slot, then the trash page
    for k in ("X", "XA", "Hh", "Hl", "Qraw"):
        assert _same(again[k], out[k]), (form, k)
    assert _same(again["Sraw"][:n], out["Sraw"][:n])


def test_dead_lanes_do_not_reach_live_rows():
    """NaN in what only dead lanes read -- the attention-output rows past M of the last panel, the residual tile's rows past M -- leaves every
    live row's bits as they were (lane-local arithmetic; LayerNorm's sums stay inside a token)."""
    x, o_hi, o_lo = T.pool()
    M = 17
    lib = _handle(True)._lib
    for form in ("proj_mlp_qkv_pe", "proj_fc1_planes"):
        base = _case(form, M)
        R, Rp = 64, 32
        sh = np.full(int(lib.uu3d_op_tchain_scratch_bytes(M)) // 4 + GUARD, np.nan, np.float32)
        assert lib.uu3d_op_tchain_xs_pack(_p(np.ascontiguousarray(x[:M])), M, 1 if form == "proj_fc1_planes" else 0, M, _p(sh)) == 0
        nan_rows = np.full((Rp - M, K), np.nan, np.float16)
        out = _launch(form, x[:M], np.concatenate([o_hi[:M], nan_rows]), np.concatenate([o_lo[:M], nan_rows]), scratch=torch.from_numpy(sh).cuda())
        got, want = _row_outputs(form, out, np.arange(M)), _row_outputs(form, base, np.arange(M))
        for k in got:
            assert _same(got[k], want[k]), (form, k)
        assert np.isnan(out["X"][M:]).all() and np.isnan(out["XA"][M:]).all() and np.isnan(out["Hguard"]).all()


def test_handoff_between_two_launches():
    """Launch 0 then launch 1 on the same scratch, no host repack: x_out of launch 1 against float64 from the row-major input."""
    x, o_hi, o_lo = T.pool()
    M = 129
    w = T.weights(True)
    first = _launch("qkv", x[:M], o_hi[:M], o_lo[:M])
    out = _launch("proj_mlp_qkv", x[:M], o_hi[:M], o_lo[:M], scratch=first["scratch_dev"])
    p = T.block(False, 0)
    err = np.abs(T.f64(out["S0"][:M]) - T.ref_mlp(w, p, T.ref_proj(w, p, x[:M], T.planes_value(o_hi[:M], o_lo[:M])))).max()
    print(f"tchain handoff M={M}: x_out {err:.2e} of {T.TOL_X:.0e}")
    assert err <= T.TOL_X
    assert _same(out["S0"], _case("proj_mlp_qkv", M)["S0"])                              # the tile launch 0 stored is the tile the host packs


def test_rejected_calls_launch_nothing():
    x, o_hi, o_lo = T.pool()
    M = 17
    a = (x[:M], o_hi[:M], o_lo[:M])
    _untouched(_launch("qkv", *a, nulls=("model",), expect=INV), x[:M])
    for bad_m in (0, -5):
        _untouched(_launch("proj_mlp_qkv", *a, M=bad_m, expect=INV))
    for launch in (-1, 4, 100):
        _untouched(_launch("proj_mlp_qkv", *a, launch=launch, expect=INV))
    _untouched(_launch("proj_mlp", *a, launch=3, expect=INV))                            # the handle without strided blocks has three launches
    needs = {"qkv": ("x", "q", "s"), "proj_mlp_qkv": ("o", "q", "s"), "proj_mlp_qkv_pe": ("o", "x", "q", "s"), "proj_mlp": ("o", "x", "s"),
             "proj_fc1_planes": ("o", "xa", "h", "s")}
    for form, names in needs.items():
        for nm in names:
            _untouched(_launch(form, *a, nulls=(nm,), expect=INV), x[:M] if form == "qkv" else None)
        spare = tuple(k for k in ("o", "x", "xa", "q", "h") if k not in names)         # pointers the stage set does not use may be null
        ok = _launch(form, *a, nulls=spare)
        want = _case(form, M)
        for k in ("X", "XA", "Hh", "Hl", "Qraw"):
            assert _same(ok[k], want[k]), (form, k)
    # a handle of precision f32 has no chain
    m32 = pkg.build_uplift_upsample_transformer(T.config(True), weights=T.weights(True), precision="f32")
    assert m32._lib.uu3d_op_tchain_launches(m32._h, None, 0) == 0
    _untouched(_launch("proj_mlp_qkv", *a, model=m32, expect=UNSUP))
    assert _handle(True)._lib.uu3d_op_tchain_launches(None, None, 0) == -1
    # an uncommitted handle: a weight set since the last commit
    fresh = _chain_model(T.config(True), T.weights(True))
    name, shape = fresh._spec[0]
    z = np.zeros(shape, np.float32)
    assert fresh._lib.uu3d_set_weight(fresh._h, name.encode(), _p(z), z.size) == OK
    _untouched(_launch("proj_mlp_qkv", *a, model=fresh, expect=NOT_READY))
    assert fresh._lib.uu3d_op_tchain_launches(fresh._h, None, 0) == 0
