"""The host plan arithmetic of csrc/uu3d_launch.h, restated for the operator tests (tests/test_bwd_ops_edges_gpu.py,
tests/test_train_gemm_ops_gpu.py, tests/test_train_gemm_ops_cpu.py).  Used ONLY to assert that a case reaches the branch it is named after."""
import os


def _cdiv(a, b):
    return (a + b - 1) // b


def _ru(v, m):
    return _cdiv(v, m) * m


def _plan_gemm_tn(R, P, Q, scratch, h3=False):
    """launch_gemm_tn (uu3d_launch.h: the h3 branch `if (h3 && P >= 128 && Q >= 128)`, then the f32 plan below it)."""
    KT, ldslab = _cdiv(R, 32), _ru(Q, 4)
    if h3 and P >= 128 and Q >= 128:
        tiles = _cdiv(P, 128) * _cdiv(Q, 128)
        tnh = int(os.environ.get("UU3D_TNH_WGS", "192"))
        slices = max(1, min(KT // 2, (tnh + tiles - 1) // tiles))
        wanted = slices
        while slices > 1 and slices * P * ldslab > scratch:
            slices -= 1
        kps = _cdiv(KT, slices)
        slices = _cdiv(KT, kps)
        return dict(kernel="tn_h3", KT=KT, tiles=tiles, wanted=wanted, slices=slices, kps=kps, combine=None if slices == 1 else "reduce")
    tiles = _cdiv(P, 64) * _cdiv(Q, 64)
    skinny = tiles <= 4 and KT >= 256
    slices = max(1, min(KT // 4, 256 // tiles)) if skinny else max(1, min(min(max(KT // 4, 1), 48), (1024 + tiles // 2) // tiles))
    wanted = slices
    while slices > 1 and slices * P * ldslab > scratch:
        slices -= 1
    kps = _cdiv(KT, slices)
    slices = _cdiv(KT, kps)
    return dict(kernel="tn_f32", KT=KT, tiles=tiles, wanted=wanted, slices=slices, kps=kps,
                combine=None if slices == 1 else ("reduce16" if skinny else "reduce"))


def _plan_gemm_nt(M, N, K, scratch):
    """splitk_rule as launch_gemm calls it (uu3d_launch.h: target 768, no full-chip exception)."""
    KT = _ru(K, 32) // 32
    tiles = _cdiv(M, 64) * _cdiv(N, 64)
    slices = 1
    if tiles < 384 and KT >= 8:
        slices = max(1, min(KT // 4, (768 + tiles // 2) // tiles))
    kps = _cdiv(KT, slices)
    slices = _cdiv(KT, kps)
    wanted = slices
    if slices > 1 and slices * M * _ru(N, 4) > scratch:
        slices, kps = 1, KT
    return dict(KT=KT, wanted=wanted, slices=slices, kps=kps)


def _plan_colsum(ldx, R, Cc, period, masked, scratch):
    """launch_colsum (uu3d_launch.h) and launch_reduce_partials (uu3d_bwd.h: 64 lanes per column from 128 slices)."""
    P = period if period > 0 else 1
    slices = max(1, min(256, R // max(128, P)))
    while slices > 1 and slices * P * Cc > scratch:
        slices -= 1
    if slices * P * Cc > scratch:
        return dict(kernel=None)
    extra = {}
    if period > 0 and not masked and Cc % 4 == 0 and ldx % 4 == 0 and R % period == 0:
        nb, xb = R // period, _cdiv(period * (Cc // 4), 256)
        slices = max(1, min(max(1, 512 // xb), nb // 4))
        while slices > 1 and slices * P * Cc > scratch:
            slices -= 1
        kernel = "period4"
    elif period <= 0 and not masked and Cc % 4 == 0 and ldx % 4 == 0:
        cgs = max(1, min(64, (Cc + 3) // 4))
        xb = _cdiv(Cc, 4 * cgs)
        slices = max(1, min(max(1, 320 // xb), R // 64))
        while slices > 1 and slices * Cc > scratch:
            slices -= 1
        kernel, extra = "colsum4", dict(cgs=cgs, xb=xb)
    else:
        kernel = "generic"
    return dict(kernel=kernel, slices=slices, combine=64 if slices >= 128 else 16, **extra)


def _plan_ln_bwd(D, ld, M, scratch):
    """launch_ln_bwd_rows (uu3d_launch.h)."""
    if 2 * D > scratch:
        return dict(kernel=None)
    if D in (32, 64) and ld % 4 == 0:
        RG = 1024 // D
        rows = first = max(4, _cdiv(M, RG * 512))
        wgs = _cdiv(M, RG * rows)
        while wgs > 1 and wgs * 2 * D > scratch:
            rows *= 2
            wgs = _cdiv(M, RG * rows)
        return dict(kernel="narrow<8>" if D == 32 else "narrow<16>", rows=rows, first=first, wgs=wgs)
    rows = first = max(2, _cdiv(M, 4 * 2048)) if D > 64 else max(8, _cdiv(M, 4 * 512))
    wgs = _cdiv(M, 4 * rows)
    while wgs > 1 and wgs * 2 * D > scratch:
        rows *= 2
        wgs = _cdiv(M, 4 * rows)
    return dict(kernel="wide<2>" if D <= 512 else "wide<4>", rows=rows, first=first, wgs=wgs)


def _plan_attn(backward, L, dh, masked, generic=False):
    """launch_attn_generic (uu3d_launch.h), head dims 4 and 48, no Dropout."""
    if dh == 4:
        pack = max(1, 128 // L)
        if not backward:
            return dict(kernel="generic_fwd<4>", pack=pack)
        return dict(kernel="small_bwd<17>" if (L == 17 and not masked and not generic) else "generic_bwd<4>", pack=pack)
    if not backward:
        return dict(kernel="generic_fwd<48>", pack=1)
    if L <= 128 and not generic:
        return dict(kernel="mfma<%d,48>" % _cdiv(L, 16), pack=1)
    return dict(kernel="generic_bwd<48>", pack=1)
