"""Compile-time guards on the inference instantiation of the tiled exact-f32 attention (uu3d_attn_long.h, attn_long_fwd_kernel<48, false>:
the exact-f32 forward above 128 tokens), cross-compiled for gfx950 in the pattern of tests/test_long_attention_isa_cpu.py, and the host rule
that sends a launch to it (uu3d_launch.h, attn_choose), compiled host-only into a small program and run."""
import os
import re
import subprocess
import tempfile

import pytest

from tests import util

CSRC = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
INCLUDE = os.path.join(util.ROOT, "include")
NAME = "attn_long_fwd_kernel"
SRC = r'''
#include "uu3d_attn_long.h"
using namespace uu3d;
template __global__ void uu3d::attn_long_fwd_kernel<48, false>(const float*, int, int, int, int, const uint8_t*, float*, int, attn_long::NoStats);
'''
# attn_choose over (precision, L, planes_out, qfrag) at H = 8: one line per case
RULE_SRC = r'''
#include "uu3d_launch.h"
#include <cstdio>
int main() {
    using namespace uu3d;
    static_assert(ATTN_LONG_MAX_L == 416, "the lengths below");
    const int precs[2] = {UU3D_PREC_F16X3, UU3D_PREC_F32};
    for (int p = 0; p < 2; ++p)
        for (int L : {128, 129, 416, 417})
            for (int po = 0; po < 2; ++po)
                for (int qf = 0; qf < 2; ++qf) {
                    AttnRule r; r.precision = precs[p];
                    const int k = attn_choose(r, L, 8, po != 0, qf != 0);
                    printf("%s %d %d %d %d %s\n", p ? "f32" : "f16x3", L, po, qf, k, attn_class_name(k));
                }
    AttnRule forced; forced.precision = UU3D_PREC_F32; forced.forced = ATTN_F32_WG;
    printf("forced_wg 129 0 0 %d -\n", attn_choose(forced, 129, 8, false, false));
    return 0;
}
'''


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


def _device_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("uu3d_build", os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "build.py"))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    return b.DEVICE_FLAGS


@pytest.fixture(scope="module")
def asm():
    hipcc = _hipcc()
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "k.hip"), os.path.join(d, "k.s")
        open(src, "w").write(SRC)
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", *_device_flags(), "-I", CSRC, "-I", INCLUDE,
                        "-S", "--cuda-device-only", "-o", out, src], check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def _body(asm):
    m = re.search(r"^(_ZN4uu3d\w*" + NAME + r"\w*):.*?s_endpgm", asm, re.S | re.M)
    assert m, f"{NAME} not in the gfx950 code"
    return m.group(1), m.group(0)


def _meta(asm, key):
    m = re.search(r"\.amdhsa_kernel _ZN4uu3d\w*" + NAME + r"\w*\n(.*?)\.end_amdhsa_kernel", asm, re.S)
    assert m
    v = re.search(r"\.amdhsa_" + key + r"\s+(\d+)", m.group(1))
    assert v, key
    return int(v.group(1))


def test_the_inference_instantiation_exists_on_the_f32_matrix_pipe(asm):
    symbol, body = _body(asm)
    assert "ILi48ELb0EE" in symbol, symbol                     # <48, false>: the instantiation without statistics, not the training one
    assert "v_mfma_f32_16x16x4_f32" in body


def test_no_scratch_no_global_atomics(asm):
    _, body = _body(asm)
    assert "scratch_" not in body
    assert "global_atomic" not in body
    assert _meta(asm, "private_segment_fixed_size") == 0


def test_static_lds_within_64_kib(asm):
    lds = _meta(asm, "group_segment_fixed_size")
    assert 0 < lds <= 64 * 1024


@pytest.fixture(scope="module")
def rule():
    hipcc = _hipcc()
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "rule.hip"), os.path.join(d, "rule")
        open(src, "w").write(RULE_SRC)
        subprocess.run([hipcc, "-O0", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", CSRC, "-I", INCLUDE, "-o", exe, src],
                       check=True, stderr=subprocess.DEVNULL)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        p, L, po, qf, k, klass = line.split()
        table[(p, int(L), bool(int(po)), bool(int(qf)))] = (int(k), klass)
    return table


AUTO, F32_WG, HEAD_WAVE, H3, F32_LONG = range(5)


def test_attn_choose_takes_the_long_family_only_for_an_f32_call_above_128_tokens(rule):
    for L in (128, 129, 416, 417):
        for po in (False, True):
            for qf in (False, True):
                k, klass = rule[("f32", L, po, qf)]
                want_long = 128 < L <= 416 and not po and not qf
                assert (k == F32_LONG) == want_long, (L, po, qf, k)
                if want_long:
                    assert klass == "attn_f32"
    assert rule[("f32", 128, False, False)][0] == F32_WG       # up to 128 tokens: the register-resident kernel, as before
    assert rule[("f32", 417, False, False)][0] == AUTO         # beyond every kernel
    assert rule[("forced_wg", 129, False, False)][0] == AUTO   # a forced kernel is not overruled


def test_attn_choose_is_unchanged_at_precision_f16x3(rule):
    """What uu3d_op_attn_infer (UU3D_ATTN_AUTO) and every f16x3 forward answer: no exact-f32 kernel above 128 tokens."""
    for L in (128, 129, 416, 417):
        for po in (False, True):
            for qf in (False, True):
                k, _ = rule[("f16x3", L, po, qf)]
                if L > 416:
                    want = AUTO
                elif po or qf:
                    want = H3
                else:
                    want = F32_WG if L <= 128 else AUTO
                assert k == want, (L, po, qf, k)
