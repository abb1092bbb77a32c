"""Compile-time guards on the tiled exact-f32 attention of the training step beyond 128 tokens (uu3d_attn_long.h),
cross-compiled for gfx950 like tests/test_isa_cpu.py: the kernels exist, run on v_mfma_f32_16x16x4_f32, spill nothing,
add no float atomics (the backward is bitwise reproducible) and stay within 160 KiB of LDS."""
import os
import re
import subprocess
import tempfile

import pytest

from tests import util

CSRC = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
KERNELS = ("attn_long_fwd_kernel", "attn_long_dq_kernel", "attn_long_dkv_kernel")
SRC = r'''
#include "uu3d_attn_long.h"
using namespace uu3d;
template __global__ void uu3d::attn_long_fwd_kernel<48>(const float*, int, int, int, int, const uint8_t*, float*, int, float2*);
template __global__ void uu3d::attn_long_dq_kernel<48>(const float*, const float*, const float*, const float2*, int, int, int, int, const uint8_t*, float*, int);
template __global__ void uu3d::attn_long_dkv_kernel<48>(const float*, const float*, const float*, const float2*, int, int, int, int, const uint8_t*, float*, int);
'''


@pytest.fixture(scope="module")
def asm():
    import importlib.util
    spec = importlib.util.spec_from_file_location("uu3d_build", os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "build.py"))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "k.hip"), os.path.join(d, "k.s")
        open(src, "w").write(SRC)
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", *b.DEVICE_FLAGS, "-I", CSRC,
                        "-I", os.path.join(util.ROOT, "include"), "-S", "--cuda-device-only", "-o", out, src],
                       check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def _body(asm, name):
    m = re.search(r"^(_ZN4uu3d\w*" + name + r"\w*):.*?s_endpgm", asm, re.S | re.M)
    assert m, f"{name} not in the gfx950 code"
    return m.group(0)


def _meta(asm, name, key):
    """A field of the kernel descriptor (.amdhsa_kernel ... .end_amdhsa_kernel)."""
    m = re.search(r"\.amdhsa_kernel _ZN4uu3d\w*" + name + r"\w*\n(.*?)\.end_amdhsa_kernel", asm, re.S)
    assert m, name
    v = re.search(r"\.amdhsa_" + key + r"\s+(\d+)", m.group(1))
    assert v, (name, key)
    return int(v.group(1))


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_exists_on_the_f32_matrix_pipe(asm, name):
    body = _body(asm, name)
    assert "v_mfma_f32_16x16x4_f32" in body
    assert "v_pk_mul_f32" not in body and "v_pk_fma_f32" not in body and "v_pk_add_f32" not in body      # build.py DEVICE_FLAGS


@pytest.mark.parametrize("name", KERNELS)
def test_no_scratch_no_float_atomics(asm, name):
    body = _body(asm, name)
    assert "scratch_" not in body and "buffer_store" not in body
    assert "global_atomic_add_f32" not in body and "global_atomic" not in body
    assert _meta(asm, name, "private_segment_fixed_size") == 0


@pytest.mark.parametrize("name", KERNELS)
def test_lds_within_160_kib(asm, name):
    lds = _meta(asm, name, "group_segment_fixed_size")
    assert 0 < lds <= 160 * 1024
    assert lds <= 64 * 1024          # static LDS only: no hipFuncSetAttribute needed on any device
