"""Compile-time guards on spatial_stack_p16_kernel (csrc/uu3d_spatial_p16.h), the shape the library launches (spatial_stage in
uu3d_forward.inc: 7 frames on 8 waves of one 16-token panel): no scratch, packed f32 without op_sel, the register budget of four waves per SIMD,
the 16x16x32 MFMA form, and LDS stores only for K / V, the parameter table and the spare key slots."""
import os
import re
import subprocess
import tempfile

import pytest

from tests import util

CSRC = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
SRC = r'''
#include "uu3d_spatial_p16.h"
using namespace uu3d;
template __global__ void uu3d::spatial_stack_p16_kernel<17, 7, 1>(const float*, const SpatialParams, const _Float16*, float*, _Float16*, _Float16*);
'''


@pytest.fixture(scope="module")
def kernel():
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
        asm = open(out).read()
    m = re.search(r"^(_ZN4uu3d24spatial_stack_p16_kernel\w+):(.*?)^\.Lfunc_end", asm, re.S | re.M)
    assert m, "kernel not found"
    ins = [l.strip() for l in m.group(2).split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    return ins, asm, m.group(1)


def _meta(asm, name, key):
    """A metadata key of the kernel (the keys after .name in its amdhsa.kernels entry, alphabetical order)."""
    tail = re.search(r"\.name:\s+" + name + r"\n(.*?)(?:\n\s+-\s+\.|\n\.\.\.)", asm, re.S).group(1)
    return int(re.search(r"\." + key + r":\s+(\d+)", tail).group(1))


def test_no_scratch_and_register_budget(kernel):
    ins, asm, name = kernel
    assert not any("scratch_" in i or "buffer_store" in i for i in ins)
    assert _meta(asm, name, "private_segment_fixed_size") == 0
    assert _meta(asm, name, "vgpr_count") <= 128          # four waves per SIMD


def test_packed_f32_without_op_sel(kernel):
    ins, _, _ = kernel
    pk = [i for i in ins if re.match(r"v_pk_(fma|mul|add)_f32", i)]
    assert len(pk) > 300
    assert not [i for i in pk if "op_sel" in i]


def test_products_on_16x16x32(kernel):
    ins, _, _ = kernel
    mf = [i.split()[0] for i in ins if i.startswith("v_mfma")]
    assert set(mf) == {"v_mfma_f32_16x16x32_f16"} and len(mf) == 48        # per block: 6 + 6 + 6 + 6 + 12 + 12
    assert any(i.startswith("v_permlane16_swap") for i in ins) and any(i.startswith("v_permlane32_swap") for i in ins)


def test_lds_stores_are_kv_parameters_and_spare_keys_only(kernel):
    """K and V are single-float stores (8 per lane and matrix); the one-time parameter copy and spare-key zeroing are the only
    other LDS writes: no activation operand tile (the h3 kernel's ds_write_b64 planes)."""
    ins, _, _ = kernel
    ds_w = [i for i in ins if i.startswith("ds_write")]
    assert not [i for i in ds_w if not re.match(r"ds_write(2st64)?_b32|ds_write2_b32", i)], ds_w
    assert len(ds_w) <= 24, len(ds_w)
    assert not [i for i in ins if i.startswith("ds_read") and "_b64" in i and "b128" not in i and "ds_read2" not in i]
