"""Multi-rank custom-loss training without a GPU: the accumulating tape backward is declared, exported and bound, refuses null
handles and buffers, Trainer.no_sync exists, and the gfx950 code of its kernel (scale_accumulate_kernel, cross-compiled like
tests/test_long_attention_isa_cpu.py) moves 16 bytes per access and rounds the multiply and the add separately (no fma)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from tests import util

CSRC = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
NEW_SYMBOLS = ("uu3d_train_backward_tape_accumulate", "uu3d_train_copy_nonfinite")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    return _capi.load_library()


def test_accumulate_symbol_declared_exported_and_bound(lib):
    from uplift_upsample_3dhpe_amd import _capi
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _capi.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
    assert len(lib.uu3d_train_backward_tape_accumulate.argtypes) == 9 and lib.uu3d_train_backward_tape_accumulate.restype is C.c_int
    assert lib.uu3d_train_backward_tape_accumulate.argtypes[7] is C.c_int32
    assert len(lib.uu3d_train_copy_nonfinite.argtypes) == 3 and lib.uu3d_train_copy_nonfinite.restype is C.c_int


def test_accumulate_refuses_null_handles_and_buffers(lib):
    from uplift_upsample_3dhpe_amd import _capi
    buf = C.c_void_p(0x1000)                    # never dereferenced: every call below is refused before anything is enqueued
    assert lib.uu3d_train_backward_tape_accumulate(None, None, None, None, buf, buf, None, 1, None) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_train_backward_tape_accumulate(None, buf, None, None, buf, buf, None, 1, None) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_train_copy_nonfinite(None, buf, None) == _capi.UU3D_ERR_INVALID_ARGUMENT


def test_trainer_has_no_sync():
    from uplift_upsample_3dhpe_amd.trainer import Trainer
    assert callable(getattr(Trainer, "no_sync", None))
    assert callable(getattr(Trainer, "_accumulate_backward", None))


SRC = r'''
#include "uu3d_bwd.h"
#include "uu3d_train_kernels.h"
void uu3d_isa_probe(float* a, const float* g, long long n, const float* s, unsigned* f) {
    hipLaunchKernelGGL(uu3d::scale_accumulate_kernel, dim3(1), dim3(256), 0, 0, a, g, n, s, f);
}
'''


@pytest.fixture(scope="module")
def kernel_asm():
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
    m = re.search(r"^(_ZN4uu3d\w*scale_accumulate_kernel\w*):.*?s_endpgm", asm, re.S | re.M)
    assert m, "scale_accumulate_kernel not in the gfx950 code"
    return m.group(0)


def test_accumulate_kernel_uses_16_byte_accesses(kernel_asm):
    assert "global_load_dwordx4" in kernel_asm and "global_store_dwordx4" in kernel_asm
    assert "scratch_" not in kernel_asm


def test_accumulate_kernel_rounds_multiply_and_add_separately(kernel_asm):
    assert not re.search(r"\bv_(pk_)?fmac?_f32", kernel_asm), "the unscale and the add must not contract into an fma"
    assert "v_mul_f32" in kernel_asm and "v_add_f32" in kernel_asm


def test_accumulate_kernel_has_no_float_atomics(kernel_asm):
    atomics = re.findall(r"\b(global_atomic_\w+)", kernel_asm)
    assert atomics and set(atomics) == {"global_atomic_or"}        # the non-finite word only
