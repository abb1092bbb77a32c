"""Autograd entry points without a GPU: the library exports the tape symbols, include/uu3d.h declares them, _capi binds them, and
the Python surface (model.parameters() / named_parameters() / requires_grad_() / parameters_changed(), Trainer.zero_grad()) exists."""
import ctypes as C
import os
import re

import pytest

from tests import util

TAPE_SYMBOLS = ("uu3d_train_forward_tape", "uu3d_train_backward_tape", "uu3d_tape_destroy")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    return _capi.load_library()


def test_tape_symbols_exported_declared_and_bound(lib):
    from uplift_upsample_3dhpe_amd import _capi
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    assert "typedef struct uu3d_tape uu3d_tape;" in header
    for s in TAPE_SYMBOLS + ("uu3d_train_clear_nonfinite",):
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _capi.EXPORTED_SYMBOLS, s
        assert hasattr(lib, s), s
    assert len(lib.uu3d_train_forward_tape.argtypes) == 15 and lib.uu3d_train_forward_tape.restype is C.c_int
    assert len(lib.uu3d_train_backward_tape.argtypes) == 7 and lib.uu3d_train_backward_tape.restype is C.c_int
    assert lib.uu3d_tape_destroy.argtypes == [C.c_void_p] and lib.uu3d_tape_destroy.restype is None


def test_tape_calls_refuse_null_handles(lib):
    tape = C.c_void_p()
    assert lib.uu3d_train_forward_tape(None, None, None, None, 1, None, None, None, 0.0, None, None, None, 0, C.byref(tape), None) != 0
    assert not tape.value
    assert lib.uu3d_train_backward_tape(None, None, None, None, None, None, None) != 0
    lib.uu3d_tape_destroy(None)                       # a no-op


def test_python_surface():
    from uplift_upsample_3dhpe_amd.net.uplift_upsample_transformer import UpliftUpsampleTransformer
    from uplift_upsample_3dhpe_amd.trainer import Trainer
    for name in ("parameters", "named_parameters", "requires_grad_", "parameters_changed"):
        assert callable(getattr(UpliftUpsampleTransformer, name)), name
    assert callable(Trainer.zero_grad)
