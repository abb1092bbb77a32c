"""The C-ABI library builds, loads and exports every symbol include/uu3d.h declares.
No compute is attempted without a GPU: uu3d_create must refuse cleanly."""
import ctypes as C
import os
import re

import pytest

from tests import util


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    return _capi.load_library()


def test_header_symbols_exported(lib):
    from uplift_upsample_3dhpe_amd import _capi
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    declared = set(re.findall(r"\b(uu3d_[a-z_0-9]+)\s*\(", header))
    declared -= {"uu3d_status", "uu3d_precision"}
    assert declared == set(_capi.EXPORTED_SYMBOLS)
    ops_header = open(os.path.join(util.ROOT, "include", "uu3d_ops.h")).read()
    ops = set(re.findall(r"\b(uu3d_op_[a-z_0-9]+)\s*\(", ops_header))
    assert ops == set(_capi.OPS_SYMBOLS)
    for s in declared | ops:
        assert hasattr(lib, s), s
    assert lib.uu3d_version().decode().startswith("uu3d ")
    assert lib.uu3d_status_string(0) == b"ok" and lib.uu3d_status_string(2) != b"ok"


def test_config_struct_matches_header():
    from uplift_upsample_3dhpe_amd import _capi
    # 9 scalars + 3 arrays of 8 + 6 scalars, all int32
    assert C.sizeof(_capi.Uu3dConfig) == 4 * (9 + 3 * 8 + 8)          # 9 scalars + 3 arrays of 8 + 8 scalars (output_bn and learnable_masked_token since round 3), all int32
    assert C.sizeof(_capi.Uu3dProfileEntry) == 48 + 32 + 4 + 4 + 8 + 8


def test_create_rejects_bad_arguments_without_compute(lib):
    import torch
    from uplift_upsample_3dhpe_amd import _capi
    h = C.c_void_p()
    assert lib.uu3d_create(None, 0, C.byref(h)) == _capi.UU3D_ERR_INVALID_ARGUMENT
    cfg = _capi.Uu3dConfig()
    assert lib.uu3d_create(C.byref(cfg), 0, C.byref(h)) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert b"num_frames" in lib.uu3d_last_error(None)
    if not torch.cuda.is_available():
        import uplift_upsample_3dhpe_amd as pkg
        with pytest.raises(_capi.Uu3dLibraryError):           # product path fails loudly, no CPU fallback
            pkg.build_uplift_upsample_transformer(util.load_config("h36m_81"))
    assert lib.uu3d_workspace_bytes(None, 4) == 0
    assert lib.uu3d_num_weights(None) == 0
    assert lib.uu3d_mpjpe(None, None, 1, 17, 6, None, None) == _capi.UU3D_ERR_INVALID_ARGUMENT


def test_training_gemm_operators_refuse_null_arguments_without_compute(lib):
    """The operator entries of the training step's GEMM forms (include/uu3d_ops.h): the ctypes argument records have the size of the
    fields the header lists (a hand count, not read from the header), and NULL records, NULL buffers and unknown kinds are refused before
    any launch."""
    from uplift_upsample_3dhpe_amd import _capi
    INVALID = _capi.UU3D_ERR_INVALID_ARGUMENT
    assert C.sizeof(_capi.Uu3dTrainDenseArgs) == 12 * 8 + 8 + 8 + 16 * 4 + 4 + 3 * 4 and C.sizeof(_capi.Uu3dTrainWgradArgs) == 9 * 8 + 8 + 14 * 4
    assert lib.uu3d_op_train_operand_bytes(1, 51, 40, 0) == 8 * 128 * 64 and lib.uu3d_op_train_operand_bytes(4, 51, 40, 0) == 8 * 64 * 64
    assert lib.uu3d_op_train_operand_bytes(5, 72, 40, 24) == 8 * 128 * 128
    assert lib.uu3d_op_train_operand_bytes(5, 72, 40, 25) == 0 and lib.uu3d_op_train_operand_bytes(2, 51, 40, 0) == 0 and lib.uu3d_op_train_operand_bytes(1, 0, 40, 0) == 0
    assert lib.uu3d_op_train_pack(None, 1, 51, 40, 0, None, None) == INVALID
    assert lib.uu3d_op_train_dense(None, None) == INVALID and lib.uu3d_op_train_wgrad(None, None) == INVALID
    assert lib.uu3d_op_train_dense(C.byref(_capi.Uu3dTrainDenseArgs()), None) == INVALID
    assert lib.uu3d_op_train_wgrad(C.byref(_capi.Uu3dTrainWgradArgs()), None) == INVALID
    assert lib.uu3d_op_colsum3(None, 96, 8, 32, None, None, None, 0, None, 0, None) == INVALID
    assert lib.uu3d_op_ln_bwd_ex(None, None, None, None, 32, 32, 8, None, None, None, 1.0, 1, None, None, None, None, 0, None) == INVALID
    assert lib.uu3d_op_identity_bwd(None, 1, 9, 3, 3, 1, 32, None, None) == INVALID
    assert lib.uu3d_op_scale_rows(None, 8, 32, None, 1.0, 1, None, 0, None, None) == INVALID


def test_missing_library_fails_loudly(tmp_path):
    from uplift_upsample_3dhpe_amd import _capi
    with pytest.raises(_capi.Uu3dLibraryError):
        _capi.load_library(str(tmp_path / "nope.so"))


def test_product_library_has_no_timing_hooks_and_the_bench_refuses_them(lib, monkeypatch):
    """Round 6: UU3D_SKIP / UU3D_TIMING_PARTS (launches left out, results wrong) exist only in a -DUU3D_TIMING_BUILD library whose version
    string says so; the product library does not even contain the variable names, and bench.py refuses to produce a line under them."""
    import bench
    from uplift_upsample_3dhpe_amd import _capi
    assert "timing" not in lib.uu3d_version().decode()
    blob = open(_capi.LIB_PATH, "rb").read()
    assert b"UU3D_SKIP" not in blob and b"UU3D_TIMING_PARTS" not in blob
    monkeypatch.setenv("UU3D_TCHAIN", "0")
    assert bench.env_switches() == {"UU3D_TCHAIN": "0"}                      # A/B switches are recorded ...
    monkeypatch.setenv("UU3D_SKIP", "128")
    with pytest.raises(SystemExit):                                            # ... result-changing ones refused
        bench.env_switches()
    assert "UU3D_SKIP" in bench.env_switches(timing_experiment=True)           # (tools/marginal_r06.sh: the line is labelled INVALID)


def test_build_is_keyed_by_content_not_by_file_times(tmp_path):
    """build.py rebuilds unless the fingerprint next to the library matches the sources (sha256 over sources, headers, flags, hipcc version)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("uu3d_build_t", os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "build.py"))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    assert not b._stale(b.LIB)                                                 # (the fixture built it)
    assert b._fingerprint() != b._fingerprint(("-DUU3D_TIMING_BUILD",))
    stamp = b.LIB + ".sha256"
    good = open(stamp).read()
    try:
        open(stamp, "w").write("0" * 64 + "\n")
        assert b._stale(b.LIB)                                                 # a binary of other sources passes for stale whatever its mtime
    finally:
        open(stamp, "w").write(good)


def test_every_included_piece_of_the_api_unit_is_fingerprinted():
    """uu3d_api.hip is one translation unit made of .inc pieces: each `#include "uu3d_*.inc"` names a file that exists, is included
    once, and is in build.HEADERS -- so an edit to any piece rebuilds the library."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("uu3d_build_i", os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "build.py"))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    pieces = re.findall(r'^#include "(uu3d_\w+\.inc)"', open(os.path.join(b.CSRC, "uu3d_api.hip")).read(), re.M)
    assert len(pieces) >= 6 and len(pieces) == len(set(pieces))
    for f in pieces:
        assert os.path.isfile(os.path.join(b.CSRC, f)), f
        assert f in b.HEADERS, f
    assert set(pieces) == {f for f in os.listdir(b.CSRC) if f.endswith(".inc")}       # and no piece is left lying around unincluded


def test_environment_switches_live_in_one_table():
    """Every UU3D_* variable the library reads is read by one of the two reader functions of csrc/uu3d_switches.h (read_switches: per
    handle, process_switches: per process), nowhere else, and INTEGRATION.md section 5 lists exactly those names."""
    import glob
    import re
    csrc = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
    sources = [f for f in glob.glob(os.path.join(csrc, "*")) if f.endswith((".hip", ".h", ".inc"))]
    sources += glob.glob(os.path.join(util.ROOT, "include", "*.h"))
    assert len(sources) > 20
    for f in sources:
        if os.path.basename(f) != "uu3d_switches.h":
            assert "getenv(" not in open(f).read(), f

    def body(text, signature):                      # the brace-balanced body behind a function's signature
        start = text.index("{", text.index(signature))
        depth = 0
        for i in range(start, len(text)):
            depth += {"{": 1, "}": -1}.get(text[i], 0)
            if depth == 0:
                return text[start:i + 1]
        raise AssertionError(signature)
    text = open(os.path.join(csrc, "uu3d_switches.h")).read()
    readers = body(text, "inline Switches read_switches()") + body(text, "inline const ProcessSwitches& process_switches()")
    assert text.count("getenv(") == readers.count("getenv(") > 0
    read = set(re.findall(r'"(UU3D_[A-Z0-9_]+)"', readers))
    assert len(read) >= 29 and {"UU3D_SKIP", "UU3D_TIMING_PARTS", "UU3D_TCHAIN", "UU3D_TRAIN_F32"} <= read
    doc = open(os.path.join(util.ROOT, "INTEGRATION.md")).read()
    table = doc[doc.index("<!-- switch-table -->"):doc.index("<!-- /switch-table -->")]
    listed = re.findall(r"^\| `(UU3D_[A-Z0-9_]+)", table, re.M)
    assert len(listed) == len(set(listed))
    assert set(listed) == read
    # the table is in the structs' order: the order in which the readers take the variables
    order = []
    for name in re.findall(r'"(UU3D_[A-Z0-9_]+)"', readers):
        if name not in order:
            order.append(name)
    assert listed == order
    # the timing hooks stay behind the timing build inside the per-process reader
    proc = body(text, "inline const ProcessSwitches& process_switches()")
    guarded = proc[proc.index("#ifdef UU3D_TIMING_BUILD"):proc.index("#endif")]
    assert "UU3D_SKIP" in guarded and "UU3D_TIMING_PARTS" in guarded
    assert "UU3D_SKIP" not in proc.replace(guarded, "") and "UU3D_TIMING_PARTS" not in proc.replace(guarded, "")
