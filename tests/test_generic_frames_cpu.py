"""No GPU: the gates of the frames form for generic dims (StreamSession's constructor with stubs), the one-workgroup-per-frame spatial stack
(csrc/uu3d_spatial_generic.h) cross-compiled for gfx950 -- its code object's metadata only -- the host rule for its LDS, and the entry points
of the frames form in the symbol and argument tables."""
import ctypes as C
import os
import re
import subprocess
import tempfile
import types

import pytest

from tests import util

CSRC = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
INCLUDE = os.path.join(util.ROOT, "include")
NAME = "spatial_generic_kernel"
SRC = r'''
#include "uu3d_spatial_generic.h"
using namespace uu3d;
template __global__ void uu3d::spatial_generic_kernel<SG_ROWS>(const float*, const SpatialGenericParams, float*);
'''
# spatial_generic_lds_bytes / spatial_generic_head_group over (J, d_s, h_s, heads): one line per case
RULE_SRC = r'''
#include "uu3d_spatial_generic.h"
#include <cstdio>
int main() {
    using namespace uu3d;
    const int cases[][4] = {{17, 16, 32, 4}, {13, 24, 48, 3}, {15, 32, 64, 8}, {17, 32, 128, 8}, {17, 128, 128, 2}, {8, 32, 64, 16},
                            {25, 16, 32, 4}, {3, 16, 32, 4}, {32, 128, 512, 2}, {128, 128, 512, 2}, {64, 64, 256, 4}};
    for (const auto& c : cases)
        printf("%d %d %d %d %zu %d %zu\n", c[0], c[1], c[2], c[3], spatial_generic_lds_bytes(c[0], c[1], c[2], c[3]),
               spatial_generic_head_group(c[0], c[3]), SG_LDS_LIMIT);
    return 0;
}
'''


def _stub(has_form, strided=True, J=25):
    m = types.SimpleNamespace(arch=types.SimpleNamespace(compiled_dims=False, num_keypoints=J), device="cpu", has_strided_input=strided)
    if has_form is not None:
        m.has_frames_form = has_form
    return m


def test_stream_session_gate_follows_has_frames_form():
    from uplift_upsample_3dhpe_amd import stream
    cfg = util.load_config("h36m_81")
    for stub in (_stub(False), _stub(None)):                            # no form; no such attribute: the arch's compiled_dims decides
        with pytest.raises(NotImplementedError, match="generic dims"):
            stream.StreamSession(stub, cfg, slots=2, flip=False)
    # a generic model WITH the form passes the gate: the next refusals it meets need no device either
    with pytest.raises(ValueError, match=r"permutation of range\(25\)"):   # the config's 17-entry flip table on 25 joints
        stream.StreamSession(_stub(True), cfg, slots=2, flip=True)
    bad = cfg.copy()
    bad.AUGM_FLIP_KEYPOINT_ORDER = list(range(24)) + [0]                # 25 entries, not a permutation
    with pytest.raises(ValueError, match="permutation"):
        stream.StreamSession(_stub(True), bad, slots=2, flip=True)
    with pytest.raises(ValueError, match="missed_detections needs a model with strided input"):
        stream.StreamSession(_stub(True, strided=False), cfg, slots=2, flip=False, missed_detections=True)
    # a generic model with 17 joints is checked like any other: the shipped table passes, a table that is no permutation does not
    with pytest.raises(ValueError, match="missed_detections needs a model with strided input"):
        stream.StreamSession(_stub(True, strided=False, J=17), cfg, slots=2, flip=True, missed_detections=True)
    bad17 = cfg.copy()
    bad17.AUGM_FLIP_KEYPOINT_ORDER = [0] * 17
    with pytest.raises(ValueError, match=r"permutation of range\(17\)"):
        stream.StreamSession(_stub(True, J=17), bad17, slots=2, flip=True)
    ok = cfg.copy()
    ok.AUGM_FLIP_KEYPOINT_ORDER = [0] + [i + 1 if i % 2 else i - 1 for i in range(1, 25)]      # an involution of range(25)
    assert sorted(ok.AUGM_FLIP_KEYPOINT_ORDER) == list(range(25))
    with pytest.raises(ValueError, match="missed_detections needs a model with strided input"):
        stream.StreamSession(_stub(True, strided=False), ok, slots=2, flip=True, missed_detections=True)


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


def _meta(asm, key):
    m = re.search(r"\.amdhsa_kernel _ZN4uu3d\w*" + NAME + r"\w*\n(.*?)\.end_amdhsa_kernel", asm, re.S)
    assert m, f"{NAME} not in the gfx950 code"
    v = re.search(r"\.amdhsa_" + key + r"\s+(\d+)", m.group(1))
    assert v, key
    return int(v.group(1))


def test_the_kernel_compiles_for_gfx950_without_spills_and_with_dynamic_lds_only(asm):
    assert _meta(asm, "private_segment_fixed_size") == 0                 # no scratch: nothing spilled
    assert _meta(asm, "group_segment_fixed_size") == 0                   # no static LDS: the frame's buffers are the launch's dynamic LDS


@pytest.fixture(scope="module")
def rule():
    hipcc = _hipcc()
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "rule.hip"), os.path.join(d, "rule")
        open(src, "w").write(RULE_SRC)
        subprocess.run([hipcc, "-O0", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", CSRC, "-I", INCLUDE, "-o", exe, src],
                       check=True, stderr=subprocess.DEVNULL)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return {tuple(int(v) for v in line.split()[:4]): tuple(int(v) for v in line.split()[4:]) for line in out.splitlines()}


def test_the_lds_rule_is_the_one_the_header_states(rule):
    """bytes = 4 (2 J d_s + J (max(3 d_s, h_s) + 1) + hg J (J | 1)), hg = clamp(2048 // (J (J | 1)), 1, heads); the form exists up to 160 KiB."""
    assert len(rule) == 11
    for (J, ds, hs, H), (nbytes, hg, limit) in rule.items():
        want_hg = max(1, min(H, 2048 // (J * (J | 1))))
        assert hg == want_hg and limit == 160 * 1024
        assert nbytes == 4 * (2 * J * ds + J * (max(3 * ds, hs) + 1) + want_hg * J * (J | 1)), (J, ds, hs, H)
    fits = lambda k: rule[k][0] <= 160 * 1024
    # every row of CASES in tests/test_generic_dims_gpu.py, and the corner J = 32, d_s = 128, MLP ratio 4, have the form
    assert all(fits(k) for k in rule if k[0] <= 32)
    assert not fits((128, 128, 512, 2))                                   # J = 128, d_s = 128, ratio 4: refused
    assert fits((64, 64, 256, 4))


def test_frames_form_entry_points_are_in_the_tables():
    from uplift_upsample_3dhpe_amd import _capi
    header = open(os.path.join(INCLUDE, "uu3d.h")).read()
    for s in ("uu3d_frame_features_bytes", "uu3d_frame_features", "uu3d_forward_frames_ex", "uu3d_stream_state_layout"):
        assert s in _capi.EXPORTED_SYMBOLS and re.search(r"\b" + s + r"\s*\(", header), s
    import __graft_entry__ as ge
    ge.build()
    lib = _capi.load_library()
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    assert lib.uu3d_frame_features_bytes.restype is sz and list(lib.uu3d_frame_features_bytes.argtypes) == [vp, i32]
    assert list(lib.uu3d_frame_features.argtypes) == [vp, vp, i32, vp, vp, sz, i32, vp]
    assert list(lib.uu3d_forward_frames_ex.argtypes) == [vp, vp, i64, vp, vp, i32, vp, vp, C.POINTER(vp), vp, sz, i32, vp]
    # the header states the rule and no longer the restriction
    assert "compiled dims only" not in header and "spatial_generic" in header and "160 KiB" in header
    assert lib.uu3d_frame_features_bytes(None, 1) == 0                    # (no handle: no form, nothing dereferenced)
