"""CPU: the frames form of evaluation (include/uu3d.h, FRAMES FORM; eval.predict_windows(reuse_frames=True)).

* ``eval.window_frames`` -- which frames a set of windows reads, the set whose features are computed once -- against a brute-force,
  one token at a time restatement of the gather rules (common/dataset/uplifiting_dataset.py:322-394 as csrc/uu3d_misc.h states them).
* The new C entries are declared, bound and exported.
* Code shape of the two new gfx950 kernels: 16-byte row accesses, no scratch, no packed-fp32 ops.
"""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import util

NEW = ("uu3d_frame_features_bytes", "uu3d_frame_features", "uu3d_gather_window_frames", "uu3d_forward_frames_ex")


def _brute_force(desc, N, starts, lens, pad_edge, zero_masked):
    plain, flipped, zero = set(), set(), False
    for v, c, s, ms, sh, fl in np.asarray(desc, np.int64).tolist():
        ln = int(lens[v])
        for n in range(N):
            f = c - ((N - 1) * s) // 2 + n * s
            if 0 <= f < ln:
                src = f
            elif f < 0:                                            # first sampled frame >= 0
                src = f
                while src < 0:
                    src += s
            else:                                                  # last sampled frame < len
                src = f
                while src >= ln:
                    src -= s
            inside = 0 <= f < ln
            have = inside or (pad_edge and 0 <= src < ln)
            sm = ((n - N // 2) * s + sh) % ms == 0
            if zero_masked and not sm:
                continue                                           # the masked token: no frame read
            if not have:
                zero = True
                continue
            (flipped if fl else plain).add(int(starts[v]) + src)
    return np.array(sorted(plain), np.int64), np.array(sorted(flipped), np.int64), zero


@pytest.mark.parametrize("N,pad_edge,zero_masked", [(71, True, True), (71, False, True), (41, False, False), (9, True, False), (27, False, True)])
def test_window_frames_match_the_gather_rules(N, pad_edge, zero_masked):
    from uplift_upsample_3dhpe_amd.eval import window_frames
    rng = np.random.default_rng(N)
    lens = np.array([3, 40, 97, 260, 7, 351], np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    rows = []
    for _ in range(400):
        v = int(rng.integers(0, len(lens)))
        s = int(rng.choice([1, 2, 3, 5]))
        ms = s * int(rng.choice([1, 2, 4]))
        c = int(rng.integers(0, lens[v]))
        sh = int(rng.choice([c, -s, 0, 2 * s, -3 * s]))           # global alignment and random (also negative) shifts
        rows.append((v, c, s, ms, sh, int(rng.integers(0, 2))))
    desc = np.array(rows, np.int32)
    got = window_frames(desc, N, starts, lens, pad_edge, zero_masked)
    want = _brute_force(desc, N, starts, lens, pad_edge, zero_masked)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    # windows longer than their videos read every frame of the short ones with copy padding, and zero padding needs the zero frame
    if pad_edge:
        assert not got[2]


def test_new_entries_are_declared_and_exported():
    from uplift_upsample_3dhpe_amd import _capi
    hdr = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    for s in NEW:
        assert s in _capi.EXPORTED_SYMBOLS
        assert re.search(r"\b" + s + r"\(", hdr), s
    lib_path = _capi.LIB_PATH
    if not os.path.exists(lib_path):
        pytest.skip("libuu3d.so not built")
    lib = _capi.load_library()
    for s in NEW:
        assert hasattr(lib, s), s


SRC = r'''
#include "uu3d_misc.h"
using namespace uu3d;
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
        open(src, "w").write(SRC + "template <class T> void keep(T) {}\n"
                             "void uses() { keep(&gather_window_frames_kernel); keep(&frames_to_tokens_kernel); keep(&gather_windows_kernel); }\n")
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", *b.DEVICE_FLAGS, "-I", os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc"),
                        "-I", os.path.join(util.ROOT, "include"), "-S", "--cuda-device-only", "-o", out, src],
                       check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def _kernel(asm, name):
    m = re.search(r"^(_ZN4uu3d\w*" + name + r"\w*):.*?s_endpgm", asm, re.S | re.M)
    assert m is not None, name
    return m.group(0)


def test_frames_to_tokens_moves_16_byte_rows(asm):
    body = _kernel(asm, "frames_to_tokens_kernel")
    assert "scratch_" not in body
    assert "v_pk_" not in body                                     # packed-fp32 ops are off for device code (build.py DEVICE_FLAGS)
    assert body.count("global_store_dwordx4") == 1
    assert body.count("global_load_dwordx4") >= 2                  # PE + (token | feature row)
    assert not re.search(r"global_store_dword\s", body)             # no 4-byte row stores ...
    assert len(re.findall(r"global_load_dword\s", body)) <= 1      # ... and one 4-byte load: the token's table row


def test_gather_window_frames_code_shape(asm):
    body = _kernel(asm, "gather_window_frames_kernel")
    assert "scratch_" not in body and "v_pk_" not in body
    assert "global_store_dword " in body                           # one int32 row per token
