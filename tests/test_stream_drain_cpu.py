"""CPU: the end of a live track (include/uu3d.h, LIVE TRACKS: END OF A TRACK; stream.StreamSession.finish) -- the host mirror of the drain
window (stream.window_plan(drained=k)) against a plain restatement, the drain steps of the two numpy state machines (stream.LiveRootHost,
stream.LiveOneEuroHost), the refusals that need no device, the C ABI."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import util
from tests.test_stream_root_cpu import CAMERA, J, bits, synthetic


def _strides(cfg, ms):
    from uplift_upsample_3dhpe_amd import stream
    return stream.session_strides(cfg, ms)


@pytest.mark.parametrize("cfgname,ms", [("h36m_81", 2), ("h36m_81", 4), ("h36m_351", 5), ("h36m_351", 10)])
def test_drain_window_plan_against_a_plain_restatement(cfgname, ms):
    """The k-th drain tick of a track that ended at L frames in a session of lookahead a: the window a session of lookahead a - k writes at
    its L-th push (same centre, masks, sources and kinds), at the ring places of the draining session's own capacity; every ring source is
    a keyframe the ring still holds at L frames, the edge source is the last edge frame filed."""
    from uplift_upsample_3dhpe_amd import stream
    cfg = util.load_config(cfgname)
    S, s_in, pred = _strides(cfg, ms)
    a_max = stream.max_lookahead(cfg)
    rng = np.random.default_rng(ms)
    fresh_rows = 0
    for a in (1, 7, a_max):
        cap = stream.ring_capacity(cfg, ms, a)
        assert cap == (a + a_max) // s_in + 1
        for L in (1, 5, 60, 3 * cap * s_in + 1):
            newest_key = (L - 1) // s_in * s_in
            oldest_kept = max(0, newest_key - (cap - 1) * s_in)          # the ring keeps the newest `cap` multiples of s_in
            flags = rng.uniform(size=L) < 0.7
            for valid in (None, flags):
                for k in range(1, a + 1):
                    c = L - 1 - a + k
                    got = stream.window_plan(L, a, cfg, ms, valid, drained=k)
                    want = stream.window_plan(L, a - k, cfg, ms, valid)
                    assert stream.emits(L, a, cfg, ms, drained=k) == (c >= 0 and c % pred == 0) == stream.emits(L, a - k, cfg, ms)
                    if not (c >= 0 and c % pred == 0):                     # (L <= a: the first drain ticks centre on frames < 0)
                        assert got is None and want is None
                        continue
                    fresh_rows += 1
                    assert got["centre"] == want["centre"] == c
                    for name in ("mask", "src", "kind"):
                        assert np.array_equal(got[name], want[name]), (L, a, k, name)
                    ring, edge = got["kind"] == 2, got["kind"] == 3
                    assert np.array_equal(got["place"][ring], (got["src"][ring] // s_in) % cap) and (got["place"][~ring] == -1).all()
                    assert (got["src"][ring] % s_in == 0).all() and (got["src"][ring] >= oldest_kept).all() and (got["src"][ring] < L).all()
                    assert (got["src"][edge] == (L - 1) // S * S).all()
                    if valid is not None:                                  # a real token never reads a missing frame
                        read = got["kind"] >= 2
                        assert flags[got["src"][read]].all()
    assert fresh_rows > 100


def test_drained_zero_is_todays_window_plan():
    from uplift_upsample_3dhpe_amd import stream
    cfg = util.load_config("h36m_81")
    for L in (1, 5, 41, 60, 200):
        for a in (0, 7, 40):
            p, q = stream.window_plan(L, a, cfg, 4), stream.window_plan(L, a, cfg, 4, None, 0)
            assert stream.emits(L, a, cfg, 4) == stream.emits(L, a, cfg, 4, 0) == (p is not None) == (q is not None)
            if p is not None:
                assert p.keys() == q.keys() and all(np.array_equal(p[k], q[k]) for k in p)
    for bad in (-1, 8):
        with pytest.raises(ValueError, match="drained must be in"):
            stream.window_plan(60, 7, cfg, 4, drained=bad)


@pytest.mark.parametrize("lookahead", [1, 5])
def test_root_mirror_drain_step(lookahead):
    """LiveRootHost.drain: the k-th drain tick solves frame n - 1 - lookahead + k from the ring -- solve_roots_host on that frame --, files
    nothing, holds by step's rule; a tick that is not fresh, a tick beyond the lookahead and a slot without frames change nothing."""
    from uplift_upsample_3dhpe_amd import predict, stream
    n, m = 20, 6
    P, uv, _ = synthetic(n, seed=3)
    uv = uv.copy()
    flags = np.ones((n, J), bool)
    if lookahead >= 3:
        flags[n - 2, 3:] = False                                      # too few used joints in the tail: held
    want, solved = predict.solve_roots_host(P, uv, CAMERA, flags=flags, min_root_joints=m)
    host = stream.LiveRootHost(J, lookahead, CAMERA, m)
    assert host.drain(P[0])[1] == 0 and host.drained == 0               # no frames: nothing to drain
    for t in range(n):
        c = t - lookahead
        root, state = host.step(uv[t], flags[t], P[c] if c >= 0 else None)
    ring = (host.raw.copy(), host.used.copy())
    last = want[n - 1 - lookahead].astype(np.float32)
    assert state == 1 and np.array_equal(bits(root), bits(last))
    for k in range(1, lookahead + 1):
        c = n - 1 - lookahead + k
        if k == 2:                                                    # a drain tick that is not fresh returns the previous root
            root, state = host.drain(None)
            assert host.drained == 2 and np.array_equal(bits(root), bits(last))
            continue
        root, state = host.drain(P[c])
        if solved[c]:
            last = want[c].astype(np.float32)
            assert state == 1 and np.array_equal(bits(root), bits(last)), c
        else:
            assert state == 2 and np.array_equal(bits(root), bits(last)), c
    assert lookahead < 3 or not solved[n - 2]
    assert host.frames == n and host.drained == lookahead
    assert np.array_equal(host.raw, ring[0]) and np.array_equal(host.used, ring[1])
    before = (root.copy(), state)
    root, state = host.drain(P[0])                                    # beyond the lookahead: nothing changes
    assert host.drained == lookahead and state == before[1] and np.array_equal(bits(root), bits(before[0]))
    host.reset()
    assert host.frames == 0 and host.drained == 0


@pytest.mark.parametrize("lookahead,pred", [(3, 1), (7, 5)])
def test_filter_mirror_drain_step(lookahead, pred):
    """LiveOneEuroHost.drain: one sample at the virtual counter -- the pushes and then the drain ticks give one_euro_host over the fresh
    frames of the WHOLE track; a slot that is not chosen keeps its state."""
    from uplift_upsample_3dhpe_amd import predict, stream
    n, slots, ch, rate = 31, 2, 6, 50
    filt = predict.OneEuro(1.5, 0.3, 1.0)
    rng = np.random.default_rng(9)
    x = np.cumsum(rng.normal(size=(n, slots, ch)), axis=0).astype(np.float32)
    host = stream.LiveOneEuroHost(slots, ch, rate, filt, lookahead)
    got = {}
    for t in range(n):
        c = t - lookahead
        f = c >= 0 and c % pred == 0
        out = host.step(x[max(c, 0)], [t + 1] * slots, [f] * slots)
        if f:
            got[c] = out.copy()
    state = [a.copy() for a in (host.xh, host.dxh, host.last, host.taken)]
    for k in range(1, lookahead + 1):
        c = n - 1 - lookahead + k
        f = c % pred == 0
        out = host.drain(x[c], [n, n], [k, k], [f, f], chosen=[True, False])
        if f:
            got[c] = out.copy()
        for a, b in zip((host.xh, host.dxh, host.last, host.taken), state):       # slot 1 is not chosen: untouched, returns its xh
            assert np.array_equal(a[1], b[1])
        assert np.array_equal(bits(out[1]), bits(state[0][1].astype(np.float32)))
    centres = list(range(0, n, pred))
    assert sorted(got) == centres
    want = predict.one_euro_host(x[centres, 0], None, rate / pred, filt)
    assert np.array_equal(bits(np.stack([got[c][0] for c in centres])), bits(want))


def _stub_model():
    return types.SimpleNamespace(arch=types.SimpleNamespace(compiled_dims=True), device="cpu", has_strided_input=True)


def test_refusals_need_no_device():
    from uplift_upsample_3dhpe_amd import stream
    cfg = util.load_config("h36m_81")
    for rates in ({"fps": 25}, {"fps": 10, "out_fps": 50}):
        s = object.__new__(stream.StreamSession)
        s._init_plan(_stub_model(), cfg, 3, (1920, 1080), 4, True, 40, True, False, rates["fps"], 50, rates.get("out_fps"))
        with pytest.raises(ValueError, match="finish in a session with fps / out_fps is not supported yet.*later change"):
            s.finish()
        with pytest.raises(ValueError, match="drain=True together with fps / out_fps.*later change"):
            stream.replay_tracks(_stub_model(), cfg, [np.zeros((5, 17, 2), np.float32)], lookahead=40, drain=True, **rates)
    with pytest.raises(SystemExit):
        stream.parse_args(["--config", "c", "--weights", "w", "--input", "i", "--output", "o", "--drain", "--fps", "25"])
    args = stream.parse_args(["--config", "c", "--weights", "w", "--input", "i", "--output", "o", "--drain", "--lookahead", "7"])
    assert args.drain is True and args.lookahead == 7
    assert stream.parse_args(["--config", "c", "--weights", "w", "--input", "i", "--output", "o"]).drain is False


def test_c_abi_declared_and_refusing():
    import __graft_entry__ as ge
    ge.build()
    import re
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(util.ROOT + "/include/uu3d.h").read()
    assert "LIVE TRACKS: END OF A TRACK" in header
    for s in ("uu3d_stream_drain_bytes", "uu3d_stream_drain_layout", "uu3d_stream_drain_commit", "uu3d_stream_root_drain",
              "uu3d_stream_drain_file", "uu3d_stream_drain_reset"):
        assert re.search(r"\b" + s + r"\s*\(", header) and s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    fields = re.search(r"typedef struct uu3d_stream_drain_state_layout \{ int64_t ([^;]*);", header).group(1)
    assert [f for f, _ in _capi.Uu3dStreamDrainLayout._fields_] == fields.replace(" ", "").split(",")
    BAD = _capi.UU3D_ERR_INVALID_ARGUMENT
    lay = _capi.Uu3dStreamDrainLayout()
    assert lib.uu3d_stream_drain_bytes(0) == 0 and lib.uu3d_stream_drain_bytes((1 << 20) + 1) == 0
    assert lib.uu3d_stream_drain_layout(5, C.byref(lay)) == 0 and lay.bytes == lib.uu3d_stream_drain_bytes(5) and lay.bytes % 256 == 0
    assert 0 <= lay.drained_offset and lay.drained_offset + 20 <= lay.virtual_frames_offset and lay.virtual_frames_offset + 20 <= lay.ticked_offset
    assert lay.ticked_offset + 5 <= lay.bytes and lay.virtual_frames_offset % 256 == 0 and lay.ticked_offset % 256 == 0
    assert lib.uu3d_stream_drain_layout(0, C.byref(lay)) == BAD and lib.uu3d_stream_drain_layout(5, None) == BAD
    cfg = _capi.Uu3dStreamConfig(3, 2, 4, 2, 7, 1, 1, 0)
    block = C.c_void_p(256 * 4096)                                    # an aligned address that is never dereferenced: the calls refuse first
    assert lib.uu3d_stream_drain_commit(None, C.byref(cfg), *[None] * 8) == BAD
    assert lib.uu3d_stream_drain_reset(3, None, None, None) == BAD and lib.uu3d_stream_drain_reset(0, block, None, None) == BAD
    assert lib.uu3d_stream_drain_reset(3, C.c_void_p(256 * 4096 + 8), None, None) == BAD
    assert lib.uu3d_stream_root_drain(3, 65, 7, block, block, *[None] * 4, 6, None, None, None) == _capi.UU3D_ERR_UNSUPPORTED
    assert lib.uu3d_stream_root_drain(3, 17, 7, block, None, *[None] * 4, 6, None, None, None) == BAD
    assert lib.uu3d_stream_root_drain(3, 17, 7, block, block, *[None] * 4, 6, None, None, None) == BAD
    ptrs, widths = (C.c_void_p * 1)(256 * 4096), (C.c_int32 * 1)(51)
    assert lib.uu3d_stream_drain_file(3, 0, block, 1, ptrs, widths, ptrs, block, block, None, None, None) == BAD        # no rows
    assert lib.uu3d_stream_drain_file(3, 7, block, 5, ptrs, widths, ptrs, block, block, None, None, None) == BAD        # too many buffers
    assert lib.uu3d_stream_drain_file(3, 7, block, 1, ptrs, widths, ptrs, block, block, None, None, None) == BAD        # dst is src
    assert lib.uu3d_stream_drain_file(3, 7, block, 1, ptrs, widths, ptrs, block, block, block, None, None) == BAD       # half a root state pair


def test_drain_source_has_no_atomics_and_shares_the_window_and_the_solve():
    import os
    import re
    csrc = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "uu3d_stream_drain.h")).read())
    assert "atomic" not in code.lower()
    assert "stream_write_window(" in code and "stream_root_settle(" in code
    assert "window_frame(" not in code and "solve_root(" not in code     # the rules are the shared device code, not restated
    root_h = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "uu3d_stream_root.h")).read())
    assert root_h.count("solve_root(") == 1 and root_h.count("stream_root_settle(") == 2
