"""The accumulating tape backward (uu3d_train_backward_tape_accumulate), one process, one rank: against uu3d_train_backward_tape
followed by torch's add, bit for bit; two passes add up; the reported ranges tile the buffer once and are final when reported;
a non-finite cotangent raises the non-finite word; and the same at 176 tokens, where the tiled attention pair runs."""
import ctypes as C

import numpy as np
import pytest

import uplift_upsample_3dhpe_amd as pkg
from tests import util

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _model(long_seq=False):
    cfg = util.load_config("h36m_351")
    if long_seq:
        cfg.SEQUENCE_LENGTH, cfg.STRIDES, cfg.PADDINGS = 176, [4, 4, 11], None
        cfg.SPATIAL_TRANSFORMER_BLOCKS, cfg.TEMPORAL_TRANSFORMER_BLOCKS = 1, 2
    cfg.BATCH_SIZE = 4
    cfg.DROP_PATH_RATE = [0.0, 0.0, 0.0]
    arch = pkg.arch_from_config(cfg)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=5, perturb=0.1))
    model.requires_grad_()
    return cfg, arch, model


def _tape(cfg, arch, model, B=2, seed=1):
    x, m = util.synthetic_batch(cfg, B, seed=seed)
    xm = x * m[:, :, None, None].astype(np.float32)
    full, central, tape = model._tape_forward(torch.from_numpy(xm).cuda(), model._mask_u8(torch.from_numpy(m).cuda()))
    return full, central, tape


def _cotangents(full, central, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.randn(full.shape, generator=g, device="cuda") * 1e-3, torch.randn(central.shape, generator=g, device="cuda") * 1e-2)


def _plain(model, tape, gF, gC):
    gp = torch.empty(int(model._lib.uu3d_num_params(model._h)), dtype=torch.float32, device="cuda")
    assert model._lib.uu3d_train_backward_tape(model._h, tape.handle, _p(gF), _p(gC), _p(gp), None, _stream()) == 0
    return gp


def _accumulate(model, tape, gF, gC, acc, report=0, scratch=None):
    if scratch is None:
        scratch = torch.empty_like(acc)
    st = model._lib.uu3d_train_backward_tape_accumulate(model._h, tape.handle, _p(gF), _p(gC), _p(scratch), _p(acc), None, report, _stream())
    assert st == 0, model._lib.uu3d_last_error(model._h).decode()


def _random(n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn(n, generator=g, device="cuda") * 1e-2


@pytest.mark.parametrize("long_seq", [False, True])
def test_accumulate_is_bitwise_plain_backward_plus_add(long_seq):
    """(a) accumulate into preloaded values == those values + what uu3d_train_backward_tape returns, bit for bit; (b) two passes ==
    the two plain gradients added in the same order; (e) long_seq: 176 tokens, the tiled attention pair."""
    cfg, arch, model = _model(long_seq)
    if long_seq:
        assert arch.num_frames == 176
    full, central, tape = _tape(cfg, arch, model)
    gF, gC = _cotangents(full, central, 3)
    gF2, gC2 = _cotangents(full, central, 4)
    n = int(model._lib.uu3d_num_params(model._h))
    pre = _random(n, 7)
    g1 = _plain(model, tape, gF, gC)
    g2 = _plain(model, tape, gF2, None)
    acc = pre.clone()
    _accumulate(model, tape, gF, gC, acc)
    torch.cuda.synchronize()
    assert torch.isfinite(g1).all() and g1.abs().max() > 0
    assert torch.equal(acc, pre + g1)
    _accumulate(model, tape, gF2, None, acc)
    torch.cuda.synchronize()
    assert torch.equal(acc, (pre + g1) + g2)
    # the plain entry still gives what it gave before the accumulating passes ran on the same tape
    assert torch.equal(_plain(model, tape, gF, gC), g1)


def test_reported_ranges_tile_the_buffer_and_are_final():
    """(c) with report_ranges the grad-ready callback sees ranges that tile [0, n) once; each range, copied on the stream the
    callback names, already holds its end value."""
    cfg, arch, model = _model()
    full, central, tape = _tape(cfg, arch, model, B=3)
    gF, gC = _cotangents(full, central, 5)
    n = int(model._lib.uu3d_num_params(model._h))
    acc = _random(n, 8)
    snap = torch.full_like(acc, float("nan"))
    seen = []

    def ready(user, first, count, stream):
        seen.append((int(first), int(count), stream))
        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=acc.device)):
            snap[first:first + count].copy_(acc[first:first + count])
    from uplift_upsample_3dhpe_amd import _capi
    cb = _capi.GRAD_READY_FN(ready)
    lib = model._lib
    assert lib.uu3d_train_set_grad_callback(model._h, cb, None) == 0
    try:
        _accumulate(model, tape, gF, gC, acc, report=1)
        torch.cuda.synchronize()
        assert len(seen) >= 4 and all(s is not None for _, _, s in seen)
        pos = 0
        for f, c, _ in sorted(seen):
            assert f == pos and c > 0
            pos = f + c
        assert pos == n
        assert torch.equal(snap, acc)
        # report_ranges = 0: no callback
        del seen[:]
        _accumulate(model, tape, gF, gC, acc, report=0)
        torch.cuda.synchronize()
        assert seen == []
    finally:
        lib.uu3d_train_set_grad_callback(model._h, _capi.GRAD_READY_FN(), None)


def test_nonfinite_cotangent_raises_the_word_and_null_buffers_are_refused():
    """(d) an Inf in the cotangent raises the model's non-finite word (uu3d_train_copy_nonfinite hands it to a device word of the
    caller); a null scratch or accumulator, or the two overlapping, is refused before anything runs, and the accumulator is left
    alone."""
    from uplift_upsample_3dhpe_amd import _capi
    cfg, arch, model = _model()
    lib = model._lib
    full, central, tape = _tape(cfg, arch, model)
    gF, gC = _cotangents(full, central, 6)
    n = int(lib.uu3d_num_params(model._h))
    acc = _random(n, 9)
    before = acc.clone()
    both = torch.empty(2 * n, device="cuda")
    for scratch, accum in ((None, acc), (acc, None), (acc, acc), (both[:n], both[n // 2:n // 2 + n]), (both[n - 1:], both[:n])):
        st = lib.uu3d_train_backward_tape_accumulate(model._h, tape.handle, _p(gF), _p(gC), _p(scratch), _p(accum), None, 1, _stream())
        assert st == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_train_backward_tape_accumulate(model._h, None, _p(gF), _p(gC), _p(acc), _p(acc), None, 1, _stream()) == \
        _capi.UU3D_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert torch.equal(acc, before)

    word = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    assert lib.uu3d_train_clear_nonfinite(model._h, _stream()) == 0
    _accumulate(model, tape, gF, gC, acc)
    assert lib.uu3d_train_copy_nonfinite(model._h, _p(word), _stream()) == 0
    torch.cuda.synchronize()
    assert int(word.item()) == 0
    gF[1, 3, 2, 0] = float("inf")
    _accumulate(model, tape, gF, gC, acc)
    assert lib.uu3d_train_copy_nonfinite(model._h, _p(word), _stream()) == 0
    torch.cuda.synchronize()
    assert int(word.item()) != 0
    out = C.c_int32()
    assert lib.uu3d_train_nonfinite(model._h, C.byref(out)) == 0 and out.value != 0
