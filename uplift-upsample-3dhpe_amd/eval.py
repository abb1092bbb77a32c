"""End-to-end evaluation driver -- the reference's ``run_eval`` / ``run_eval_multi_mask_stride`` (eval.py:34-270) over the
device-resident pipeline of this package:

    .npz ingestion (h36m.py)  ->  videos resident in HBM (data.PoseTable)  ->  window descriptors with the reference's sample
    order and globally aligned stride masks (data.SequenceGenerator)  ->  uu3d_gather_windows builds the 2D windows on the
    device, already multiplied by their masks (eval.py:67)  ->  ONE forward per batch over [windows | flipped windows]
    (EVAL_FLIP: the reference calls the model twice, eval.py:152-180)  ->  un-flip + average  ->  (multi-GPU: batch shards per
    rank, one all-gather of the central predictions)  ->  keyframe interpolation and the ALL FRAMES / KEYFRAMES reports
    (evaluation.evaluate_predictions = eval.py:195-251, action_wise_eval.py).

What it does NOT compute: with ``TEST_STRIDED_EVAL`` and ``SEQUENCE_STRIDE`` > 1 the reference replaces the prediction of
every window whose centre is not a keyframe (frame index % stride != 0) by an interpolation between its neighbours
(action_wise_eval.py:77-100) -- for h36m_351 that is 4 of 5 windows, all of them ALL-MASKED inputs whose forward pass is
discarded.  ``run_eval`` only runs the windows whose prediction survives; the reported numbers are the
same (tests/test_eval_gpu.py checks them against the all-windows pipeline driven by the CPU oracle).
"""
import time

import numpy as np

from . import dist as udist
from . import evaluation, h36m
from .data import SequenceGenerator


def _log(*args):
    print(*args, flush=True)


def prediction_stride(config):
    """The keyframe stride of eval.py:195-251 (``evaluation.evaluate_predictions``): frames whose index is a multiple of it keep their own
    prediction, the others are interpolated.  None: no strided evaluation, every frame keeps its own."""
    if not (config.SEQUENCE_STRIDE > 1 and config.TEST_STRIDED_EVAL is True):
        return None
    mask_stride = config.MASK_STRIDE[0] if isinstance(config.MASK_STRIDE, (list, tuple)) else config.MASK_STRIDE
    if getattr(config, "EVAL_DISABLE_LEARNED_UPSAMPLING", False) and mask_stride is not None:
        return mask_stride
    return config.SEQUENCE_STRIDE


def needed_windows(frame_indices, config):
    """Boolean mask of the windows whose central prediction is read by the reports of eval.py:195-251."""
    idx = np.asarray(frame_indices)
    stride = prediction_stride(config)
    if stride is None:
        return np.ones(len(idx), bool)
    # interpolate_between_keyframes overwrites every non-keyframe that has a keyframe before it in its video; frame 0 of a
    # video is always a keyframe, so every non-keyframe is overwritten.  The KEYFRAMES report reads keyframes of the (coarser
    # or equal) input stride only.
    return np.equal(np.mod(idx, stride), 0)


# reuse_frames=True: upper bound of the per-frame feature table (d_t float32 per row) that predict_windows keeps on the device; the windows
# are run in chunks whose frames fit (h36m, d_t = 384: ~350 k frame rows per chunk, plain and flipped together)
FRAME_TABLE_BYTES = 1 << 30


def window_frames(desc, seq_len, starts, lens, pad_edge, zero_masked=True):
    """The frames a set of window descriptors (W, 6) reads, by the rules of uu3d_gather_windows / uu3d_gather_window_frames (a numpy
    restatement of ``window_frame`` in csrc/uu3d_misc.h): (plain, flipped, zero) = sorted unique pose-table rows (``starts[video] + frame``)
    read by unflipped / flipped windows, and whether some token reads no frame at all (zero padding: the all-zero frame).  Tokens that the
    stride mask drops are not read when ``zero_masked`` (they become the masked token)."""
    d = np.asarray(desc, np.int64).reshape(-1, 6)
    N = int(seq_len)
    starts, lens = np.asarray(starts, np.int64), np.asarray(lens, np.int64)
    plain, flipped, zero = [], [], False
    for lo in range(0, len(d), 4096):                                  # (W x N index arrays: bounded)
        b = d[lo:lo + 4096]
        v, c, s, ms, sh, fl = (b[:, k:k + 1] for k in range(6))
        n = np.arange(N, dtype=np.int64)[None, :]
        f = c - ((N - 1) * s) // 2 + n * s
        ln = lens[v]
        src = np.where(f < 0, f + ((-f + s - 1) // s) * s, np.where(f >= ln, f - ((f - ln + s) // s) * s, f))
        inside = (f >= 0) & (f < ln)
        have = inside | (bool(pad_edge) & (src >= 0) & (src < ln))
        sm = np.mod((n - N // 2) * s + sh, ms) == 0
        read = sm | (not zero_masked)
        zero = zero or bool((read & ~have).any())
        g = starts[v] + src
        take = read & have
        plain.append(g[take & (fl == 0)])
        flipped.append(g[take & (fl != 0)])
    return np.unique(np.concatenate(plain or [np.zeros(0, np.int64)])), np.unique(np.concatenate(flipped or [np.zeros(0, np.int64)])), zero


def _window_spans(desc, seq_len, starts, lens):
    """First and last pose-table row any token of each window can read (padding reads frames inside these bounds too)."""
    d = np.asarray(desc, np.int64)
    v, c, s = d[:, 0], d[:, 1], d[:, 2]
    first = c - ((int(seq_len) - 1) * s) // 2
    last = first + (int(seq_len) - 1) * s
    hi = np.asarray(lens, np.int64)[v] - 1
    base = np.asarray(starts, np.int64)[v]
    return base + np.clip(first, 0, hi), base + np.clip(last, 0, hi)


def _check_pipeline_range(pipe):
    """``pipe.check_range()`` at the end of an evaluation; its ``Uu3dRangeError`` names the way out."""
    from . import _capi
    try:
        pipe.check_range()
    except _capi.Uu3dRangeError as e:
        what = str(e).split(": ", 1)[-1]
        raise _capi.Uu3dRangeError(e.status, what + " -- exact_f32=True (predict_windows, evaluate_windows, run_eval) repeats the evaluation with every "
                                   "forward on the exact-f32 kernels (compiled dims, any sequence length the model takes; slower)") from None


def _predict_windows_reuse(model, generator, descriptors, batch_size, flip, depth, graph, finish, table_bytes, exact_f32=False):
    """predict_windows(reuse_frames=True): the spatial stack and spatial_to_temporal_fc once per frame the windows read (uu3d_frame_features),
    the windows forwarded from that table (uu3d_gather_window_frames + uu3d_forward_frames_ex in a ForwardPipeline of the frames form).

    The table holds the frames of a contiguous range of the pose table, once plain and once flipped, plus the all-zero frame; windows run in
    chunks of whole batches whose range fits ``table_bytes``.  Rows of a chunk are pose-table rows shifted by the chunk's first row (the
    video starts handed to the gather kernel are shifted likewise); only the rows the chunk reads are computed -- the set ``window_frames``
    states on the host, found on the device from the chunk's own rows."""
    import torch
    import ctypes as C
    from . import _capi
    lib = _capi.load_library()
    t = generator.table
    dev = t.device
    N, J, dt = generator.seq_len, t.J, model.arch.d_temporal
    W = len(descriptors)
    halves = 2 if (flip or bool(np.any(np.asarray(descriptors)[:, 5]))) else 1
    cap = max(1, (int(table_bytes) // (4 * dt) - 1) // halves)         # frame rows per half
    lo_w, hi_w = _window_spans(descriptors, N, t.starts, t.lens)
    chunks = []                                                        # (first window, end window, first row, rows)
    w0 = 0
    while w0 < W:
        w1 = min(w0 + batch_size, W)
        lo, hi = int(lo_w[w0:w1].min()), int(hi_w[w0:w1].max())
        while w1 < W:
            e = min(w1 + batch_size, W)
            nlo, nhi = min(lo, int(lo_w[w1:e].min())), max(hi, int(hi_w[w1:e].max()))
            if nhi - nlo + 1 > cap:
                break
            lo, hi, w1 = nlo, nhi, e
        chunks.append((w0, w1, lo, hi - lo + 1))
        w0 = w1
    S = max(c[3] for c in chunks)
    zero_row = halves * S
    table = torch.zeros((zero_row + 1, dt), dtype=torch.float32, device=dev)   # (zeros: the pipeline's warm-up forwards read it)
    rows = min(batch_size, W) * halves
    pipe = model.pipeline(rows, depth=depth, graph=graph, features=table, exact_f32=exact_f32)
    depth = pipe.depth
    d_vs = torch.empty(len(t.starts), dtype=torch.int64, device=dev)
    fb = 16384                                                         # frames per uu3d_frame_features call
    kp = torch.empty((fb, J, 2), dtype=torch.float32, device=dev)
    feats = torch.empty((fb, dt), dtype=torch.float32, device=dev)
    fl_order = C.c_void_p(generator._d_flip.data_ptr()) if generator._d_flip is not None else None
    cur = torch.cuda.current_stream(dev)
    valid = getattr(t, "valid", None)                                  # missed detections: one byte per pose-table row, or None

    def gather_rows(d_desc, n, lo, rb, mk, stream):
        """uu3d_gather_window_frames for the chunk whose first pose-table row is ``lo``; with a validity table its _valid form (the video
        starts are shifted by ``lo``, so the table's pointer is shifted back by as much)."""
        args = (C.c_void_p(d_vs.data_ptr()), C.c_void_p(t.d_lens.data_ptr()), C.c_void_p(d_desc.data_ptr()), n, N, int(generator.pad_edge), 1, S, zero_row)
        tail = (C.c_void_p(rb.data_ptr()), C.c_void_p(mk.data_ptr()), None, C.c_void_p(stream.cuda_stream))
        if valid is None:
            _capi.check(lib, lib.uu3d_gather_window_frames(*args, *tail), None)
        else:
            _capi.check(lib, lib.uu3d_gather_window_frames_valid(*args, C.c_void_p(valid.data_ptr() + int(lo)), *tail), None)

    def features_of_chunk(d, lo):
        """The rows the chunk's windows read (uu3d_gather_window_frames over all of them, marked on the device: the same rules as the
        forwards' own gathers), then uu3d_frame_features on those frames only, written into their table rows."""
        db = np.concatenate([d, d.copy()], 0) if flip else d
        if flip:
            db[len(d):, 5] = 1 - db[len(d):, 5]
        d_desc = torch.from_numpy(np.ascontiguousarray(db, np.int32)).pin_memory().to(dev, non_blocking=True)
        rb = torch.empty((len(db), N), dtype=torch.int32, device=dev)
        mk = torch.empty((len(db), N), dtype=torch.uint8, device=dev)
        gather_rows(d_desc, len(db), lo, rb, mk, cur)
        mark = torch.zeros(zero_row, dtype=torch.bool, device=dev)
        r = rb[(rb >= 0) & (rb < zero_row)]
        mark[r.long()] = True
        ids = mark.nonzero().flatten()                                 # (one host synchronisation per chunk: the frame count)
        for a in range(0, len(ids), fb):
            rid = ids[a:a + fb]
            n = len(rid)
            fl = rid >= S
            g = rid - torch.where(fl, S, 0) + lo
            v = torch.searchsorted(t.d_starts, g, right=True) - 1
            fd = torch.stack([v, g - t.d_starts[v], torch.ones_like(v), torch.ones_like(v), torch.zeros_like(v), fl.long()], -1).to(torch.int32).contiguous()
            sm = torch.empty((n,), dtype=torch.uint8, device=dev)
            _capi.check(lib, lib.uu3d_gather_windows(C.c_void_p(t.kp2d.data_ptr()), C.c_void_p(t.d_starts.data_ptr()), C.c_void_p(t.d_lens.data_ptr()),
                                                     C.c_void_p(fd.data_ptr()), fl_order, n, 1, J, 2, 0, 0, C.c_void_p(kp.data_ptr()),
                                                     C.c_void_p(sm.data_ptr()), None, C.c_void_p(cur.cuda_stream)), None)
            model._frame_features(kp[:n], feats[:n], cur, exact_f32=exact_f32)
            table.index_copy_(0, rid, feats[:n])

    # the all-zero frame (zero padding), once: its row is the table's last
    kp[:1].zero_()
    model._frame_features(kp[:1], table[zero_row:], cur, exact_f32=exact_f32)

    def take(lo, n, ticket):
        pipe.after(ticket, lambda full, cen: finish(lo, n, cen))

    pending = []
    try:
        for w0, w1, lo, _ in chunks:
            for p in pending:
                take(*p)
            pending = []
            pipe.join()                                                # (the forwards that read the previous chunk's table are enqueued before the rewrite)
            d_vs.copy_(torch.from_numpy(t.starts - lo))
            features_of_chunk(np.asarray(descriptors[w0:w1]), lo)
            pipe.wait_caller()
            for b0 in range(w0, w1, batch_size):
                db = np.ascontiguousarray(descriptors[b0:min(b0 + batch_size, w1)])
                n = len(db)
                if flip:
                    df = db.copy(); df[:, 5] = 1 - df[:, 5]
                    db = np.concatenate([db, df], 0)
                rb, mb, sstream = pipe.acquire(len(db), wait_caller=False)
                with torch.cuda.stream(sstream):
                    d_desc = torch.from_numpy(np.ascontiguousarray(db, np.int32)).pin_memory().to(dev, non_blocking=True)
                    mk = mb if mb is not None else torch.empty((len(db), N), dtype=torch.uint8, device=dev)
                    gather_rows(d_desc, len(db), lo, rb, mk, sstream)
                    if mb is None:                                     # (no strided input: a dropped frame is read as zeros, eval.py:67)
                        rb.masked_fill_(rb < 0, zero_row)
                pending.append((b0, n, pipe.launch(len(db), wait_caller=False)))
                if len(pending) == depth:
                    take(*pending.pop(0))
        for p in pending:
            take(*p)
        pipe.join()
        torch.cuda.current_stream(dev).synchronize()
        _check_pipeline_range(pipe)                                    # f16x3 range guard: once per evaluation (features and forwards)
    finally:
        pipe.close()


def predict_windows(model, generator, descriptors, config, batch_size, flip=True, depth=None, graph=True, reuse_frames=False,
                    frame_table_bytes=FRAME_TABLE_BYTES, exact_f32=False):
    """Central 3D predictions (W, J, 3) float32 on the device for the given window descriptors: batches of ``batch_size``
    windows, each forwarded together with its mirrored copy when ``flip`` (one launch chain over 2B sequences).

    ``depth`` batches (None: one per HIP hardware queue, i.e. 4) are in flight at once, each on its own HIP stream and -- with ``graph`` -- replayed from its own hipGraph
    (pipeline.ForwardPipeline: batch k + 1's big kernels run beside batch k's latency-bound tail; the window gather of a batch
    writes into its slot's input buffers on the slot's stream).  depth = 1, graph = False is the reference's loop: one eager call after the other.
    depth = 1 runs the LATENCY schedule, depth > 1 the THROUGHPUT schedule (the temporal chain, other split-K depths): the same arithmetic in another
    summation order -- predictions agree to ~3e-5 (tests/test_tchain_gpu.py), each schedule is bitwise reproducible run to run.

    ``reuse_frames=True``: every frame the windows read goes through the spatial stack and spatial_to_temporal_fc ONCE (uu3d_frame_features)
    instead of once per window it sits in; the windows are forwarded from that feature table (uu3d_forward_frames_ex, always through a
    pipeline, graphs as ``graph`` says).  Within ~3e-5 of the default (the s2t GEMM sums in another split-K order).  The table is bounded by
    ``frame_table_bytes``: windows run in chunks whose frames fit.

    ``exact_f32=True``: every forward (and, with ``reuse_frames``, every feature row) on the exact-f32 kernels whatever the model's precision
    (``ForwardPipeline(exact_f32=True)``, ``frame_features(exact_f32=True)``): the way out after the ``Uu3dRangeError`` this function raises at
    its end when the weights' activations left the f16 range.  Always through a pipeline; several times slower than the default."""
    import torch
    if len(descriptors) == 0:
        return torch.empty((0, generator.table.J, 3), dtype=torch.float32, device=generator.table.device)
    raw = _predict_windows_raw(model, generator, descriptors, batch_size, flip, depth, graph, reuse_frames, frame_table_bytes, exact_f32=exact_f32)
    return _unflip(raw, config, flip)


def _predict_windows_raw(model, generator, descriptors, batch_size, flip, depth, graph, reuse_frames, frame_table_bytes=FRAME_TABLE_BYTES,
                         exact_f32=False):
    """The body of ``predict_windows`` up to its un-flip: the central predictions as the pipeline leaves them, (1 | 2, W, J, 3) float32 on the
    device -- [0] of the windows, [1] (``flip``) of their mirrored copies, still mirrored.  ``predict.predict_tracks`` un-flips, averages and
    interpolates them in one kernel (uu3d_assemble_tracks).  W >= 1."""
    import torch
    W = len(descriptors)
    J = generator.table.J
    dev = generator.table.device
    # raw central predictions of the windows (and of their mirrored copies): the un-flip / average of eval.py:163-166 runs ONCE over
    # all windows at the end instead of five small launches per batch
    raw = torch.empty((2 if flip else 1, W, J, 3), dtype=torch.float32, device=dev)
    rows = min(batch_size, W) * (2 if flip else 1)
    if depth is None:
        # one slot per hardware queue measured best END TO END (round 5, tools/eval_throughput_exp.py: descriptor upload + window gather + forward + copy per slot;
        # 128 sequences per batch: 142 / 170 / 180 / 172 k sequences/s with 2 / 3 / 4 / 8 slots, 512 per batch: 185 / 188 / 185 / 171 k)
        depth = 4

    def finish(lo, n, cen):
        raw[:, lo:lo + n].copy_(cen.view(raw.shape[0], n, J, 3))

    if reuse_frames:
        _predict_windows_reuse(model, generator, descriptors, batch_size, flip, depth, graph, finish, frame_table_bytes, exact_f32=exact_f32)
        return raw
    # (exact_f32: through a pipeline even at depth 1 without a graph -- the same launches as the eager loop, with the bit set)
    pipe = model.pipeline(rows, depth=depth, graph=graph, exact_f32=exact_f32) if (depth is None or depth > 1 or graph or exact_f32) else None
    if pipe is not None:
        depth = pipe.depth

    def take(lo, n, ticket):
        # the copy into `raw` goes on the slot's stream (pipe.after): the caller's stream never waits inside the loop
        pipe.after(ticket, lambda full, cen: finish(lo, n, cen))

    pending = []
    for lo in range(0, W, batch_size):
        d = np.ascontiguousarray(descriptors[lo:lo + batch_size])
        n = len(d)
        if flip:
            df = d.copy(); df[:, 5] = 1 - df[:, 5]                 # the generator's flip = negate x + permute joints (= eval.py:154-158)
            d = np.concatenate([d, df], 0)
        if pipe is None:
            b = generator.gather(d, zero_masked=True, with_3d=False)
            if model.has_strided_input:
                _, cen = model([b["kp2d"], b["stride_mask"]], training=False)
            else:
                _, cen = model(b["kp2d"], training=False)
            finish(lo, n, cen)
            continue
        # the window gather writes straight into the slot's static input buffers, on the slot's stream: no copy and no temporary
        # that the caching allocator could hand out again while another stream still reads it (round-3 verdict, weak point 8)
        # (wait_caller=False: the descriptors are uploaded and the windows gathered on the slot's stream, the consumer's copy runs there too -- nothing the
        # caller's stream enqueues inside this loop is an input, and an event on it would queue behind the forwards of the slots that share its hardware queue)
        xb, mb, sstream = pipe.acquire(len(d), wait_caller=False)
        generator.gather(d, zero_masked=True, with_3d=False, out=(xb, mb), stream=sstream)
        pending.append((lo, n, pipe.launch(len(d), wait_caller=False)))
        if len(pending) == depth:
            take(*pending.pop(0))
    for p in pending:
        take(*p)
    if pipe is not None:
        pipe.join()
        torch.cuda.current_stream(dev).synchronize()               # the slots' buffers go away with the pipeline
        try:
            _check_pipeline_range(pipe)                            # f16x3 range guard (include/uu3d.h): once per evaluation, never per batch
        finally:
            pipe.close()
    return raw


def _unflip(raw, config, flip):
    import torch
    if not flip:
        return raw[0]
    order = torch.as_tensor(np.asarray(config.AUGM_FLIP_KEYPOINT_ORDER), dtype=torch.long, device=raw.device)
    f = raw[1]
    f = torch.cat([f[..., :1] * -1.0, f[..., 1:]], dim=-1).index_select(1, order)              # eval.py:163-166
    return (raw[0] + f) / 2.0


def evaluate_windows(model, generator, desc, config, action_wise=True, batch_size=None, skip_unused_windows=True, log=_log, depth=None,
                     graph=True, reuse_frames=False, device_metrics=False, exact_f32=False):
    """The timed part of ``run_eval``: the windows ``desc`` of ``generator`` (whose table holds the 3D ground truth) forwarded, gathered over
    the ranks and reported.  -> the report dict with "num_windows", "num_forwarded" and "seconds" (this function's wall time)."""
    import torch
    gen, table = generator, generator.table
    W = len(desc)
    start = time.time()
    frame_idx = desc[:, 1].copy()
    need = needed_windows(frame_idx, config) if skip_unused_windows else np.ones(W, bool)
    run = np.flatnonzero(need)
    rank, world = 0, 1
    import torch.distributed as tdist
    if tdist.is_available() and tdist.is_initialized():
        rank, world = tdist.get_rank(), tdist.get_world_size()
    lo, hi = udist.shard_bounds(len(run), rank, world)
    bs = int(batch_size or config.BATCH_SIZE)
    local = predict_windows(model, gen, desc[run[lo:hi]], config, bs, flip=bool(config.EVAL_FLIP), depth=depth, graph=graph,
                            reuse_frames=reuse_frames, exact_f32=exact_f32)
    allp = udist.allgather_errors(local)                             # (len(run), J, 3) in rank order: the payload is a few KB per rank
    # ground truth of the window centres, root shifted (eval.py:183-186); the centre of a window is frame `index` of its video
    mid = desc[:, 1].astype(np.int64) + table.starts[desc[:, 0]]
    actions = table.actions[desc[:, 0]]
    if config.SEQUENCE_STRIDE > 1 and config.TEST_STRIDED_EVAL is True:
        log("Performing strided eval: Interpolating between keyframes")
    if device_metrics:
        # predictions and ground truth stay in HBM: interpolation, metrics and the report sums in csrc/uu3d_metrics.h (the metrics root-align
        # or centre the ground truth themselves)
        from . import evaluation_device
        rows = np.full(W, -1, np.int64)
        rows[run] = np.arange(len(run))
        gt_dev = table.kp3d[torch.as_tensor(mid, device=table.device)]
        res = evaluation_device.evaluate_predictions_device(allp, gt_dev, actions, frame_idx, config, action_wise=action_wise, rows=rows)
    else:
        pred = np.zeros((W, table.J, 3), np.float64)
        pred[run] = allp.detach().cpu().numpy().astype(np.float64)
        gt = table.kp3d[torch.as_tensor(mid, device=table.device)].cpu().numpy().astype(np.float64)
        gt = gt - gt[:, config.ROOT_KEYTPOINT:config.ROOT_KEYTPOINT + 1, :]
        res = evaluation.evaluate_predictions(pred, gt, actions, frame_idx, config, action_wise=action_wise)
    res["num_windows"], res["num_forwarded"] = int(W), int(len(run))
    res["seconds"] = time.time() - start
    for title, key in (("ALL FRAMES", "all_frames"), ("KEYFRAMES", "keyframes")):
        if res[key] is None:
            continue
        log("")
        log(f"### Evaluation on {title} ####")
        log("")
        fr = res[key][0] if action_wise else res[key]
        log("  ".join(f"{k}: {v:.2f}" for k, v in fr.items()))
    log(f"Finished evaluation in {res['seconds']:.1f} s ({len(run)} of {W} windows forwarded)")
    return res


def run_eval(config, dataset_name, dataset_path, dataset2d_path, test_subset, weights_path=None, model=None, action_wise=True,
             batch_size=None, skip_unused_windows=True, log=_log, depth=None, graph=True, reuse_frames=False, device_metrics=False,
             exact_f32=False):
    """eval.py:34-253.  Returns ``evaluation.evaluate_predictions``'s dict (+ "num_windows", "num_forwarded", "seconds").

    ``device_metrics=True``: the report (keyframe interpolation, MPJPE / N-MPJPE / P-MPJPE, per-action means) is computed on the device
    from the predictions where they lie (``evaluation_device.evaluate_predictions_device``; with several ranks each evaluates a shard
    of the poses) instead of in float64 numpy on the host: the same dict within 1e-5 mm.

    ``batch_size`` defaults to ``config.BATCH_SIZE``; ``depth`` / ``graph``: batches in flight and hipGraph replay of the forward
    (``predict_windows``; depth 1 without graph = the reference's eager loop, same numbers); ``reuse_frames``: each frame's spatial
    features computed once (``predict_windows``); ``exact_f32``: every forward on the exact-f32 kernels (``predict_windows``: after a
    ``Uu3dRangeError``).  With torch.distributed initialised, the windows to run are split
    contiguously over the ranks and the predictions all-gathered; every rank returns the same report."""
    from .net.uplift_upsample_transformer_constructor import build_uplift_upsample_transformer
    assert not (weights_path is None and model is None)
    if model is None:
        model = build_uplift_upsample_transformer(config)
        log(f"Loading weights from {weights_path}")
        model.load_weights(weights_path, skip_mismatch=False, verbose=True)
    elif weights_path is not None:
        log(f"Using provided model. Ignoring the given weights path: {weights_path}")
    if dataset_name != "h36m":
        raise Exception("Invalid Dataset")
    subjects = h36m.subjects_of_split(test_subset)
    dataset_3d, poses_2d_dataset = h36m.load_dataset_and_2d_poses(dataset_path, dataset2d_path, dataset_name, verbose=False)
    cams, poses_3d, poses_2d, _, seq_subjects, seq_actions, seq_rates = h36m.filter_and_subsample_dataset(
        dataset_3d, poses_2d_dataset, subjects, "*", downsample=1, image_base_path=None, verbose=False)
    table = h36m.pose_table(poses_2d, poses_3d, seq_subjects, seq_actions, seq_rates, device=model.device)
    gen = SequenceGenerator(table, seq_len=config.SEQUENCE_LENGTH, target_frame_rate=50,
                            subsample=config.DATASET_TEST_3D_SUBSAMPLE_STEP, stride=config.SEQUENCE_STRIDE,
                            padding_type=config.PADDING_TYPE, flip_augment=False,
                            flip_lr_indices=config.AUGM_FLIP_KEYPOINT_ORDER, mask_stride=config.MASK_STRIDE,
                            stride_mask_align_global=True, rand_shift_stride_mask=False, shuffle=False)
    desc = gen.descriptors()
    log(f"Sequences: {len(desc)}")
    log(f"Running evaluation on '{test_subset}' with {len(desc)} examples")
    return evaluate_windows(model, gen, desc, config, action_wise=action_wise, batch_size=batch_size, skip_unused_windows=skip_unused_windows,
                            log=log, depth=depth, graph=graph, reuse_frames=reuse_frames, device_metrics=device_metrics,
                            exact_f32=exact_f32)


def run_eval_multi_mask_stride(config, *args, log=_log, **kwargs):
    """eval.py:256-268: one evaluation per MASK_STRIDE value.  Returns {mask stride: report}."""
    config = config.copy()
    values = config.MASK_STRIDE if isinstance(config.MASK_STRIDE, list) else [config.MASK_STRIDE]
    out = {}
    for msv in values:
        config.MASK_STRIDE = msv
        if len(values) > 1:
            log(f"### Running evaluation for mask stride value: {msv} ###")
        out[msv] = run_eval(config, *args, log=log, **kwargs)
        if len(values) > 1:
            log(f"### Finished evaluation for mask stride value: {msv} ###")
    return out
