"""Host side of the evaluation protocol: the metrics and the bookkeeping that eval.py runs on
the collected predictions, in float64 numpy like the reference, but batched (no per-pose Python loop).

* ``mpjpe / nmpjpe / pmpjpe``          -- common/dataset/metrics.py:13-37, 40-84, 87-118 (+ optimal_scaling :121-134,
                                          compute_similarity_transform :137-201 as one batched SVD)
* ``frame_wise_eval / h36_action_wise_eval`` -- common/dataset/action_wise_eval.py:17-74
* ``interpolate_between_keyframes``     -- action_wise_eval.py:77-100
* ``evaluate_predictions``              -- eval.py:214-251 (ALL FRAMES / KEYFRAMES evaluation of a finished run)

Inputs: ``pred`` (B, K, 3) root-relative predictions in metres, ``gt`` (B, K, 4) = (x, y, z, valid).  Per-joint
results use -1 for invalid ground truth, averages run over entries >= 0 (action_wise_eval.py:22).
"""
import numpy as np

# common/dataset/h36m_splits.py:73-76
H36M_ACTIONS = ["Directions", "Discussion", "Eating", "Greeting", "Phoning", "Photo", "Posing", "Purchases",
                "Sitting", "SittingDown", "Smoking", "Waiting", "WalkDog", "Walking", "WalkTogether"]
METRICS = ["mpjpe", "nmpjpe", "pampjpe"]


def _finish(dist, valid, normalize):
    if normalize is False:
        return np.where(valid, dist, -1.)
    return np.sum(np.where(valid, dist, 0.)) / float(np.sum(valid > 0.))


def mpjpe(pred, gt, root_index, normalize=True):
    gt3d, valid = gt[:, :, :3], gt[:, :, 3] > 0
    p = pred - pred[:, [root_index], :]
    g = gt3d - gt3d[:, [root_index], :]
    return _finish(np.linalg.norm(p - g, ord=2, axis=-1), valid, normalize)


def nmpjpe(pred, gt, root_index, alignment="root", normalize=True):
    gt3d, valid = gt[:, :, :3], gt[:, :, 3] > 0
    if alignment == "mean":
        n = np.sum(valid, axis=1)
        g = gt3d - (np.sum(gt3d * valid[:, :, None], axis=1) / n[:, None])[:, None, :]
        p = pred - (np.sum(pred * valid[:, :, None], axis=1) / n[:, None])[:, None, :]
    else:
        g = gt3d - gt3d[:, [root_index], :]
        p = pred - pred[:, [root_index], :]
    mp, mg = p * valid[:, :, None], g * valid[:, :, None]
    s_opt = np.sum(mp * mg, axis=(1, 2)) / np.sum(mp * mp, axis=(1, 2))          # optimal_scaling, metrics.py:121-134
    return _finish(np.linalg.norm(p * s_opt[:, None, None] - g, ord=2, axis=-1), valid, normalize)


def procrustes_align(pred, gt3d):
    """Similarity transform (scale, rotation, translation) of every pose of ``pred`` onto ``gt3d``: the batched form of
    compute_similarity_transform(X=gt, Y=pred, compute_optimal_scale=True) (metrics.py:137-201)."""
    muX, muY = gt3d.mean(axis=1, keepdims=True), pred.mean(axis=1, keepdims=True)
    X0, Y0 = gt3d - muX, pred - muY
    normX = np.sqrt(np.square(X0).sum(axis=(1, 2)))
    normY = np.sqrt(np.square(Y0).sum(axis=(1, 2)))
    X0, Y0 = X0 / normX[:, None, None], Y0 / normY[:, None, None]
    A = np.einsum("bki,bkj->bij", X0, Y0)                       # X0^T Y0
    U, s, Vt = np.linalg.svd(A, full_matrices=False)
    V = np.transpose(Vt, (0, 2, 1))
    det = np.linalg.det(np.einsum("bij,bkj->bik", V, U))       # det(V U^T)
    sign = np.sign(det)
    V = V.copy(); s = s.copy()
    V[:, :, -1] *= sign[:, None]
    s[:, -1] *= sign
    T = np.einsum("bij,bkj->bik", V, U)
    trace = s.sum(axis=1)
    return (normX * trace)[:, None, None] * np.einsum("bki,bij->bkj", Y0, T) + muX


def pmpjpe(pred, gt, normalize=True):
    gt3d, valid = gt[:, :, :3], gt[:, :, 3] > 0
    aligned = procrustes_align(np.asarray(pred, np.float64), np.asarray(gt3d, np.float64))
    bad = ~np.isfinite(aligned).all(axis=(1, 2))               # the reference keeps the raw prediction when the SVD fails (:107-109)
    if bad.any():
        aligned[bad] = pred[bad]
    return _finish(np.linalg.norm(aligned - gt3d, ord=2, axis=-1), valid, normalize)


def _average(a):
    return np.mean(a[a >= 0])


def _frame_metrics(pred_3d, gt_3d, root_index):
    return {"mpjpe": mpjpe(pred_3d, gt_3d, root_index, normalize=False) * 1000.,
            "nmpjpe": nmpjpe(pred_3d, gt_3d, root_index, alignment="root", normalize=False) * 1000.,
            "pampjpe": pmpjpe(pred_3d, gt_3d, normalize=False) * 1000.}


def frame_wise_eval(pred_3d, gt_3d, root_index):
    fm = _frame_metrics(pred_3d, gt_3d, root_index)
    return {k: _average(v) for k, v in fm.items()}


def h36_action_wise_eval(pred_3d, gt_3d, actions, root_index, action_set=None):
    """-> (frame_results, average_results, per_action_results), millimetres (action_wise_eval.py:17-54)."""
    action_set = H36M_ACTIONS if action_set is None else action_set
    fm = _frame_metrics(pred_3d, gt_3d, root_index)
    per_action = {}
    for a_i, name in enumerate(action_set):
        sel = np.where(actions == a_i)
        per_action[name] = {k: _average(fm[k][sel]) for k in METRICS}
    frame_results = {k: _average(fm[k]) for k in METRICS}
    average_results = {k: np.mean([d[k] for d in per_action.values()]) for k in METRICS}
    return frame_results, average_results, per_action


def interpolate_between_keyframes(pred3d, frame_indices, keyframe_stride):
    """Linear interpolation of the predictions between keyframes (frame index % stride == 0) of each video; frames after
    the last keyframe repeat it; a drop of the frame index starts a new video (action_wise_eval.py:77-100).  Frames before
    the first keyframe of a video keep their own prediction (the reference indexes with ``None`` there)."""
    interp = np.copy(pred3d)
    frame_indices = np.asarray(frame_indices)
    keyframes = np.equal(np.mod(frame_indices, keyframe_stride), 0)
    last = None
    for i, (f, is_key) in enumerate(zip(frame_indices, keyframes)):
        if i > 0 and f <= frame_indices[i - 1]:
            last = None
        if is_key:
            if last is not None and i - last > 1:
                k = np.arange(last + 1, i)
                w_right = ((k - last) / float(i - last)).reshape((-1,) + (1,) * (pred3d.ndim - 1))
                interp[k] = pred3d[last] * (1.0 - w_right) + pred3d[i] * w_right
            last = i
        elif last is not None:
            interp[i] = pred3d[last]
    return interp, keyframes


def keyframe_plan(frame_indices, keyframe_stride, rows=None):
    """``interpolate_between_keyframes`` as a gather plan, without a loop over frames: -> (left, right, weight, keyframes) with
    ``interp[i] = pred3d[left[i]] * (1 - weight[i]) + pred3d[right[i]] * weight[i]``.  A keyframe, a frame in front of its video's first
    keyframe and a frame behind its last one have ``left == right`` and weight 0 (their own prediction, or the last keyframe's); the
    weight counts positions, not frame numbers.

    ``rows`` (positions -> row of the array that holds the forwarded predictions, -1: not forwarded): left / right are returned as
    rows of that array, and a position whose plan needs a row that was not forwarded raises ValueError."""
    f = np.asarray(frame_indices).astype(np.int64)
    n = len(f)
    pos = np.arange(n, dtype=np.int64)
    key = np.equal(np.mod(f, keyframe_stride), 0)
    new = np.ones(n, bool)
    new[1:] = f[1:] <= f[:-1]                                        # a drop (or repeat) of the frame index starts a new video
    video = np.cumsum(new) - 1
    start = np.maximum.accumulate(np.where(new, pos, 0)) if n else pos
    last = np.maximum.accumulate(np.where(key, pos, -1)) if n else pos
    has_last = last >= start
    nxt = np.minimum.accumulate(np.where(key, pos, n)[::-1])[::-1] if n else pos
    has_next = nxt < n
    has_next[has_next] = video[nxt[has_next]] == video[has_next]
    between = ~key & has_last & has_next
    tail = ~key & has_last & ~has_next
    left, right, weight = pos.copy(), pos.copy(), np.zeros(n, np.float64)
    left[between], right[between] = last[between], nxt[between]
    weight[between] = (pos[between] - last[between]) / (nxt[between] - last[between]).astype(np.float64)
    left[tail] = right[tail] = last[tail]
    if rows is not None:
        rows = np.asarray(rows).astype(np.int64)
        left, right = rows[left], rows[right]
        missing = np.flatnonzero((left < 0) | (right < 0))
        if len(missing):
            raise ValueError(f"{len(missing)} positions need a prediction that was not forwarded (first: position {int(missing[0])}, "
                             f"frame {int(f[missing[0]])})")
    return left, right, weight, key


def keyframe_plan_at(frame_indices, keyframe_stride, positions, rows=None):
    """``keyframe_plan`` at rational positions: a video's motion is the piecewise-linear function through its keyframes (frames behind the
    last keyframe repeat it), and this reads it anywhere, not only at whole frames -> (left, right, weight), one entry per position.

    ``positions`` = (video, num, den), three integer arrays: entry i asks for position ``num[i] / den[i]`` (in frames, counted from the
    first frame of the video, exact) of video ``video[i]``; videos are numbered as ``frame_indices`` lists them (a drop of the frame index
    starts the next one).  Positions lie in [0, frames of the video - 1].  An integral position gives ``keyframe_plan``'s own entry for that
    frame: the same rows and the same bits of the weight (the same integer / integer float64 division).  A fractional position between
    frames p and p + 1 lies between the last keyframe L at or before p and the first keyframe N behind p; its weight is
    ``((p - L) * den + num - p * den) / ((N - L) * den)``, one float64 division of two integers below 2^53.  Without N it repeats L, and
    without L (in front of the video's first keyframe, where every frame keeps its own prediction) it takes frame p.  ``rows`` as in
    ``keyframe_plan``.  ``keyframe_stride`` 1: every frame is a keyframe."""
    f = np.asarray(frame_indices).astype(np.int64)
    n = len(f)
    video, num, den = (np.asarray(a).astype(np.int64).reshape(-1) for a in positions)
    if not (len(video) == len(num) == len(den)):
        raise ValueError("positions must be three arrays of one length: video, numerator, denominator")
    pl, pr, pw, key = keyframe_plan(f, keyframe_stride)
    new = np.ones(n, bool)
    new[1:] = f[1:] <= f[:-1]
    starts = np.flatnonzero(new)
    lens = np.diff(np.append(starts, n))
    if len(video) and (video.min() < 0 or video.max() >= len(starts)):
        raise ValueError(f"positions name video {int(video.max() if video.max() >= len(starts) else video.min())}, there are {len(starts)}")
    if (den < 1).any() or (num < 0).any():
        raise ValueError("positions must be num / den with num >= 0 and den >= 1")
    p = num // den
    frac = num - p * den
    if (p + (frac > 0) > lens[video] - 1).any():
        i = int(np.flatnonzero(p + (frac > 0) > lens[video] - 1)[0])
        raise ValueError(f"position {int(num[i])}/{int(den[i])} lies behind the last frame of video {int(video[i])} ({int(lens[video[i]])} frames)")
    g = starts[video] + p                                              # the frame at or before the position, as a place in frame_indices
    left, right, weight = pl[g].copy(), pr[g].copy(), pw[g].copy()     # integral positions: keyframe_plan's entries
    pos = np.arange(n, dtype=np.int64)
    vid = np.cumsum(new) - 1
    last = np.maximum.accumulate(np.where(key, pos, -1)) if n else pos
    nxt = np.append(np.minimum.accumulate(np.where(key, pos, n)[::-1])[::-1], n)[1:] if n else pos      # first keyframe BEHIND a place
    fr = frac > 0
    L, N = last[g], nxt[g]
    has_last = L >= starts[video]
    has_next = N < n
    has_next[has_next] = vid[N[has_next]] == video[has_next]
    between, tail = fr & has_last & has_next, fr & has_last & ~has_next
    wn, wd = (g - L) * den + frac, (N - L) * den
    if between.any() and max(int(wn[between].max()), int(wd[between].max())) >= 2 ** 53:
        raise ValueError("position too fine: the weight's integers must stay below 2^53")
    left[between], right[between] = L[between], N[between]
    weight[between] = wn[between] / wd[between].astype(np.float64)
    left[tail] = right[tail] = L[tail]
    weight[tail] = 0.0
    own = fr & ~has_last
    left[own] = right[own] = g[own]
    weight[own] = 0.0
    if rows is not None:
        rows = np.asarray(rows).astype(np.int64)
        left, right = rows[left], rows[right]
        missing = np.flatnonzero((left < 0) | (right < 0))
        if len(missing):
            raise ValueError(f"{len(missing)} positions need a prediction that was not forwarded (first: position {int(num[missing[0]])}/"
                             f"{int(den[missing[0]])} of video {int(video[missing[0]])})")
    return left, right, weight


def _outer_keyframes(frame_indices, keyframe_stride, left, right, rows, where):
    """What the cubic plans add to the linear ones.  ``left`` / ``right``: a linear plan as PLACES in ``frame_indices`` -> (before, after):
    per entry with ``left != right`` the keyframe in front of ``left`` and the one behind ``right`` in the same video, -1 where the video
    has none; -1 wherever ``left == right``.  With ``rows`` they are returned as rows, as ``keyframe_plan`` returns left and right.
    ``where(i)`` names entry i in an error message."""
    f = np.asarray(frame_indices).astype(np.int64)
    n = len(f)
    pos = np.arange(n, dtype=np.int64)
    key = np.equal(np.mod(f, keyframe_stride), 0)
    new = np.ones(n, bool)
    new[1:] = f[1:] <= f[:-1]                                        # a drop (or repeat) of the frame index starts a new video
    video = np.cumsum(new) - 1
    last = np.maximum.accumulate(np.where(key, pos, -1)) if n else pos
    nxt = np.minimum.accumulate(np.where(key, pos, n)[::-1])[::-1] if n else pos
    in_front = np.concatenate([[-1], last[:-1]]).astype(np.int64)    # the last keyframe strictly in front of a place (-1: none)
    behind = np.concatenate([nxt[1:], [n]]).astype(np.int64)         # the first keyframe strictly behind a place (n: none)
    mixed = np.flatnonzero(left != right)
    L, N = left[mixed], right[mixed]
    b, a = in_front[L], behind[N]
    b = np.where((b >= 0) & (video[np.maximum(b, 0)] == video[L]), b, -1)
    a = np.where((a < n) & (video[np.minimum(a, n - 1)] == video[N]), a, -1)
    uneven = np.flatnonzero(((b >= 0) & (L - b != N - L)) | ((a >= 0) & (a - N != N - L)))
    if len(uneven):
        u = uneven[0]
        raise ValueError(f"the cubic rule needs equally spaced keyframes: around {where(int(mixed[u]))} they lie at places "
                         f"{[int(x) for x in (b[u], L[u], N[u], a[u]) if x >= 0]}")
    if rows is not None:
        rows = np.asarray(rows).astype(np.int64)
        has_b, has_a = b >= 0, a >= 0
        b, a = np.where(has_b, rows[np.maximum(b, 0)], -1), np.where(has_a, rows[np.maximum(a, 0)], -1)
        missing = np.flatnonzero((has_b & (b < 0)) | (has_a & (a < 0)))
        if len(missing):
            raise ValueError(f"{len(missing)} positions need a prediction that was not forwarded (first: {where(int(mixed[missing[0]]))})")
    before, after = np.full(len(left), -1, np.int64), np.full(len(left), -1, np.int64)
    before[mixed], after[mixed] = b, a
    return before, after


def keyframe_plan_cubic(frame_indices, keyframe_stride, rows=None):
    """``keyframe_plan`` for the C1 cubic through the keyframes (``interpolate_cubic_host``) -> (before, left, right, after, weight).
    ``left`` / ``right`` / ``weight`` are ``keyframe_plan``'s own; ``before`` / ``after``: the keyframe in front of ``left`` and the one
    behind ``right`` in the same video, -1 where there is none and wherever ``left == right``.  The rule takes the four keyframes as
    equally spaced in positions: ValueError where they are not.  ``rows`` as in ``keyframe_plan``, for all four."""
    left, right, weight, _ = keyframe_plan(frame_indices, keyframe_stride, rows=rows)
    pl, pr = (left, right) if rows is None else keyframe_plan(frame_indices, keyframe_stride)[:2]
    f = np.asarray(frame_indices)
    before, after = _outer_keyframes(f, keyframe_stride, pl, pr, rows, lambda i: f"position {i}, frame {int(f[i])}")
    return before, left, right, after, weight


def keyframe_plan_cubic_at(frame_indices, keyframe_stride, positions, rows=None):
    """``keyframe_plan_at`` for the C1 cubic through the keyframes -> (before, left, right, after, weight), one entry per position:
    ``left`` / ``right`` / ``weight`` are ``keyframe_plan_at``'s own, ``before`` / ``after`` as in ``keyframe_plan_cubic``."""
    left, right, weight = keyframe_plan_at(frame_indices, keyframe_stride, positions, rows=rows)
    pl, pr = (left, right) if rows is None else keyframe_plan_at(frame_indices, keyframe_stride, positions)[:2]
    video, num, den = (np.asarray(a).astype(np.int64).reshape(-1) for a in positions)
    before, after = _outer_keyframes(frame_indices, keyframe_stride, pl, pr, rows,
                                     lambda i: f"position {int(num[i])}/{int(den[i])} of video {int(video[i])}")
    return before, left, right, after, weight


def interpolate_cubic_host(pred3d, plan):
    """The C1 motion through the keyframes, in numpy: ``pred3d`` (W, ...) float32 predictions, ``plan`` = (before, left, right, after,
    weight) of ``keyframe_plan_cubic`` / ``keyframe_plan_cubic_at`` as rows of ``pred3d`` -> (F, ...) float32.

    Where ``left == right`` the value is that prediction, its own bits (a keyframe, a frame behind the last keyframe of its video, one in
    front of the first).  Else it lies on the cubic Hermite segment from P1 = pred[left] (t = 0) to P2 = pred[right] (t = 1), t = weight,
    whose tangents are Catmull-Rom's over equally spaced keyframes: half the difference of the two neighbours, with P0 = pred[before]
    and P3 = pred[after], or the segment's own difference where before / after is -1.  Consecutive segments share the tangent at
    their common keyframe, so the motion has a continuous velocity; a quadratic in time is reproduced where all four keyframes exist.
    All in float64 on the float32 predictions, every operation rounded on its own, in exactly this order, rounded once to float32 --
    uu3d_assemble_tracks_cubic computes the same bits.  A row outside the predictions gives NaN (before / after: other than -1)."""
    pred = np.asarray(pred3d)
    if pred.dtype != np.float32:
        raise ValueError("interpolate_cubic_host takes float32 predictions")
    before, left, right, after = (np.asarray(a).astype(np.int64) for a in plan[:4])
    weight = np.asarray(plan[4], np.float64)
    W = len(pred)
    out = np.full((len(left),) + pred.shape[1:], np.nan, np.float32)
    inside = (left >= 0) & (left < W) & (right >= 0) & (right < W)
    own = inside & (left == right)
    out[own] = pred[left[own]]
    mix = np.flatnonzero(inside & (left != right) & (before >= -1) & (before < W) & (after >= -1) & (after < W))
    each = (-1,) + (1,) * (pred.ndim - 1)                              # one value per frame, for all of its joints and coordinates
    has0, has3 = (before[mix] >= 0).reshape(each), (after[mix] >= 0).reshape(each)
    t = weight[mix].reshape(each)
    P0, P1 = pred[np.maximum(before[mix], 0)].astype(np.float64), pred[left[mix]].astype(np.float64)
    P2, P3 = pred[right[mix]].astype(np.float64), pred[np.maximum(after[mix], 0)].astype(np.float64)
    m1 = np.where(has0, (P2 - P0) * 0.5, P2 - P1)
    m2 = np.where(has3, (P3 - P1) * 0.5, P2 - P1)
    t2 = t * t
    t3 = t2 * t
    h01 = 3.0 * t2 - 2.0 * t3
    h00 = 1.0 - h01
    h11 = t3 - t2
    h10 = (h11 - t2) + t
    out[mix] = ((h00 * P1 + h01 * P2) + h10 * m1) + h11 * m2
    return out


def report_from_sums(sums, action_wise=True, action_set=None):
    """The report of ``h36_action_wise_eval`` / ``frame_wise_eval`` from a table ``sums[a, m] = (sum of the errors >= 0 in metres, their
    count)`` with the actions of ``action_set`` in rows 0 .. A-1 and all poses in the last row (uu3d_pose_errors / uu3d_error_sums):
    means over entries >= 0 in millimetres; average_results is the plain mean of the per-action means."""
    sums = np.asarray(sums, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = sums[..., 0] / sums[..., 1] * 1000.
    frame_results = {k: mean[-1, m] for m, k in enumerate(METRICS)}
    if not action_wise:
        return frame_results
    action_set = H36M_ACTIONS if action_set is None else action_set
    assert len(mean) == len(action_set) + 1
    per_action = {name: {k: mean[a, m] for m, k in enumerate(METRICS)} for a, name in enumerate(action_set)}
    average_results = {k: np.mean([d[k] for d in per_action.values()]) for k in METRICS}
    return frame_results, average_results, per_action


def evaluate_predictions(pred3d, gt3d, actions, frame_indices, config, action_wise=True):
    """The bookkeeping of eval.py:195-251 on a finished run: pred3d (B,K,3), gt3d (B,K,3) root-relative, actions (B,),
    frame_indices (B,).  -> {"all_frames": ..., "keyframes": ... or None}; each entry is
    (frame_results, average_results, per_action_results) when ``action_wise`` else frame_results."""
    gt = np.concatenate([np.asarray(gt3d, np.float64), np.ones(np.shape(gt3d)[:-1] + (1,))], axis=-1)   # dummy valid flag
    pred = np.asarray(pred3d, np.float64)
    full_pred = pred
    mask_stride = config.MASK_STRIDE[0] if isinstance(config.MASK_STRIDE, (list, tuple)) else config.MASK_STRIDE
    if config.SEQUENCE_STRIDE > 1 and config.TEST_STRIDED_EVAL is True:
        strides = np.tile([config.SEQUENCE_STRIDE], reps=(len(frame_indices)))
        if getattr(config, "EVAL_DISABLE_LEARNED_UPSAMPLING", False) and mask_stride is not None:
            strides[:] = mask_stride
        pred, _ = interpolate_between_keyframes(pred, frame_indices, strides)

    def run(p, g, a):
        if action_wise:
            return h36_action_wise_eval(p, g, a, config.ROOT_KEYTPOINT)
        return frame_wise_eval(p, g, config.ROOT_KEYTPOINT)

    out = {"all_frames": run(pred, gt, np.asarray(actions)), "keyframes": None}
    if (config.SEQUENCE_STRIDE > 1 or (mask_stride is not None and mask_stride > 1)) and config.TEST_STRIDED_EVAL is True:
        input_stride = config.SEQUENCE_STRIDE if mask_stride is None else mask_stride
        key = np.equal(np.mod(frame_indices, input_stride), 0)
        out["keyframes"] = run(full_pred[key], gt[key], np.asarray(actions)[key])
    return out
