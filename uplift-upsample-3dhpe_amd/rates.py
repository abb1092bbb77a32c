"""The host arithmetic of frame rates, strides and lookaheads for ``predict.predict_tracks(fps=F, out_fps=G)`` and
``stream.StreamSession(fps=F, out_fps=G)``: integers, ``Fraction``s and numpy only -- nothing here touches a device.  ``predict`` and
``stream`` re-export these names; the rules they implement are defined in those modules' docstrings.  ``keyframe_bracket`` is THE bracket
rule: the two keyframes around a rational model position and the weight between them."""
import argparse
import collections
import math
from fractions import Fraction

import numpy as np

from . import eval as ev


def frame_rate(value):
    """One frame rate as an exact ``Fraction``: an int, a ``Fraction``, a ``(num, den)`` tuple of two integers, or a float, which becomes
    ``Fraction(f).limit_denominator(1001)`` (29.97 -> 2997/100, 23.976 -> 2997/125, 30000 / 1001 stays itself).  A string is "NUM/DEN" or
    a float, as the command line gives it.  Anything non-finite or <= 0 raises ValueError."""
    if isinstance(value, str):
        num, _, den = value.partition("/")
        try:
            value = (int(num), int(den)) if den else float(num)
        except ValueError:
            raise ValueError(f"a frame rate is a number or NUM/DEN, got {value!r}") from None
    if isinstance(value, tuple) and len(value) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in value):
        if value[1] == 0:
            raise ValueError(f"a frame rate must be finite, got {value}")
        rate = Fraction(int(value[0]), int(value[1]))
    elif isinstance(value, bool):
        raise ValueError(f"a frame rate is a number, got {value!r}")
    elif isinstance(value, (int, np.integer, Fraction)):
        rate = Fraction(value)
    elif isinstance(value, (float, np.floating)):
        if not np.isfinite(value):
            raise ValueError(f"a frame rate must be finite, got {value}")
        rate = Fraction(float(value)).limit_denominator(1001)
    else:
        raise ValueError(f"a frame rate is an int, a Fraction, a (num, den) tuple or a float, got {value!r}")
    if rate <= 0:
        raise ValueError(f"a frame rate must be > 0, got {value}")
    return rate


def frame_rates(fps, num_tracks):
    """``predict_tracks``' ``fps`` / ``out_fps`` -> one ``Fraction`` per track.  One rate for all tracks (see ``frame_rate``; a tuple of two
    integers is ONE rate num / den) or a list / array with one rate per track."""
    if isinstance(fps, (list, np.ndarray)) or (isinstance(fps, tuple) and not (len(fps) == 2 and all(isinstance(v, (int, np.integer)) for v in fps))):
        if len(fps) != num_tracks:
            raise ValueError(f"fps must be one rate or one per track: {num_tracks} tracks, {len(fps)} rates")
        return [frame_rate(v) for v in fps]
    return [frame_rate(fps)] * num_tracks


def _rate_argument(text):
    """--fps / --out_fps: "NUM/DEN" or a float -> the exact rate."""
    try:
        return frame_rate(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def resample_plan(lens, fps, model_fps=50):
    """Where the frames of the model's time grid lie in tracks filmed at another rate -> (model_lens, left, right, weight); exact integer
    arithmetic in numpy and Python integers, nothing touches a device.

    A track of T source frames at rate f becomes ``T' = ceil((T - 1) * model_fps / f) + 1`` model frames (``model_lens``); model frame k
    sits at source position ``p_k = k * f / model_fps``.  ``left`` / ``right`` (sum(model_lens),) int64: the two source frames around it
    as GLOBAL source rows (all tracks back to back), ``weight`` float64 = p_k - floor(p_k), one division of two integers below 2^53.
    weight == 0 has right == left; a position at or behind the last source frame (only a track's final model frame can be) repeats it:
    left == right == T - 1, weight 0.  ``fps``: as ``frame_rates``; ``model_fps``: one rate."""
    lens = np.asarray(lens, np.int64).reshape(-1)
    if (lens < 1).any():
        raise ValueError("every track needs at least one frame")
    rates, mf = frame_rates(fps, len(lens)), frame_rate(model_fps)
    model_lens, left, right, weight = [], [], [], []
    start = 0
    for T, f in zip((int(n) for n in lens), rates):
        step = f / mf                                                  # source frames per model frame, exact
        N, D = step.numerator, step.denominator
        span = (T - 1) * D
        Tm = -(-span // N) + 1                                         # ceil((T - 1) * model_fps / f) + 1
        if max(Tm * N, D) >= 2 ** 53:
            raise ValueError(f"a track of {T} frames at {f} fps: the plan's integers must stay below 2^53")
        pos = np.arange(Tm, dtype=np.int64) * N
        l, rem = pos // D, pos % D
        rem[l >= T - 1] = 0
        l = np.minimum(l, T - 1)
        model_lens.append(Tm)
        left.append(start + l)
        right.append(start + l + (rem > 0))
        weight.append(rem / np.float64(D))
        start += T
    return np.array(model_lens, np.int64), np.concatenate(left), np.concatenate(right), np.concatenate(weight)


def output_positions(lens, fps, out_fps, model_fps=50):
    """The model positions of the frames ``predict_tracks(fps=..., out_fps=...)`` returns -> (out_lens, (track, num, den)) for
    ``evaluation.keyframe_plan_at``: a track of T frames at rate f has ``floor((T - 1) * out_fps / f) + 1`` output frames, frame i at time
    i / out_fps, which is model position ``i * model_fps / out_fps`` (never behind the last model frame of ``resample_plan``)."""
    lens = np.asarray(lens, np.int64).reshape(-1)
    rates, outs, mf = frame_rates(fps, len(lens)), frame_rates(out_fps, len(lens)), frame_rate(model_fps)
    out_lens, track, num, den = [], [], [], []
    for t, (T, f, o) in enumerate(zip((int(n) for n in lens), rates, outs)):
        n = ((T - 1) * o.numerator * f.denominator) // (o.denominator * f.numerator) + 1
        q = mf / o
        if max(n * q.numerator, q.denominator) >= 2 ** 53:
            raise ValueError(f"a track of {T} frames at {f} fps returned at {o} fps: the plan's integers must stay below 2^53")
        out_lens.append(n)
        track.append(np.full(n, t, np.int64))
        num.append(np.arange(n, dtype=np.int64) * q.numerator)
        den.append(np.full(n, q.denominator, np.int64))
    return np.array(out_lens, np.int64), (np.concatenate(track), np.concatenate(num), np.concatenate(den))


def given_positions(out_lens, steps=None):
    """Where the frames a call returns lie among the frames it was GIVEN, for the root trajectory of ``predict_tracks(camera=...)`` ->
    (track, num, den) int64 arrays, one entry per returned frame: frame i of track t sits at given-frame position i * steps[t] = num / den.
    ``steps``: None (a returned frame is a given frame: the plain call, ``fps`` alone) or one exact rate per track as ``frame_rates`` takes
    them -- ``Fraction(1, s_in)`` with ``keyframes_only``, ``fps / out_fps`` with an output rate."""
    out_lens = np.asarray(out_lens, np.int64).reshape(-1)
    steps = [Fraction(1)] * len(out_lens) if steps is None else frame_rates(steps, len(out_lens))
    track, num, den = [], [], []
    for t, (n, q) in enumerate(zip((int(n) for n in out_lens), steps)):
        if max(n * q.numerator, q.denominator) >= 2 ** 53:
            raise ValueError(f"track {t}: {n} returned frames {q} given frames apart: the positions' integers must stay below 2^53")
        track.append(np.full(n, t, np.int64))
        num.append(np.arange(n, dtype=np.int64) * q.numerator)
        den.append(np.full(n, q.denominator, np.int64))
    return np.concatenate(track), np.concatenate(num), np.concatenate(den)


def root_plan(given, positions=None):
    """The host plan of uu3d_root_trajectory -> (base, wnum, wden) int64 arrays, one entry per returned frame: ``base`` the GLOBAL row (all
    tracks' given frames back to back) of the given frame at or before the position, ``wnum / wden`` the fraction behind it, 0 <= wnum <
    wden.  ``given``: given frames per track; ``positions``: (track, num, den) of ``given_positions`` (None: every given frame itself).
    Exact integer arithmetic.  ValueError: a position whose whole part lies behind its track's last given frame, or a track's given
    frames times a denominator reaching 2^53 -- the weight's two integers, (base - L) wden + wnum and (R - L) wden, stay below it."""
    given = np.asarray(given, np.int64).reshape(-1)
    if (given < 1).any():
        raise ValueError("every track needs at least one given frame")
    start = np.concatenate([[0], np.cumsum(given)[:-1]])
    if positions is None:
        rows = np.arange(int(given.sum()), dtype=np.int64)
        return rows, np.zeros_like(rows), np.ones_like(rows)
    track, num, den = (np.asarray(a, np.int64).reshape(-1) for a in positions)
    if not (len(track) == len(num) == len(den)) or (track < 0).any() or (track >= len(given)).any() or (den < 1).any() or (num < 0).any():
        raise ValueError("positions must be (track, num, den) with one entry per returned frame, num >= 0 and den >= 1")
    if ((given[track].astype(object) * den.astype(object)) >= 2 ** 53).any():
        raise ValueError("given frames times a position's denominator must stay below 2^53")
    floor = num // den
    if (floor >= given[track]).any():
        raise ValueError("a returned frame lies behind its track's last given frame")
    return start[track] + floor, num - floor * den, den


def default_mask_stride(config):
    """The mask stride a call takes when none is given: the config's first MASK_STRIDE (None: the config has none)."""
    return config.MASK_STRIDE[0] if isinstance(config.MASK_STRIDE, (list, tuple)) else config.MASK_STRIDE


def session_strides(config, mask_stride=None):
    """(SEQUENCE_STRIDE, input stride s_in, prediction stride) of a session: ``mask_stride`` defaults to the config's first MASK_STRIDE (no
    mask stride at all: every sampled frame is input); a pose comes out for centres that are multiples of the prediction stride."""
    cfg = config.copy()
    if mask_stride is None:
        mask_stride = default_mask_stride(cfg)
    cfg.MASK_STRIDE = mask_stride
    S = int(cfg.SEQUENCE_STRIDE)
    s_in = S if mask_stride is None else int(mask_stride)
    if s_in < S or s_in % S != 0:
        raise ValueError("the mask stride must be a multiple of the sequence stride")
    return S, s_in, int(ev.prediction_stride(cfg) or 1)


def max_lookahead(config):
    return (int(config.SEQUENCE_LENGTH) // 2) * int(config.SEQUENCE_STRIDE)


def keyframe_bracket(num, den, P):
    """The bracket rule, on Python ints and on int64 arrays alike: model position u = num / den between keyframes P model frames apart ->
    (k0, k1, off, den_w): k0 = floor(u / P) P, k1 = k0 where u == k0, else k0 + P; the weight of k1 is off / den_w =
    (num - k0 den) / (P den), for the caller to divide once in float64.  The device reads a pose by the same rule (keyframe_read,
    csrc/uu3d_stream_rate.h)."""
    k0 = num // den // P * P
    off = num - k0 * den
    return k0, k0 + P * (off != 0), off, P * den


def newest_model_frame(j, A, B):
    """K(j) = floor(j A / B): the newest model frame after a slot's j-th push (0-based)."""
    return (j * A) // B


def _fraction_lcm(*values):
    """The smallest positive Fraction that is a whole multiple of every given one: lcm of the numerators over gcd of the denominators."""
    return Fraction(math.lcm(*(v.numerator for v in values)), math.gcd(*(v.denominator for v in values)))


def _output_ring_depth(A, B, c, d, un, ud, P, lookahead, a_m, period):
    """D for a session with an output rate, by exact enumeration in numpy int64 over the pushes q + lookahead, q = 0 .. period (one common
    period of source frames, output frames and keyframes, and the push that closes it): the push returns output frames i_lo .. i_hi,
    the newest emitted centre is ((K(q + lookahead) - a_m) // P) P; the oldest k0 read is k0(i_lo), the newest k1 read is k1(i_hi).
    -> (D, the smallest newest centre - k1(i_hi): >= 0 means every keyframe read has been emitted)."""
    q = np.arange(period + 1, dtype=np.int64)
    hi = q * c // d
    lo = np.where(q == 0, 0, (q - 1) * c // d + 1)
    due = hi >= lo
    newest = (newest_model_frame(q + lookahead, A, B) - a_m) // P * P
    k0_lo, k1_hi = keyframe_bracket(lo * un, ud, P)[0], keyframe_bracket(hi * un, ud, P)[1]
    return 1 + int(((newest - k0_lo) // P)[due].max()), int((newest - k1_hi)[due].min())


def _output_reads_cubic(A, B, c, d, un, ud, P, period):
    """What the pushes q + lookahead, q = 0 .. period, of a cubic session with an output rate read, in numpy int64 -> (due, oldest,
    newest): a mixed output frame (off != 0) reads keyframes k0 - P .. k0 + 2 P, one on a keyframe k0 alone.  Of the frames i_lo .. i_hi
    of a push the oldest read is that of i_lo or of i_lo + 1 (a mixed frame just behind a keyframe), the newest that of i_hi or of
    i_hi - 1.  ``oldest`` is not clamped at 0: the one-sided first segment reads less, and the value is the one a period later."""
    q = np.arange(period + 1, dtype=np.int64)
    hi = q * c // d
    lo = np.where(q == 0, 0, (q - 1) * c // d + 1)
    due = hi >= lo

    def reads(i):
        k0, _, off, _ = keyframe_bracket(i * un, ud, P)
        mixed = off != 0
        return k0 - P * mixed, k0 + 2 * P * mixed
    oldest = np.minimum(reads(lo)[0], reads(np.minimum(lo + 1, hi))[0])
    newest = np.maximum(reads(hi)[1], reads(np.maximum(hi - 1, lo))[1])
    return due, oldest, newest


RatePlan = collections.namedtuple("RatePlan", "A B n_max a_m D min_lookahead pred_stride lookahead out_c out_d pos_num pos_den max_out",
                                  defaults=(None, None, None, None, None))


def _rate_plan_cubic(config, fps, lookahead, A, B, P, keys, out):
    """``rate_plan(interpolation="cubic")`` behind its checks.  ``keys``: ``keyframe_bracket`` of the source frames of one period B P;
    ``out``: () or (c, d, un, ud, R, common period) of the output rate."""
    if out:
        due, oldest, need = _output_reads_cubic(A, B, *out[:4], P, out[5])
        pushes = np.arange(out[5] + 1, dtype=np.int64)
        oldest, need, pushes = oldest[due], need[due], pushes[due]
    else:                                                             # (a mixed pose reads k0 - P .. k1 + P = k0 + 2 P, a keyframe k0 alone)
        oldest = np.array([k[0] - P * (k[2] != 0) for k in keys], np.int64)
        need = np.array([k[1] + P * (k[2] != 0) for k in keys], np.int64)
        pushes = np.arange(len(keys), dtype=np.int64)

    def slack(L):                                                      # min over one period of K(q + L) - the newest keyframe read
        return int((newest_model_frame(pushes + L, A, B) - need).min())
    min_lookahead = 0
    while slack(min_lookahead) < 0:
        min_lookahead += 1
    lookahead = min_lookahead if lookahead is None else int(lookahead)
    if lookahead < min_lookahead:
        raise ValueError(f"lookahead {lookahead} is too small at {frame_rate(fps)} fps with interpolation=\"cubic\": a pose between two model "
                         f"keyframes {P} model frames apart is read from the cubic through four of them, one behind the pair, and the "
                         f"cubic's minimum is a lookahead of at least {min_lookahead} source frames")
    a_m = min(max_lookahead(config), slack(lookahead))
    newest = (newest_model_frame(pushes + lookahead, A, B) - a_m) // P * P
    if int((newest - need).min()) < 0:
        raise AssertionError("a pose due at a push reads a keyframe that has not been emitted")
    D = 1 + int(((newest - oldest) // P).max())
    if D > 4096:
        raise ValueError(f"lookahead {lookahead} would keep {D} keyframes per slot; at most 4096")
    return RatePlan(A, B, -(-A // B), a_m, D, min_lookahead, P, lookahead, *out[:5])


def rate_plan(config, fps, lookahead, mask_stride=None, model_fps=50, out_fps=None, interpolation="linear"):
    """The plan of ``StreamSession(fps=fps, lookahead=lookahead)`` -> RatePlan(A, B, n_max, a_m, D, min_lookahead, pred_stride, lookahead,
    ...); integers and ``Fraction`` only.  A / B = model_fps / fps in lowest terms; n_max = ceil(A / B), the most model frames one push makes;
    a_m the model lookahead and D the places of the keyframe ring (``stream``'s module docstring), both by exact enumeration over one
    period B P of j; min_lookahead the smallest ``lookahead`` (in source frames) for which an a_m >= 0 exists.  A smaller ``lookahead``
    raises ValueError naming it; ``lookahead=None`` plans for min_lookahead itself.
    ``out_fps=G`` (None: the five further fields are None and the others are what they were): out_c / out_d = G / fps and
    pos_num / pos_den = model_fps / G in lowest terms, max_out = R = ceil(G / fps) poses per push at most.  a_m and min_lookahead are
    unchanged -- an output frame due at a push is never later than the push's source frame q -- and D is enumerated over one common
    period of the source frames, the output frames and the keyframes (an lcm of Fractions), the oldest output frame of every push
    included; the enumeration also checks the claim about a_m.  ValueError, naming the quantity: more than 2^24 source frames per
    period, a term of out_fps / fps or of model_fps / out_fps >= 2^20, more than 64 poses per push.
    ``interpolation="cubic"`` (``StreamSession(interpolation="cubic")``; "linear": everything above, unchanged): a pose between two
    keyframes is read from the C1 cubic through FOUR of them, k0 - P (none in a slot's first segment), k0, k1 and k1 + P
    (``evaluation.interpolate_cubic_host``); a pose on a keyframe still reads k0 alone.  Two requirements change, both enumerated the same
    way.  The newest emitted centre must reach k1 + P wherever the position is not a keyframe: min_lookahead and a_m come from that slack
    -- without ``out_fps`` over the source frames of one period B P, with it over the output frames of every push of one common period,
    because an output frame just in front of a source frame that sits on a keyframe needs the keyframe behind it (the ValueError names
    the new minimum as the cubic's).  And the ring keeps k0 - P of the oldest pose a push reads: D is one deeper wherever that read
    decides it.  The fields are the same; the session remembers the interpolation itself."""
    from .options import check_interpolation                       # (options imports the stage modules, which import this one)
    cubic = check_interpolation(interpolation) == "cubic"
    rho = frame_rate(model_fps) / frame_rate(fps)
    A, B = rho.numerator, rho.denominator
    if max(A, B) >= 2 ** 20:
        raise ValueError(f"model_fps / fps = {A}/{B}: numerator and denominator must stay below 2^20")
    _, _, P = session_strides(config, mask_stride)
    out = ()
    if out_fps is not None:
        up, pos = frame_rate(out_fps) / frame_rate(fps), frame_rate(model_fps) / frame_rate(out_fps)
        c, d, un, ud = up.numerator, up.denominator, pos.numerator, pos.denominator
        if max(c, d) >= 2 ** 20:
            raise ValueError(f"out_fps / fps = {c}/{d}: numerator and denominator must stay below 2^20")
        if max(un, ud) >= 2 ** 20:
            raise ValueError(f"model_fps / out_fps = {un}/{ud}: numerator and denominator must stay below 2^20")
        R = -(-c // d)
        if R > 64:
            raise ValueError(f"out_fps / fps = {c}/{d} would return up to {R} poses per push; at most 64")
        span = _fraction_lcm(1 / frame_rate(fps), 1 / frame_rate(out_fps), P / frame_rate(model_fps)) * frame_rate(fps)
        assert span.denominator == 1
        if span > 2 ** 24:
            raise ValueError(f"fps {frame_rate(fps)}, out_fps {frame_rate(out_fps)} and keyframes {P} model frames apart repeat only after {int(span)} "
                             f"source frames per period; at most 2^24")
        out = (c, d, un, ud, R, int(span))
    period = B * P
    keys = [keyframe_bracket(q * A, B, P) for q in range(period)]
    if cubic:
        return _rate_plan_cubic(config, fps, lookahead, A, B, P, keys, out)

    def slack(L):                                                      # min over one period of K(q + L) - k1(q)
        return min(newest_model_frame(q + L, A, B) - k[1] for q, k in enumerate(keys))
    min_lookahead = 0
    while slack(min_lookahead) < 0:
        min_lookahead += 1
    lookahead = min_lookahead if lookahead is None else int(lookahead)
    if lookahead < min_lookahead:
        raise ValueError(f"lookahead {lookahead} is too small at {frame_rate(fps)} fps: the pose of a source frame is read between two model "
                         f"keyframes {P} model frames apart, which needs a lookahead of at least {min_lookahead} source frames")
    a_m = min(max_lookahead(config), slack(lookahead))
    if out:
        D, spare = _output_ring_depth(A, B, *out[:4], P, lookahead, a_m, out[5])
        if spare < 0:
            raise AssertionError("an output frame due at a push reads a keyframe that has not been emitted")
    else:
        D = 1 + max(((newest_model_frame(q + lookahead, A, B) - a_m) // P * P - k[0]) // P for q, k in enumerate(keys))
    if D > 4096:
        raise ValueError(f"lookahead {lookahead} would keep {D} keyframes per slot; at most 4096")
    return RatePlan(A, B, -(-A // B), a_m, D, min_lookahead, P, lookahead, *out[:5])


def push_plan(j, plan):
    """The host mirror of what a slot's j-th push (0-based) does under ``plan``: {"model": [(k, left, right, weight), ...] -- the model
    frames the push makes, each with its two source frames and resample_plan's float64 weight (left == right: weight 0.0) --, "q": the
    source frame whose pose comes out (None while j < lookahead), "k0", "k1": its two keyframes, "weight": the float64 output weight}."""
    A, B, P = plan.A, plan.B, plan.pred_stride
    j = int(j)
    first = 0 if j == 0 else newest_model_frame(j - 1, A, B) + 1
    model = []
    for k in range(first, newest_model_frame(j, A, B) + 1):
        left, rem = divmod(k * B, A)
        model.append((k, left, left + (rem > 0), float(np.float64(rem) / np.float64(A))))
    q = j - plan.lookahead
    if q < 0:
        return {"model": model, "q": None, "k0": None, "k1": None, "weight": None}
    k0, k1, off, den = keyframe_bracket(q * A, B, P)
    return {"model": model, "q": q, "k0": k0, "k1": k1, "weight": float(np.float64(off) / np.float64(den))}


def out_push_plan(j, plan):
    """The host mirror of what a slot's j-th push (0-based) RETURNS under a ``plan`` with an output rate: [(i, k0, k1, weight), ...], the
    output frames that became due at the push, oldest first -- none while q = j - lookahead < 0, frame 0 alone at q == 0, then
    floor((q - 1) G / F) + 1 .. floor(q G / F); k0, k1 the two keyframes frame i is read between (k1 == k0 on a keyframe) and weight the
    float64 (i pos_num - k0 pos_den) / (P pos_den), ``keyframe_plan_at``'s."""
    if plan.max_out is None:
        raise ValueError("the plan has no output rate: rate_plan(..., out_fps=G)")
    q = int(j) - plan.lookahead
    if q < 0:
        return []
    first = 0 if q == 0 else ((q - 1) * plan.out_c) // plan.out_d + 1
    frames = []
    for i in range(first, (q * plan.out_c) // plan.out_d + 1):
        k0, k1, off, den = keyframe_bracket(i * plan.pos_num, plan.pos_den, plan.pred_stride)
        frames.append((i, k0, k1, float(np.float64(off) / np.float64(den))))
    return frames


def push_plan_cubic(j, plan):
    """``push_plan`` for a session with ``interpolation="cubic"`` (``plan``: ``rate_plan(..., interpolation="cubic")``): the same dict
    plus "before" and "after", the two outer keyframes of ``evaluation.interpolate_cubic_host`` as model frames -- k0 - P and k1 + P;
    None where there is none (before: the slot's first segment, k0 == 0) and wherever k0 == k1 (a keyframe's own bits, or no pose yet)."""
    pp = push_plan(j, plan)
    P = plan.pred_stride
    mixed = pp["q"] is not None and pp["k0"] != pp["k1"]
    pp["before"] = pp["k0"] - P if mixed and pp["k0"] >= P else None
    pp["after"] = pp["k1"] + P if mixed else None
    return pp


def out_push_plan_cubic(j, plan):
    """``out_push_plan`` for a session with ``interpolation="cubic"``: [(i, before, k0, k1, after, weight), ...] -- ``out_push_plan``'s
    frames with the two outer keyframes as in ``push_plan_cubic``."""
    P = plan.pred_stride
    return [(i, k0 - P if k0 != k1 and k0 >= P else None, k0, k1, k1 + P if k0 != k1 else None, w) for i, k0, k1, w in out_push_plan(j, plan)]
