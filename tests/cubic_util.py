"""Shared by test_cubic_cpu and test_cubic_gpu: the track table the cubic plans are checked on, and the plan restated as a plain loop over
the frames of one track at a time.  A plain module: nothing here is collected."""
from fractions import Fraction

import numpy as np

STRIDE = 5
# 1, 1, 2, 2, 3, 4 and 6 keyframes at stride 5, with and without frames behind the last one; the last: 4 keyframes and one frame behind
TRACK_LENS = [1, 5, 6, 10, 11, 16, 26, 3 * STRIDE + 2]                     # 92 frames, 21 keyframes
# the steps between returned frames, in model frames: fps=30 at a 50 Hz model, out_fps=50 (every model frame), out_fps=100
STEPS = {"fps30": Fraction(5, 3), "out_fps50": Fraction(1), "out_fps100": Fraction(1, 2)}


def frame_indices(lens=TRACK_LENS):
    return np.concatenate([np.arange(n) for n in lens])


def positions_at(step, lens=TRACK_LENS):
    """(video, num, den) of ``evaluation.keyframe_plan_at``: track v is read at 0, step, 2 step, ... up to its last frame."""
    video, num, den = [], [], []
    for v, n in enumerate(lens):
        count = int((n - 1) / step) + 1
        video += [v] * count
        num += [i * step.numerator for i in range(count)]
        den += [step.denominator] * count
    return np.array(video, np.int64), np.array(num, np.int64), np.array(den, np.int64)


def loop_plan(lens=TRACK_LENS, stride=STRIDE, positions=None):
    """(before, left, right, after, weight) as places in ``frame_indices(lens)``, one track at a time and one frame at a time.
    ``positions`` None: every frame of every track."""
    first = np.concatenate([[0], np.cumsum(lens)])
    if positions is None:
        positions = (np.repeat(np.arange(len(lens)), lens), frame_indices(lens), np.ones(int(np.sum(lens)), np.int64))
    out = []
    for v, num, den in zip(*(a.tolist() for a in positions)):
        n, o = lens[v], int(first[v])
        p, frac = num // den, num % den
        L = p // stride * stride                                      # the keyframe at or before the position
        N = L + stride
        if frac == 0 and p == L:                                      # a keyframe
            out.append((-1, o + p, o + p, -1, 0.0))
        elif N > n - 1:                                               # behind the track's last keyframe
            out.append((-1, o + L, o + L, -1, 0.0))
        else:
            before = o + L - stride if L - stride >= 0 else -1
            after = o + N + stride if N + stride <= n - 1 else -1
            assert (before == -1 or first[v] <= before) and (after == -1 or after < first[v + 1])      # (never a neighbouring track's)
            out.append((before, o + L, o + N, after, ((p - L) * den + frac) / (stride * den)))
    b, l, r, a, w = zip(*out)
    return tuple(np.array(x, np.int64) for x in (b, l, r, a)) + (np.array(w, np.float64),)


def key_rows(lens=TRACK_LENS, stride=STRIDE):
    """Only keyframes are forwarded -> (rows: place -> row of the predictions or -1, the number of predictions)."""
    f = frame_indices(lens)
    run = np.flatnonzero(f % stride == 0)
    rows = np.full(len(f), -1, np.int64)
    rows[run] = np.arange(len(run))
    return rows, len(run)


def to_rows(plan, rows):
    before, left, right, after, weight = plan
    return (np.where(before >= 0, rows[np.maximum(before, 0)], -1), rows[left], rows[right], np.where(after >= 0, rows[np.maximum(after, 0)], -1),
            weight)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
