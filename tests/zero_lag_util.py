"""Shared helpers of the zero-lag One-Euro tests (test_smooth_zero_lag_cpu, test_smooth_zero_lag_gpu): the input with every awkward row and
the definition of the two-pass filter as a composition of causal calls.  A plain module: nothing here is collected."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def signal(rows, channels, seed):
    """Slow sines of different amplitudes with noise on them, float32: every channel moves, so beta matters."""
    rng = np.random.default_rng(seed)
    t = np.arange(rows, dtype=np.float64)[:, None]
    return (np.sin(t * rng.uniform(0.02, 0.3, channels) + rng.uniform(0, 6, channels)) * rng.uniform(0.1, 3.0, channels)
            + 0.05 * rng.normal(size=(rows, channels))).astype(np.float32)


def hard_input(lens, channels, seed, long=3):
    """Tracks of ``lens`` rows back to back -> (x (G, channels) float32, state (G,) uint8).  Track ``long`` (40 rows or more) has NaN / Inf
    samples at its first row, its last row and in its middle, and state zeros at its first row, its last row and a run in the middle; the
    3-row track at index 2 has a state zero at its first row; the LAST track has no usable row (state zeros throughout)."""
    starts = np.concatenate([[0], np.cumsum(lens)])
    x = signal(int(starts[-1]), channels, seed)
    a, b = int(starts[long]), int(starts[long + 1])
    x[a, 0] = np.nan
    x[b - 1, 1 % channels] = np.inf
    x[a + 17, 2 % channels] = -np.inf
    x[a + 18, 0] = np.nan
    state = np.ones(len(x), np.uint8)
    state[[a, b - 1]] = 0                                             # (with state those rows' NaN / Inf is passed through twice over)
    state[a + 9:a + 13] = 0
    state[int(starts[2])] = 0
    state[int(starts[-2]):] = 0
    return x, state


def composition(x, lens, rates, filt, state=None):
    """The definition: per track reverse(one_euro_host(reverse(one_euro_host(x)))) with the CAUSAL filter of ``filt``'s three numbers, the
    state bytes reversed with the rows."""
    from uplift_upsample_3dhpe_amd import predict
    causal = predict.OneEuro(*filt)
    assert causal.zero_lag is False
    out = np.empty_like(x)
    first = 0
    for n, r in zip(lens, rates):
        rows = slice(first, first + n)
        st = None if state is None else state[rows]
        y = predict.one_euro_host(x[rows], None, r, causal, state=st)
        back = predict.one_euro_host(y[::-1].copy(), None, r, causal, state=None if st is None else st[::-1].copy())
        out[rows] = back[::-1]
        first += n
    return out
