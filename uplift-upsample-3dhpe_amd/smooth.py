"""The smoothing stage of the track pipeline: the One-Euro filter over the returned poses and roots (include/uu3d.h, STEADY OUTPUT).  Wraps
uu3d_one_euro_tracks (``one_euro``; the rule in numpy: ``one_euro_host``) and, for a live session, uu3d_stream_one_euro_bytes /
uu3d_stream_one_euro / uu3d_stream_one_euro_reset (``LiveOneEuro``; in numpy: ``LiveOneEuroHost``).

Steady output: the root is solved frame by frame and the poses carry the detector's frame-to-frame noise.  ``predict_tracks(...,
smooth=OneEuro(min_cutoff, beta, d_cutoff))`` passes the returned poses and roots through the One-Euro filter on the device
(uu3d_one_euro_tracks: one lane per track and channel walks the frames in order; ``one_euro`` is the launch alone; the rule in numpy:
``one_euro_host``).  The filter is causal, so the result lags as a live session's does; ``predict_detections(..., smooth=...)`` hands it on.
``OneEuro(..., zero_lag=True)`` is the offline answer to the lag (uu3d_one_euro_tracks_two_pass, still one launch): pass 1 is the causal
walk, pass 2 the same walk over pass 1's float32 rows taken last to first -- the same rate, parameters and ``state`` bytes, fresh filter
state, the first usable sample of each pass taken as given -- and the result is, per track and bit for bit,
reverse(one_euro_host(reverse(one_euro_host(x)))) with the causal filter.  On a ramp the two lags are one constant and cancel.
``zero_lag`` is OFFLINE ONLY: a session, ``replay_tracks`` / ``replay_detections`` and the live filters below refuse it (``check_causal``).

Steady output -- ``StreamSession(..., smooth=F)``: the root above is solved tick by tick and nothing ties one tick's root to the next, and
the poses carry the detector's frame-to-frame noise.  ``smooth`` -- True (the defaults), a ``predict.OneEuro(min_cutoff, beta, d_cutoff)``
for poses and roots alike, or a pair (pose_filter, root_filter), either None -- puts the One-Euro filter (Casiez, Roussel, Vogel 2012)
behind the tick, on the device: an exponential smoother whose cut-off rises with the speed of the signal, steady while a person stands,
little lag while they move (the rule: ``predict.one_euro_host``; include/uu3d.h, STEADY OUTPUT).  A channel is one coordinate of one joint
of one slot, or of its root.  Whenever an active slot's pose is fresh, each of its channels takes ONE sample at rate / n, n the frames
since the channel's previous sample (the frame counters are ``source_frames``; the rate is ``model_fps``, or ``fps`` in a session with
``fps``); a root of state 0 (zeros) is passed through and takes no sample, a held root (state 2) is a sample like any other.  A slot that
is not fresh returns the filter's last output.  ``push`` returns the filtered buffers in place of the poses and, with ``camera``, the
roots; ``raw_poses`` / ``raw_roots`` are the unfiltered ones, and uu3d_stream_root keeps solving against the unfiltered pose.  The
launches (uu3d_stream_one_euro, one per filtered buffer) are the LAST steps of the one captured tick -- with ``fps`` behind
uu3d_stream_timed_emit and the root solve, not captured --; ``push`` never waits.  ``reset`` and a birth at a ``push_detections`` tick
clear the filter with everything else.  ``LiveOneEuro`` owns the state block and the two launches and runs without a model;
``LiveOneEuroHost`` is the same state machine in numpy, and the device equals it bit for bit.  Not together with ``out_fps`` (ValueError:
several rows per push).  No accuracy or jitter figure is claimed.  ``smooth=None`` is the session above, bit for bit: no further launch
or buffer."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import ptr as _ptr
from .rates import frame_rate
from .roots import _root_lens
from .tracks import _host_array, _upload


MAX_SMOOTH_CHANNELS = 1 << 16                                         # kSmoothMaxChannels
TWO_PI = 6.283185307179586


class OneEuro(object):
    """A One-Euro filter (Casiez, Roussel, Vogel 2012): ``min_cutoff`` > 0 in Hz, the cut-off of a channel at rest; ``beta`` >= 0 in 1 / unit
    speed, how fast the cut-off rises with the channel's speed; ``d_cutoff`` > 0 in Hz, the cut-off of the speed estimate.  Anything else,
    or a non-finite value, is a ValueError.  The defaults are conveniences for metres and seconds; they are not tuned and claim nothing.
    ``zero_lag`` (keyword only, a bool; OFFLINE only): the track is filtered in two passes, forwards and then backwards over the result, so
    the two lags cancel (``one_euro_host``); ``tuple(f)`` stays the three numbers, ``==`` and ``hash`` tell the two kinds apart."""
    __slots__ = ("min_cutoff", "beta", "d_cutoff", "zero_lag")

    def __init__(self, min_cutoff=1.0, beta=0.5, d_cutoff=1.0, *, zero_lag=False):
        try:
            values = tuple(float(v) for v in (min_cutoff, beta, d_cutoff))
        except (TypeError, ValueError):
            raise ValueError(f"OneEuro takes three numbers, got {(min_cutoff, beta, d_cutoff)!r}") from None
        if not all(np.isfinite(values)) or values[0] <= 0 or values[1] < 0 or values[2] <= 0:
            raise ValueError(f"OneEuro needs finite min_cutoff > 0, beta >= 0 and d_cutoff > 0, got {values}")
        if not isinstance(zero_lag, (bool, np.bool_)):
            raise ValueError(f"OneEuro's zero_lag must be True or False, got {zero_lag!r}")
        self.min_cutoff, self.beta, self.d_cutoff = values
        self.zero_lag = bool(zero_lag)

    def __repr__(self):
        return (f"OneEuro(min_cutoff={self.min_cutoff!r}, beta={self.beta!r}, d_cutoff={self.d_cutoff!r}"
                + (", zero_lag=True)" if self.zero_lag else ")"))

    def __eq__(self, other):
        return isinstance(other, OneEuro) and tuple(self) == tuple(other) and self.zero_lag == other.zero_lag

    def __hash__(self):
        return hash(tuple(self) + (self.zero_lag,))

    def __iter__(self):
        return iter((self.min_cutoff, self.beta, self.d_cutoff))


def check_smooth(smooth, placed):
    """``smooth`` of ``predict_tracks`` / ``StreamSession`` -> (pose filter, root filter), each a ``OneEuro`` or None.  None: no filter;
    True: the defaults; a ``OneEuro``: that filter -- both for the poses and, where the call has a ``camera`` (``placed``), the roots; a
    pair (pose_filter, root_filter), either of which may be None: exactly those, and a root filter without ``camera`` is a ValueError."""
    if smooth is None or smooth is False:
        return None, None
    if smooth is True:
        smooth = OneEuro()
    if isinstance(smooth, OneEuro):
        return smooth, (smooth if placed else None)
    if isinstance(smooth, (tuple, list)) and len(smooth) == 2 and all(f is None or isinstance(f, OneEuro) for f in smooth):
        if smooth[1] is not None and not placed:
            raise ValueError("a root filter needs camera=(fx, fy, cx, cy): without it the call returns no roots")
        return smooth[0], smooth[1]
    raise ValueError(f"smooth must be None, True, a OneEuro or a pair (pose_filter, root_filter) of OneEuro / None, got {smooth!r}")


def check_causal(*filters):
    """The filters of a live session or a live filter (each a ``OneEuro`` or None): a ``zero_lag`` one is a ValueError -- its second pass
    walks a track from its last row back, and a live track has no last row yet."""
    for f in filters:
        if isinstance(f, OneEuro) and f.zero_lag:
            raise ValueError(f"live filtering is causal: {f!r} needs the whole track for its backward pass; filter the finished track "
                             "offline with predict_tracks(smooth=...) / predict_detections(smooth=...)")


def _one_euro_rates(rate, tracks):
    """``rate``: one sample rate in Hz or one per track, each as ``frame_rate`` takes it -> (tracks,) float64, each the exact rate rounded once."""
    many = isinstance(rate, (list, np.ndarray)) or (isinstance(rate, tuple) and not (len(rate) == 2 and all(isinstance(v, (int, np.integer)) for v in rate)))
    rates = [frame_rate(v) for v in rate] if many else [frame_rate(rate)] * int(tracks)
    if len(rates) != int(tracks):
        raise ValueError(f"rate must be one rate or one per track ({int(tracks)}), got {len(rates)}")
    return np.array([float(r) for r in rates], np.float64)


def one_euro_alpha(fc, r):
    """alpha(fc, r) = 1 / (1 + r / (2 pi fc)): the weight of the new sample at cut-off ``fc`` and sample rate ``r``, both in Hz (float64)."""
    return 1.0 / (1.0 + r / (TWO_PI * fc))


def one_euro_sample(x, r, filt, xh, dxh):
    """One later sample ``x`` of a channel at sample rate ``r`` -> (xh, dxh).  float64 scalars or arrays of channels alike; every operation
    is one IEEE operation, in the order written (what csrc/uu3d_smooth.h does, statement for statement)."""
    dx = (x - xh) * r
    ad = one_euro_alpha(filt.d_cutoff, r)
    dxh = ad * dx + (1.0 - ad) * dxh
    a = one_euro_alpha(filt.min_cutoff + filt.beta * np.abs(dxh), r)
    xh = a * x + (1.0 - a) * xh
    return xh, dxh


def one_euro_host(x, lens, rate, filt, state=None):
    """The rule of STEADY OUTPUT (include/uu3d.h) in numpy, written to be read: what uu3d_one_euro_tracks computes, bit for bit.
    ``x`` (G, ...) float32: the rows of all tracks back to back, everything behind the first axis is the C channels of a row; ``lens``:
    rows per track (None: one track); ``rate``: the rows' rate in Hz, one or one per track (as ``rates.frame_rate`` takes it); ``filt``: a
    ``OneEuro``; ``state``: None or (G,), 0 = the row is passed through unchanged and takes no sample (a root that was never solved)
    -> the filtered rows, float32, the shape of ``x``.
    Per channel: the first sample is returned as given; a later one moves xh towards it by ``one_euro_sample``; the output is xh rounded
    once.  A non-finite value is passed through and touches no state.  Rows are walked in a plain loop; the channels of a row are
    independent, so they go through numpy's element-wise float64 operations side by side.
    ``filt.zero_lag`` (uu3d_one_euro_tracks_two_pass): two passes per track.  Pass 1 is the walk above and yields the float32 rows y;
    pass 2 is the same walk over y with the track's rows taken last to first -- the same rate and parameters, the ``state`` bytes reversed
    with the rows, xh / dxh / taken fresh -- and its output, put back in row order, is the result: per track
    reverse(walk(reverse(walk(x)))).  A passed-through row is passed through by both passes; each pass takes its first usable sample as
    given, so a track's last usable row comes out as pass 1 left it.  On a ramp the two lags are one constant and cancel."""
    X = np.asarray(_host_array(x), np.float32)
    G = int(X.shape[0])
    flat = X.reshape(G, -1)
    if not isinstance(filt, OneEuro):
        raise ValueError(f"filt must be a OneEuro, got {filt!r}")
    lens = _root_lens(lens, G)
    rates = _one_euro_rates(rate, len(lens))
    keep = np.ones(G, bool) if state is None else np.asarray(_host_array(state)).reshape(-1) != 0
    if len(keep) != G:
        raise ValueError(f"state must be ({G},)")
    out = _one_euro_walk(flat, lens, rates, filt, keep)
    if filt.zero_lag:
        ends = np.cumsum(lens)
        back = np.concatenate([np.arange(e - 1, e - n - 1, -1) for n, e in zip(lens.tolist(), ends.tolist())] + [np.zeros(0, np.int64)]).astype(np.int64)
        out = _one_euro_walk(out[back], lens, rates, filt, keep[back])[back]      # (``back`` reverses every track in place: its own inverse)
    return out.reshape(X.shape)


def _one_euro_walk(flat, lens, rates, filt, keep):
    """One causal pass of ``one_euro_host``: ``flat`` (G, C) float32, ``keep`` (G,) bool -> (G, C) float32, a fresh array."""
    out = flat.copy()
    first = 0
    with np.errstate(all="ignore"):
        for n, r in zip(lens.tolist(), rates):
            xh = np.zeros(flat.shape[1], np.float64)
            dxh = np.zeros(flat.shape[1], np.float64)
            taken = np.zeros(flat.shape[1], bool)
            for i in range(first, first + n):
                if not keep[i]:
                    continue
                v = flat[i].astype(np.float64)
                ok = np.isfinite(v)
                nxh, ndxh = one_euro_sample(v, r, filt, xh, dxh)
                later = ok & taken
                start = ok & ~taken
                xh = np.where(later, nxh, np.where(start, v, xh))
                dxh = np.where(later, ndxh, np.where(start, 0.0, dxh))
                taken |= ok
                out[i] = np.where(ok, xh.astype(np.float32), flat[i])
            first += n
    return out


def one_euro(x, lens, rate, filt, state=None):
    """uu3d_one_euro_tracks on the current stream: ``one_euro_host`` on a device tensor, one launch, nothing copies to the host or waits
    (the per-track plan -- first row, length, rate -- is made on the host and goes up pinned and asynchronously).  ``x``: a contiguous
    (G, ...) float32 device tensor, only read; ``state``: None or a contiguous (G,) uint8 / bool device tensor
    -> the filtered rows, a fresh device tensor of ``x``'s shape.  One lane per (track, channel) walks the track's rows in order.  A
    ``filt`` with ``zero_lag`` is uu3d_one_euro_tracks_two_pass: still one launch, the same lane walks back over the rows it wrote."""
    import torch
    lib = _capi.load_library()
    if not isinstance(x, torch.Tensor) or x.dim() < 1 or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError("x must be a contiguous (G, ...) float32 device tensor")
    if not isinstance(filt, OneEuro):
        raise ValueError(f"filt must be a OneEuro, got {filt!r}")
    dev = x.device
    G = int(x.shape[0])
    Cn = int(x.numel() // G) if G else int(np.prod(x.shape[1:], dtype=np.int64))
    if not 1 <= Cn <= MAX_SMOOTH_CHANNELS:
        raise ValueError(f"a row must have 1 to {MAX_SMOOTH_CHANNELS} channels, got {Cn}")
    lens = _root_lens(lens, G)
    rates = _one_euro_rates(rate, len(lens))
    if state is not None:
        if tuple(state.shape) != (G,) or state.dtype not in (torch.uint8, torch.bool) or not state.is_contiguous() or state.device != dev:
            raise ValueError(f"state must be a contiguous ({G},) uint8 or bool tensor on x's device")
        state = state.view(torch.uint8)
    out = torch.empty_like(x)
    if G == 0:
        return out
    plan = _upload(np.stack([np.concatenate([[0], np.cumsum(lens)[:-1]]), lens]), np.int64, dev)
    d_rates = _upload(rates, np.float64, dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        launch = lib.uu3d_one_euro_tracks_two_pass if filt.zero_lag else lib.uu3d_one_euro_tracks
        _capi.check(lib, launch(_ptr(x), _ptr(out), G, Cn, _ptr(plan[0]), _ptr(plan[1]), _ptr(d_rates), len(lens), _ptr(state),
                                filt.min_cutoff, filt.beta, filt.d_cutoff, C.c_void_p(stream)), None)
    return out


def _live_filter_arguments(slots, channels, rate, filt, lookahead):
    slots, channels, lookahead = int(slots), int(channels), int(lookahead)
    if slots < 1 or not 1 <= channels <= MAX_SMOOTH_CHANNELS or lookahead < 0:
        raise ValueError(f"slots >= 1, channels in [1, {MAX_SMOOTH_CHANNELS}] and lookahead >= 0, got {slots}, {channels}, {lookahead}")
    if not isinstance(filt, OneEuro):
        raise ValueError(f"filt must be a predict.OneEuro, got {filt!r}")
    check_causal(filt)
    return slots, channels, float(frame_rate(rate)), filt, lookahead


class LiveOneEuroHost(object):
    """The rule of uu3d_stream_one_euro in numpy, written to be read: the live form of ``predict.one_euro_host``.  State per slot and
    channel -- xh, dxh (float64), ``last``: the frame index of the channel's last sample, ``taken``: whether it has taken one.
    ``step(values (slots, C) float32, frames (slots,), fresh (slots,), active (slots,) or None, state (slots,) or None)`` -> (slots, C)
    float32.  ``frames``: each slot's frame counter AFTER the push; the fresh value belongs to frame f = frames - 1 - lookahead.
      an active slot whose value is fresh (and frames >= 1): per channel one sample with n = f - last, anything below 1 counting as 1, at
          rate / n (``predict.one_euro_sample``); the first one is taken as given.  A non-finite value -- or, with ``state[slot] == 0``,
          the whole row -- is passed through unchanged and touches nothing.
      any other slot returns xh rounded once, zeros before the first sample.
    ``reset(slots=None)``: the chosen slots (None: all) have taken no sample."""

    def __init__(self, slots, channels, rate, filt, lookahead=0):
        self.slots, self.channels, self.rate, self.filt, self.lookahead = _live_filter_arguments(slots, channels, rate, filt, lookahead)
        shape = (self.slots, self.channels)
        self.xh, self.dxh = np.zeros(shape, np.float64), np.zeros(shape, np.float64)
        self.last, self.taken = np.zeros(shape, np.int64), np.zeros(shape, bool)

    def reset(self, slots=None):
        which = slice(None) if slots is None else np.asarray(slots, np.int64).reshape(-1)
        for a in (self.xh, self.dxh, self.last, self.taken):
            a[which] = 0

    def step(self, values, frames, fresh, active=None, state=None):
        values = np.asarray(values, np.float32).reshape(self.slots, self.channels)
        frames = np.asarray(frames, np.int64).reshape(self.slots)
        fresh = np.asarray(fresh).reshape(self.slots) != 0
        active = np.ones(self.slots, bool) if active is None else np.asarray(active).reshape(self.slots) != 0
        keep = np.ones(self.slots, bool) if state is None else np.asarray(state).reshape(self.slots) != 0
        out = np.zeros((self.slots, self.channels), np.float32)
        with np.errstate(all="ignore"):
            for i in range(self.slots):
                if not (active[i] and fresh[i] and frames[i] >= 1):
                    out[i] = np.where(self.taken[i], self.xh[i].astype(np.float32), np.float32(0))
                    continue
                if not keep[i]:
                    out[i] = values[i]
                    continue
                f = int(frames[i]) - 1 - self.lookahead
                x = values[i].astype(np.float64)
                ok = np.isfinite(x)
                n = np.maximum(f - self.last[i], 1)
                r = np.float64(self.rate) / n.astype(np.float64)
                nxh, ndxh = one_euro_sample(x, r, self.filt, self.xh[i], self.dxh[i])
                later, start = ok & self.taken[i], ok & ~self.taken[i]
                self.xh[i] = np.where(later, nxh, np.where(start, x, self.xh[i]))
                self.dxh[i] = np.where(later, ndxh, np.where(start, 0.0, self.dxh[i]))
                self.last[i] = np.where(ok, f, self.last[i])
                self.taken[i] |= ok
                out[i] = np.where(ok, self.xh[i].astype(np.float32), values[i])
        return out

    def drain(self, values, frames, drained, fresh, chosen=None, state=None):
        """One drain tick (``StreamSession.finish``): ``step`` at the VIRTUAL counter ``frames + drained`` -- ``frames``: the counters of the
        ended tracks, ``drained`` (slots,): the drain ticks each slot has taken, this one included --, so the fresh value belongs to frame
        f = frames - 1 - lookahead + drained; ``chosen``: the slots that drain, as ``step``'s ``active``."""
        virtual = np.asarray(frames, np.int64).reshape(self.slots) + np.asarray(drained, np.int64).reshape(self.slots)
        return self.step(values, virtual, fresh, chosen, state)


class LiveOneEuro(object):
    """The live One-Euro filter on the device: the thin owner of the state block of uu3d_stream_one_euro and of its two launches
    (``LiveOneEuroHost`` is the same state machine in numpy; the device equals it bit for bit).  ``slots`` rows of ``channels`` float32
    values each; ``rate``: the frames' rate in Hz (as ``rates.frame_rate`` takes it); ``filt``: a ``predict.OneEuro``; ``lookahead``: the
    fresh value belongs to frame frames - 1 - lookahead.  ``out``: the (slots, channels) float32 buffer every step writes.
    ``step(values, frames, fresh, active, state=None, stream=None)``: device tensors -- values (slots, channels) float32 contiguous (only
    read), frames (slots,) int32, fresh / active / state (slots,) uint8 or bool -- -> ``out``; enqueues on ``stream`` (None: the current
    one) and never waits.  ``reset(slots=None)``: the given slots (indices; None = all) have taken no sample; ``reset_mask(mask)`` takes a
    (slots,) uint8 device tensor instead.
    The interface of an output-side stage of a ``StreamSession`` (``field``: "poses" or "roots", what of a ``stream.Scene`` it filters):
    ``outputs``, ((scene field, name of the drained rows, buffer), ...): what it puts into the scene; ``read``: the scene in front of
    it, set by the session; ``launch(active, frames, drain_state=None)`` / ``reset_launch()``: the two calls as launch-table entries
    (function, arguments up to the slot mask / the stream) -- with ``drain_state`` the one of a drain tick of ``finish``."""

    def __init__(self, slots, channels, rate, filt, lookahead=0, device="cuda", field="poses"):
        import torch
        self.slots, self.channels, self.rate, self.filt, self.lookahead = _live_filter_arguments(slots, channels, rate, filt, lookahead)
        self._torch, self._lib = torch, _capi.load_library()
        self.device = torch.device(device)
        size = int(self._lib.uu3d_stream_one_euro_bytes(self.slots, self.channels))
        if size == 0:
            raise ValueError(f"slots = {self.slots}, channels = {self.channels} are out of uu3d_stream_one_euro's range")
        self._state = torch.zeros(size, dtype=torch.uint8, device=self.device)
        self.out = torch.zeros((self.slots, self.channels), dtype=torch.float32, device=self.device)
        self.field = field                                            # (a scene's (slots, J, 3) poses are (slots, 3 J) channels)
        self.outputs = ((field, "filtered_" + field, self.out.view(self.slots, -1, 3) if field == "poses" else self.out),)

    def _check(self, t, shape, dtypes, name):
        if tuple(t.shape) != shape or t.dtype not in dtypes or not t.is_contiguous() or t.device != self.out.device:
            raise ValueError(f"{name} must be a contiguous {shape} tensor of {' / '.join(str(d) for d in dtypes)} on {self.out.device}")
        return t

    def launch(self, active, frames, drain_state=None):
        read = self.read
        return self._entry(getattr(read, self.field), frames, read.fresh, active, read.root_state if self.field == "roots" else None)

    def _entry(self, values, frames, fresh, active, state=None):
        torch = self._torch
        T, flags = self.slots, (torch.uint8, torch.bool)
        if values.dim() < 1 or int(values.shape[0]) != T or values.numel() != T * self.channels:       # ((slots, J, 3) passes as (slots, 3 J))
            raise ValueError(f"values must be ({T}, {self.channels}), got {tuple(values.shape)}")
        self._check(values, tuple(values.shape), (torch.float32,), "values")
        self._check(frames, (T,), (torch.int32,), "frames")
        for t, name in ((fresh, "fresh"), (active, "active")) + (() if state is None else ((state, "state"),)):
            self._check(t, (T,), flags, name)
        f = self.filt
        return (self._lib.uu3d_stream_one_euro, (T, self.channels, self.lookahead, _ptr(self._state), _ptr(frames), _ptr(active), _ptr(fresh),
                                                 _ptr(values), _ptr(state), self.rate, f.min_cutoff, f.beta, f.d_cutoff, _ptr(self.out)))

    def reset_launch(self):
        return (self._lib.uu3d_stream_one_euro_reset, (self.slots, self.channels, _ptr(self._state)))

    def _enqueue(self, call, stream):
        torch = self._torch
        fn, args = call
        with torch.cuda.device(self.out.device):
            st = torch.cuda.current_stream(self.out.device) if stream is None else stream
            _capi.check(self._lib, fn(*args, C.c_void_p(st.cuda_stream)), None)

    def step(self, values, frames, fresh, active, state=None, stream=None):
        self._enqueue(self._entry(values, frames, fresh, active, state), stream)
        return self.out

    def reset_mask(self, mask=None, stream=None):
        fn, args = self.reset_launch()
        if mask is not None:
            self._check(mask, (self.slots,), (self._torch.uint8, self._torch.bool), "mask")
        self._enqueue((fn, args + (_ptr(mask),)), stream)

    def reset(self, slots=None, stream=None):
        torch = self._torch
        mask = None
        if slots is not None:
            h = np.zeros(self.slots, np.uint8)
            h[np.asarray(slots, np.int64).reshape(-1)] = 1
            with torch.cuda.device(self.out.device):
                mask = torch.from_numpy(h).pin_memory().to(self.out.device, non_blocking=True)
        self.reset_mask(mask, stream)
