"""Live uplifting: ``StreamSession`` takes one frame of 2D keypoints per track and tick and returns one 3D pose per track, on the device.

    s = StreamSession(model, config, slots=T, resolutions=(1920, 1080), lookahead=0)
    poses, fresh = s.push(kp2d)            # (T, J, 2) host or device -> (T, J, 3) float32, (T,) bool, both on the device

The one rule (the truncation identity): after the push that made frame t the newest of a track, the session emits the pose of frame
c = t - lookahead -- when c >= 0 and ``eval.needed_windows`` keeps the window centred on c (TEST_STRIDED_EVAL: c % SEQUENCE_STRIDE == 0) --
and that pose is what ``predict.predict_tracks`` returns for frame c of the track cut to its first t + 1 frames (same ``mask_stride``,
``flip``, ``resolutions``, ``root_relative``).  Frames of the window that do not exist yet are padded by the config's PADDING_TYPE, as the
end of a video is.  On every other push the slot's previous pose is held and reported as not fresh; nothing is interpolated.

Per tick (include/uu3d.h, LIVE TRACKS): uu3d_stream_stage -> uu3d_frame_features on the ``slots`` (x 2 with flip) new
frames -> uu3d_stream_commit (counters, keyframe ring, edge row, this tick's window rows and masks) -> uu3d_forward_frames_ex from the
session's resident feature table -> uu3d_stream_emit.  The spatial stack runs once per pushed frame, not once per frame of the window.  The
per-track counters live on the device, so the five steps are ONE captured hipGraph (``graph=True``) replayed at every tick; ``push`` never
waits for the device.
All arguments are the same at every push, so the constructor decides the session's mode once and builds its launch tables (the steps of a
tick, the launches of a push around them, the reset: library functions with their prebuilt arguments); ``push`` and ``reset`` walk them.
The integer planning of rates and strides (``rate_plan``, ``push_plan``, ``out_push_plan``, ``session_strides``) is ``rates.py``.

Any frame rate -- ``StreamSession(..., fps=F, model_fps=50)``: one SOURCE frame per slot and push, at F frames per second, and one pose per
slot and push, at the source frame's own time; everything on the device, ``push`` still never waits.  With model_fps / F = A / B in lowest
terms (exact integers; ``rates.rate_plan``, ``rates.push_plan``):
  input   model frame k sits at source position k B / A (``rates.resample_plan``'s definition) and is made the moment source frame
          ceil(k B / A) has been pushed: that source frame's bits where the position is whole, else the two neighbours normalised and then
          mixed in float64 with resample_plan's own weight (the device functions of uu3d_resample_tracks).  After a slot's j-th push
          (0-based) its newest model frame is K = floor(j A / B); the push made K - floor((j - 1) A / B) model frames -- 1 at j = 0, then
          0 .. ceil(A / B).
  model   every new model frame is one tick of the plain session (a SUB-TICK: uu3d_stream_resample_stage in place of uu3d_stream_stage,
          then features, commit, forward, emit as above, then uu3d_stream_file_keyframe) at the model lookahead a_m: the session with ``fps``
          IS a plain session at lookahead a_m fed the resampled model-rate frames.
  output  ``poses[i]`` is the pose of source frame q = j - lookahead of slot i (``lookahead`` counts SOURCE frames), read at model position
          u = q A / B from the piecewise-linear motion through the emitted keyframes (centres that are multiples of the prediction stride
          P; the rule of ``evaluation.keyframe_plan_at``, as ``predict_tracks(fps=F)``): k0 = floor(u / P) P, k1 = k0 where u == k0, else
          k0 + P; u == k0 gives that keyframe's bits, anything else float32(p0 (1 - w) + p1 w) in float64, w = (q A - k0 B) / (P B).
          ``fresh[i]`` is set on EVERY push with q >= 0 of an active slot, not only at keyframes; otherwise the previous pose is held.
  a_m     the largest integer in [0, max_lookahead(config)] with k1(j - lookahead) <= floor(j A / B) - a_m for every j >= lookahead: k1 has
          been emitted when it is read.  The condition repeats in j with period B P and is enumerated exactly; when no a_m >= 0 exists
          the constructor raises ValueError naming the smallest sufficient ``lookahead``.  The emitted keyframes live per slot in a ring of
          D poses, centre c at place (c / P) % D, D - 1 = the largest distance in keyframes from the newest emitted centre back to k0.
``fps=None`` is the session above, bit for bit: the same launches, the same buffers, the same single captured graph.

Live upsampling -- ``StreamSession(..., fps=F, out_fps=G, model_fps=50)``: the session returns poses on a time grid of its own, G per second,
EVERY one that has become due per push -- a camera at 50 fps whose detector runs on every fifth frame (fps=10, out_fps=50) gets its 50
poses a second, five per push.  Input and model sides, ``lookahead`` (SOURCE frames), a_m and ``missed_detections`` as above; the rules are
``rates.output_positions``' and ``evaluation.keyframe_plan_at``'s, as ``predict_tracks(fps=F, out_fps=G)``:
  grid    output frame i of a slot lies at time i / G, model position u = i model_fps / G, and is read like a source frame above:
          k0 = floor(u / P) P; u == k0 gives that keyframe's bits, anything else float32(p0 (1 - w) + p1 w) in float64, w one float64
          division of two integers.
  push    after the push that made source frame j the newest of a slot, q = j - lookahead >= 0, the slot has emitted every output frame
          i <= floor(q G / F): the frames whose time is not later than source frame q's.  The push returns the ones that became due at it,
          oldest first -- frame 0 alone at q == 0, then floor(q G / F) - floor((q - 1) G / F): at most R = ceil(G / F) (``max_out``),
          possibly none when G < F; an inactive slot returns none.  ``push`` -> (poses (slots, R, J, 3), count (slots,) int32); rows
          r >= count[i] are zeros; ``out_frames`` counts the output frames per slot on the device.
  ring    the oldest output frame of a push lies just behind source frame q - 1, so its k0 can be one keyframe older than k0(q): D is
          enumerated over one common period of the three grids (source frames, output frames, keyframes); a_m needs no change -- no due
          frame is later than source frame q -- which the enumeration checks as well (``rate_plan``, ``out_push_plan``).
One launch (uu3d_stream_timed_emit_multi) in place of uu3d_stream_timed_emit; ``out_fps=None`` is the session above, bit for bit.

    python -m uplift_upsample_3dhpe_amd.stream --config C --weights W.h5 --input tracks.npz --output out.npz [--lookahead A] [--resolution W H]
                                                 [--mask_missing] [--fps F [--out_fps G]]
"""
import argparse
import ctypes as C
import functools
import gc

import numpy as np

from . import _capi
from ._capi import ptr as _ptr
from .predict import _load_model, check_resolutions, check_valid
from .rates import (RatePlan, _rate_argument, max_lookahead, newest_model_frame, out_push_plan, push_plan,  # noqa: F401 (re-exported)
                    rate_plan, session_strides)


def ring_capacity(config, mask_stride=None, lookahead=0):
    """Keyframes kept per slot: a window centred on newest - lookahead reads frames from (SEQUENCE_LENGTH // 2) * SEQUENCE_STRIDE before its
    centre up to the newest one -- lookahead + half span + 1 consecutive indices, at most this many multiples of s_in."""
    S, s_in, _ = session_strides(config, mask_stride)
    return (int(lookahead) + max_lookahead(config)) // s_in + 1


def emits(frames, lookahead, config, mask_stride=None):
    """Whether the push that brought a track to ``frames`` frames emits a pose (of frame ``frames - 1 - lookahead``)."""
    _, _, pred = session_strides(config, mask_stride)
    c = int(frames) - 1 - int(lookahead)
    return int(frames) >= 1 and c >= 0 and c % pred == 0


def window_plan(frames, lookahead, config, mask_stride=None, valid=None):
    """The host mirror of uu3d_stream_commit's row rule for a track of ``frames`` frames: None when no pose comes out, else a dict of (N,)
    arrays over the window centred on ``frames - 1 - lookahead`` --
        "mask": the stride mask bit; "src": the frame a real token reads (-1: none -- a masked token, or zero padding);
        "kind": 0 masked token, 1 zero row, 2 keyframe ring, 3 edge row; "place": the ring place of kind 2 (-1 otherwise)
    -- and "centre".  ``valid``: (frames,) flags, 0 = a missing frame (uu3d_stream_commit_valid): a token that reads one is masked --
    mask' = mask and (no frame is read or valid[the frame read])."""
    if not emits(frames, lookahead, config, mask_stride):
        return None
    S, s_in, _ = session_strides(config, mask_stride)
    N, L = int(config.SEQUENCE_LENGTH), int(frames)
    cap = ring_capacity(config, mask_stride, lookahead)
    pad_edge = config.PADDING_TYPE == "copy"
    c = L - 1 - int(lookahead)
    n = np.arange(N, dtype=np.int64)
    f = c - ((N - 1) * S) // 2 + n * S
    src = np.where(f < 0, f + ((-f + S - 1) // S) * S, np.where(f >= L, f - ((f - L + S) // S) * S, f))
    inside = (f >= 0) & (f < L)
    have = inside | (pad_edge & (src >= 0) & (src < L))
    mask = np.mod((n - N // 2) * S + c, s_in) == 0
    if valid is not None:
        v = np.asarray(valid).reshape(-1) != 0
        if len(v) != L:
            raise ValueError(f"valid must have one flag per frame: {L} frames, {len(v)} flags")
        mask = mask & (~have | v[np.clip(src, 0, L - 1)])
    edge_frame = (L - 1) // S * S
    kind = np.zeros(N, np.int64)
    kind[mask & ~have] = 1
    is_edge = mask & have & ~inside & (src == edge_frame)
    kind[is_edge] = 3
    ring = mask & have & ~is_edge
    if (np.mod(src[ring], s_in) != 0).any() or (src[ring] < c - (N // 2) * S).any():
        raise AssertionError("a window token reads a frame that is neither a kept keyframe nor the edge frame")
    kind[ring] = 2
    return {"centre": c, "mask": mask, "src": np.where(kind >= 2, src, -1), "kind": kind,
            "place": np.where(kind == 2, (src // s_in) % cap, -1)}


class StreamSession(object):

    def __init__(self, model, config, slots, resolutions=None, mask_stride=None, flip=None, lookahead=0, root_relative=True, graph=True,
                 missed_detections=False, fps=None, model_fps=50, out_fps=None):
        """``slots``: tracks served side by side (a slot is a track: ``reset`` starts a new one).  ``resolutions``: None = the coordinates
        are normalised already, else one (w, h) in pixels or one per slot.  ``mask_stride`` / ``flip`` / ``root_relative`` as
        ``predict.predict_tracks``.  ``lookahead`` = a: frames the answer may lag behind the newest one, 0 <= a <=
        (SEQUENCE_LENGTH // 2) * SEQUENCE_STRIDE; with a at its maximum every window is complete.  ``graph``: replay one captured hipGraph
        per tick instead of enqueueing the five steps.  Models with generic dims have no frames form: NotImplementedError.
        ``missed_detections=True``: a pushed frame may be MISSING (``push(valid=...)``, or a row with a NaN / Inf coordinate) -- the slot's
        track still grows by that frame, but no window ever shows it to the network (``predict.predict_tracks(valid=...)``); the tick runs
        uu3d_stream_stage_valid / uu3d_stream_commit_valid.  Needs a model with strided input (ValueError).  False: today's session.
        ``fps``: None = the pushed frames are at the model's rate (today's session, bit for bit).  Else the ONE rate of the session's source
        frames, parsed by ``rates.frame_rate`` (int, ``Fraction``, ``(num, den)``, or a float read as
        ``Fraction(f).limit_denominator(1001)``), against ``model_fps``: the module docstring's "Any frame rate".  ``lookahead`` then counts
        SOURCE frames and must be at least ``rate_plan(...).min_lookahead`` (ValueError naming it); ``missed_detections`` flags are per
        source frame, and a model frame is missing under uu3d_resample_tracks' rule: its left source frame is missing or, where it is mixed
        from two, its right one.  ``captures`` counts captures of the sub-tick graph: 1 for the session's whole life -- the source push and
        the timed emit around the replays are two plain launches, not captured.
        ``out_fps``: None = one pose per push, at the source frame's own time (the session above, bit for bit).  Else the rate of the poses
        the session returns, parsed like ``fps`` (which it needs: ValueError without): the module docstring's "Live upsampling".  ``push``
        then returns (poses (slots, max_out, J, 3), count (slots,) int32), ``max_out`` = ceil(out_fps / fps) <= 64, and ``out_frames``
        counts the output frames per slot."""
        res = self._init_plan(model, config, slots, resolutions, mask_stride, flip, lookahead, graph, missed_detections, fps, model_fps, out_fps)
        import torch
        self._torch = torch
        self._lib = _capi.load_library()
        layouts = self._init_layout(config, root_relative)
        with torch.cuda.device(model.device):
            self._init_buffers(config, res, *layouts)
            self._init_launch_tables()
            self._zero_features()
            if self.graph:
                self._capture()

    # ---- construction: checks and plan, layout and state, buffers, launch tables (then the capture) ---------------------------------
    def _init_plan(self, model, config, slots, resolutions, mask_stride, flip, lookahead, graph, missed_detections, fps, model_fps, out_fps):
        """Every refusal that needs no device, and the session's plan.  -> the checked resolutions."""
        slots, lookahead = int(slots), int(lookahead)
        if slots < 1:
            raise ValueError("slots >= 1")
        if out_fps is not None and fps is None:
            raise ValueError("out_fps needs fps: the rate of the pushed frames")
        S, s_in, pred = session_strides(config, mask_stride)
        self.rate = None if fps is None else rate_plan(config, fps, lookahead, mask_stride, model_fps, out_fps)
        self.max_out = None if out_fps is None else self.rate.max_out
        if self.rate is None and not 0 <= lookahead <= max_lookahead(config):
            raise ValueError(f"lookahead must be in [0, {max_lookahead(config)}] = (SEQUENCE_LENGTH // 2) * SEQUENCE_STRIDE, got {lookahead}")
        res = check_resolutions(resolutions, slots, per="slot")
        if not model.arch.compiled_dims:
            raise NotImplementedError("StreamSession needs the frames form of the forward (uu3d_frame_features / uu3d_forward_frames_ex), "
                                      "which models with generic dims do not have")
        self.missed_detections = bool(missed_detections)
        if self.missed_detections and not model.has_strided_input:
            raise ValueError("missed_detections needs a model with strided input: a missing frame becomes the learned masked token")
        self.model, self.slots, self.lookahead, self.graph = model, slots, lookahead, bool(graph)
        self.seq_stride, self.mask_stride, self.pred_stride = S, s_in, pred
        self.flip = bool(config.EVAL_FLIP) if flip is None else bool(flip)
        self.captures = 0                                             # hipGraph captures so far (graph=True: 1 for the session's whole life)
        self.model_lookahead = lookahead if self.rate is None else self.rate.a_m       # the lookahead of a (sub-)tick, in model frames
        self._key = ("stream", id(self))
        return res

    def _init_layout(self, config, root_relative):
        """The C structs of the session and the layouts of its state block -> (plain, rate, out), None where the session has no such part."""
        lib, h, r = self._lib, self.model._h, self.rate
        self._cfg = _capi.Uu3dStreamConfig(self.slots, self.seq_stride, self.mask_stride, self.pred_stride, self.model_lookahead, int(self.flip),
                                           int(config.PADDING_TYPE == "copy"), int(config.ROOT_KEYTPOINT) if root_relative else -1)
        self.model._sync_from_trainer()
        lay, rlay, olay = _capi.Uu3dStreamLayout(), None, None
        _capi.check(lib, lib.uu3d_stream_state_layout(h, C.byref(self._cfg), C.byref(lay)), h)
        self.ring_capacity = int(lay.ring_capacity)
        if r is not None:
            self._rate, rlay = _capi.Uu3dStreamRate(r.A, r.B, self.lookahead, r.D), _capi.Uu3dStreamRateLayout()
            _capi.check(lib, lib.uu3d_stream_rate_state_layout(h, C.byref(self._cfg), C.byref(self._rate), C.byref(rlay)), h)
        if self.max_out is not None:
            self._outp, olay = _capi.Uu3dStreamOut(r.out_c, r.out_d, r.pos_num, r.pos_den, r.max_out), _capi.Uu3dStreamOutLayout()
            _capi.check(lib, lib.uu3d_stream_out_state_layout(h, C.byref(self._cfg), C.byref(self._rate), C.byref(self._outp), C.byref(olay)), h)
        return lay, rlay, olay

    def _init_buffers(self, config, res, lay, rlay, olay):
        """The state block and the buffers of a tick; then what a session with missed detections, with a rate and with an output rate adds."""
        torch, lib, m = self._torch, self._lib, self.model
        a, dev = m.arch, m.device
        T, J, N, dt, H = self.slots, a.num_keypoints, a.num_frames, a.d_temporal, 2 if self.flip else 1
        zeros = functools.partial(torch.zeros, device=dev)
        self._state = zeros(int((olay or rlay or lay).bytes), dtype=torch.uint8)
        view = lambda off, n, dtype: self._state[off:off + n * 4].view(dtype)
        self._frames = view(int(lay.frames_offset), T, torch.int32)
        self._table = view(int(lay.table_offset), int(lay.table_rows) * dt, torch.float32).view(int(lay.table_rows), dt)
        self._zero_row = int(lay.zero_row)
        self._kp = zeros((T, J, 2), dtype=torch.float32)
        self._active = torch.ones((T,), dtype=torch.uint8, device=dev)
        self._active_all = True
        self._res = None if res is None else torch.from_numpy(res).pin_memory().to(dev, non_blocking=True)
        self._order = torch.from_numpy(np.ascontiguousarray(config.AUGM_FLIP_KEYPOINT_ORDER, np.int32)).to(dev) if self.flip else None
        self._staged = zeros((H * T, J, 2), dtype=torch.float32)
        self._feats = zeros((H * T, dt), dtype=torch.float32)
        self._rows = torch.full((H * T, N), -1, dtype=torch.int32, device=dev)
        self._mask = zeros((H * T, N), dtype=torch.uint8)
        self._fresh = zeros((T,), dtype=torch.uint8)
        self._full = torch.empty((H * T, N, J, 3), dtype=torch.float32, device=dev) if m._returns_full else None
        self._central = zeros((H * T, J, 3), dtype=torch.float32)
        self._out = zeros((T, J, 3), dtype=torch.float32)
        # a workspace of the session's own for uu3d_frame_features: the graph holds its address
        self._fws = torch.empty(max(int(lib.uu3d_frame_features_bytes(m._h, H * T)), int(lib.uu3d_frame_features_bytes(m._h, 1))),
                                dtype=torch.uint8, device=dev)
        # missed detections: the caller's flags of this tick, the same ANDed with active and the finite test (stage), the flags kept per slot
        self._valid_in = self._valid = self._valid_state = None
        self._valid_in_all = True
        if self.missed_detections:
            self._valid_in = torch.ones((T,), dtype=torch.uint8, device=dev)
            self._valid = zeros((T,), dtype=torch.uint8)
            self._valid_state = zeros(int(lib.uu3d_stream_valid_bytes(m._h, C.byref(self._cfg))), dtype=torch.uint8)
        # what a (sub-)tick takes as `active` and where its emit writes: with a rate the sub-ticks' own buffers, else the session's
        self._tick_active, self._emit_out, self._emit_fresh = self._active, self._out, self._fresh
        self._source_frames, self._src_host, self._src_known = self._frames, None, None
        if rlay is not None:
            self._source_frames = view(int(rlay.source_frames_offset), T, torch.int32)
            self._tick_active = zeros((T,), dtype=torch.uint8)
            self._emit_out = zeros((T, J, 3), dtype=torch.float32)
            self._emit_fresh = zeros((T,), dtype=torch.uint8)
            self._src_host = np.zeros(T, np.int64)                    # host mirror of the source counters; exact where _src_known
            self._src_known = np.ones(T, bool)
        self._result = self._out, self._fresh.view(torch.bool)        # what push returns: the session's own buffers
        if olay is not None:
            self._out_frames = view(int(olay.out_frames_offset), T, torch.int32)
            self._poses = zeros((T, self.max_out, J, 3), dtype=torch.float32)
            self._count = zeros((T,), dtype=torch.int32)
            self._result = self._poses, self._count

    def _init_launch_tables(self):
        """All arguments are the same at every push (the buffers never move), so the mode is decided here, once: every launch of the
        session as (library function, its arguments up to the stream); a step whose arguments are None is a Python callable of the stream.
          _tick_steps   the steps of one (sub-)tick, in order -- what the graph captures
          _push_before  / _push_after   the launches of a push around its sub-ticks (a session with a rate; not captured)
          _reset_call   the reset of the session's kind; the slot mask and the stream follow its arguments"""
        lib, m = self._lib, self.model
        h, cfg, state = m._h, C.byref(self._cfg), _ptr(self._state)
        kp, res, order, active, staged = _ptr(self._kp), _ptr(self._res), _ptr(self._order), _ptr(self._active), _ptr(self._staged)
        tick_active, valid, feats, rows, mask = _ptr(self._tick_active), _ptr(self._valid), _ptr(self._feats), _ptr(self._rows), _ptr(self._mask)
        emit_fresh = _ptr(self._emit_fresh)
        if self.rate is not None:
            rate = C.byref(self._rate)
            stage = (lib.uu3d_stream_resample_stage, (h, cfg, rate, state, res, order, tick_active, valid, staged))
        elif self.missed_detections:
            stage = (lib.uu3d_stream_stage_valid, (h, cfg, kp, res, active, order, _ptr(self._valid_in), valid, staged))
        else:
            stage = (lib.uu3d_stream_stage, (h, cfg, kp, res, active, order, staged))
        features = (lib.uu3d_frame_features, (h, staged, int(self._staged.shape[0]), feats, _ptr(self._fws), C.c_size_t(self._fws.numel()), 0))
        if self.missed_detections:
            commit = (lib.uu3d_stream_commit_valid, (h, cfg, state, feats, tick_active, valid, _ptr(self._valid_state), rows, mask, emit_fresh))
        else:
            commit = (lib.uu3d_stream_commit, (h, cfg, state, feats, tick_active, rows, mask, emit_fresh))
        # the latency schedule: what model.forward_frames takes (below 1024 token rows both schedules give the same bits)
        forward = (functools.partial(m._forward_frames, self._table, self._rows, self._mask if m.has_strided_input else None, self._full,
                                     self._central, self._key), None)
        emit = (lib.uu3d_stream_emit, (h, cfg, state, _ptr(self._central), order, emit_fresh, _ptr(self._emit_out)))
        self._tick_steps = [stage, features, commit, forward, emit]
        self._push_before, self._push_after = [], []
        self._reset_call = (lib.uu3d_stream_reset, (h, cfg, state))
        if self.rate is not None:
            self._tick_steps.append((lib.uu3d_stream_file_keyframe, (h, cfg, rate, state, emit_fresh)))
            self._push_before = [(lib.uu3d_stream_source_push, (h, cfg, rate, state, kp, active, _ptr(self._valid_in), int(self.missed_detections)))]
            self._push_after = [(lib.uu3d_stream_timed_emit, (h, cfg, rate, state, _ptr(self._out), _ptr(self._fresh)))]
            self._reset_call = (lib.uu3d_stream_rate_reset, (h, cfg, rate, state))
        if self.max_out is not None:
            outp = C.byref(self._outp)
            self._push_after = [(lib.uu3d_stream_timed_emit_multi, (h, cfg, rate, outp, state, _ptr(self._poses), _ptr(self._count)))]
            self._reset_call = (lib.uu3d_stream_out_reset, (h, cfg, rate, outp, state))

    # ---- the steps of a tick, on ``stream`` ------------------------------------------------------------------------------------------
    def _run(self, steps, stream):
        """Enqueue the steps of a launch table on ``stream``, in order."""
        st = C.c_void_p(stream.cuda_stream)
        for fn, args in steps:
            if args is None:
                fn(stream)
            else:
                _capi.check(self._lib, fn(*args, st), self.model._h)

    def _zero_features(self):
        """The features of an all-zero frame (zero padding) into the table's zero row."""
        torch, lib, m = self._torch, self._lib, self.model
        zero = torch.zeros((1,) + tuple(self._kp.shape[1:]), dtype=torch.float32, device=m.device)
        self._run([(lib.uu3d_frame_features, (m._h, _ptr(zero), 1, _ptr(self._table[self._zero_row:]), _ptr(self._fws),
                                              C.c_size_t(self._fws.numel()), 0))], torch.cuda.current_stream(m.device))

    def _tick(self, stream):
        self._run(self._tick_steps, stream)

    def _capture(self):
        """One warm-up tick with every slot inactive (nothing advances), then the capture: a linear chain on one stream."""
        torch = self._torch
        dev = self.model.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        gc.collect()                                                  # (a collection inside a capture may free device memory: pipeline.py)
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.stream(side):
                self._active.zero_()
                self._tick(side)
                self._active.fill_(1)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                self._tick(side)
            self._graph = g
            self.captures += 1
        finally:
            if gc_was_on:
                gc.enable()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.reset()

    # ---- public ---------------------------------------------------------------------------------------------------------------------
    def _flags(self, flags, name):
        """(slots,) flags from the host or the device -> a uint8 tensor, pinned when it is on the host."""
        torch = self._torch
        if isinstance(flags, torch.Tensor):
            f = flags.to(torch.uint8) if flags.dtype != torch.bool else flags.view(torch.uint8)
        else:
            f = torch.from_numpy(np.ascontiguousarray(np.asarray(flags) != 0).view(np.uint8))
        if tuple(f.shape) != (self.slots,):
            raise ValueError(f"{name} must be ({self.slots},)")
        return f if f.is_cuda else f.contiguous().pin_memory()

    def push(self, kp2d, active=None, valid=None):
        """One tick: ``kp2d`` (slots, J, 2), a host array or a tensor on the host or the device; ``active`` (slots,) bools or None = every slot
        (an inactive slot's row of ``kp2d`` is ignored and its track does not grow).  -> (poses (slots, J, 3) float32, fresh (slots,) bool)
        on the device: the session's own buffers, valid until the next ``push``.  ``fresh[i]``: slot i's pose is new at this tick -- the
        pose of its frame ``frames[i] - 1 - lookahead``; otherwise ``poses[i]`` is the slot's previous pose (zeros before its first).
        ``valid`` (slots,) flags or None (sessions built with ``missed_detections=True`` only): 0 = slot i's frame of this tick is MISSING, as
        is a row of ``kp2d`` with a NaN or Inf coordinate.  The slot's track grows by the frame all the same (``frames`` counts it; with
        ``active[i] == 0`` it would not) and a pose comes out by the usual rule, from windows that never read the missing frame.
        A session with ``fps``: ``kp2d`` holds one SOURCE frame per slot; ``poses[i]`` is the pose of slot i's source frame
        ``source_frames[i] - 1 - lookahead`` and ``fresh[i]`` is set at every push of an active slot once that index is >= 0.  The push
        enqueues uu3d_stream_source_push, n replays of the one sub-tick graph and uu3d_stream_timed_emit; n is the largest number of model
        frames an active slot makes at this push, known from a host mirror of the source counters.  ``active`` as a DEVICE tensor leaves the
        mirror unknown: ceil(A / B) sub-ticks are replayed per push (the surplus ones change nothing) until every such slot has been reset.
        A session with ``out_fps``: -> (poses (slots, max_out, J, 3) float32, count (slots,) int32) on the device, the session's own buffers,
        valid until the next ``push``: rows r < count[i] of slot i are the output frames that became due at this push, oldest first (the
        first is output frame ``out_frames[i] - count[i]``), rows r >= count[i] are zeros; an inactive slot has count 0.
        uu3d_stream_timed_emit_multi takes uu3d_stream_timed_emit's place.
        Enqueues on the current stream and returns; never waits for the device."""
        torch = self._torch
        m = self.model
        dev = m.device
        if valid is not None and not self.missed_detections:
            raise ValueError("push(valid=...) needs a session built with missed_detections=True")
        if m._weights_dirty or getattr(m, "_pending_assigns", False):
            m._sync_from_trainer()                                    # (weights changed: the packs are rewritten on this stream)
            with torch.cuda.device(dev):
                self._zero_features()
        if not isinstance(kp2d, torch.Tensor):
            kp2d = torch.from_numpy(np.ascontiguousarray(kp2d, np.float32))
        if tuple(kp2d.shape) != tuple(self._kp.shape):
            raise ValueError(f"kp2d must be {tuple(self._kp.shape)}, got {tuple(kp2d.shape)}")
        with torch.cuda.device(dev):
            if not kp2d.is_cuda:
                kp2d = kp2d.to(torch.float32).contiguous().pin_memory()       # host input goes through pinned memory, asynchronously
            self._kp.copy_(kp2d, non_blocking=True)
            if active is None:
                if not self._active_all:
                    self._active.fill_(1)
                    self._active_all = True
            else:
                self._active.copy_(self._flags(active, "active"), non_blocking=True)
                self._active_all = False
            if valid is not None:
                self._valid_in.copy_(self._flags(valid, "valid"), non_blocking=True)
                self._valid_in_all = False
            elif not self._valid_in_all:
                self._valid_in.fill_(1)
                self._valid_in_all = True
            cur = torch.cuda.current_stream(dev)
            self._run(self._push_before, cur)                         # (with a rate: file the source frames)
            for _ in range(self._sub_ticks(active)):                  # make the model frames that are due
                if self.graph:
                    self._graph.replay()
                else:
                    self._tick(cur)
            self._run(self._push_after, cur)                          # (with a rate: read the poses)
        return self._result

    def _sub_ticks(self, active):
        """How many (sub-)ticks this push needs, advancing the host mirror of the source counters (no rate: none, and one tick per push)."""
        if self._src_host is None:
            return 1
        torch = self._torch
        r = self.rate
        if isinstance(active, torch.Tensor) and active.is_cuda:
            self._src_known[:] = False
            return r.n_max
        act = np.ones(self.slots, bool) if active is None else np.asarray(active.numpy() if isinstance(active, torch.Tensor) else active) != 0
        n = r.n_max if (act & ~self._src_known).any() else 0
        for i in np.flatnonzero(act & self._src_known):
            j = int(self._src_host[i])
            n = max(n, 1 if j == 0 else newest_model_frame(j, r.A, r.B) - newest_model_frame(j - 1, r.A, r.B))
            self._src_host[i] = j + 1
        return n

    def reset(self, slots=None):
        """The given slots (indices; None = all) start a new track: zero frames, held pose 0, with ``out_fps`` output counter 0.  Stream-ordered
        like ``push``."""
        torch = self._torch
        m = self.model
        mask = None
        with torch.cuda.device(m.device):
            if slots is not None:
                h = np.zeros(self.slots, np.uint8)
                h[np.asarray(slots, np.int64).reshape(-1)] = 1
                mask = torch.from_numpy(h).pin_memory().to(m.device, non_blocking=True)
            fn, args = self._reset_call
            self._run([(fn, args + (_ptr(mask),))], torch.cuda.current_stream(m.device))
        self._mirror_reset(slots)

    def _mirror_reset(self, slots):
        """The host mirror of the source counters after a reset: the chosen slots are at zero, and known to be."""
        if self._src_host is None:
            return
        which = slice(None) if slots is None else np.asarray(slots, np.int64).reshape(-1)
        self._src_host[which] = 0
        self._src_known[which] = True

    @property
    def frames(self):
        """MODEL frames per slot since its last reset (without ``fps``: the frames pushed): the device counters themselves, (slots,) int32."""
        return self._frames

    @property
    def source_frames(self):
        """Source frames pushed per slot since its last reset, (slots,) int32 on the device; without ``fps`` the same tensor as ``frames``."""
        return self._source_frames

    @property
    def out_frames(self):
        """Output frames emitted per slot since its last reset (sessions with ``out_fps``), (slots,) int32 on the device."""
        if self.max_out is None:
            raise AttributeError("out_frames needs a session with out_fps")
        return self._out_frames

    def check_range(self):
        """Range guard of precision f16x3 for everything pushed so far, as ``ForwardPipeline.check_range()``: waits for the current stream,
        then raises ``Uu3dRangeError`` if a tick produced non-finite values."""
        self._torch.cuda.current_stream(self.model.device).synchronize()
        return self.model.check_range()

    def close(self):
        """Wait for what is in flight and give the session's workspace back."""
        if getattr(self, "_state", None) is not None:
            self._torch.cuda.synchronize(self.model.device)
            self._graph = None
            self.model._ws.pop(self._key, None)
            self._state = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def replay_tracks(model, config, tracks, resolutions=None, mask_stride=None, flip=None, lookahead=0, root_relative=True, graph=True, valid=None, fps=None,
                  model_fps=50, out_fps=None):
    """Push complete tracks tick by tick, one slot per track (a slot is inactive once its track has ended) -> per track the pose the
    session returned at each of its ticks, (T_i, J, 3) float32, and the fresh flags (T_i,) bool, as host arrays.  One copy to the host,
    at the end.  ``valid`` as ``predict.predict_tracks``: None, "finite" (rows with a NaN / Inf coordinate are missing frames) or one (T_i,)
    host array per track -- a session with ``missed_detections=True``.  ``fps`` / ``model_fps``: the rate of the tracks, as ``StreamSession``.
    ``out_fps=G``: -> per track the poses the session emitted, concatenated in order, (n_out_i, J, 3) float32 -- output frames
    0 .. n_out_i - 1 at G per second --, and the number each of its ticks returned, (T_i,) int32; still one copy to the host, at the end."""
    import torch
    lens = [int(len(t)) for t in tracks]
    T, ticks = len(tracks), max(lens)
    flags = None
    if valid is not None and not isinstance(valid, str):
        check_valid(valid, lens)
        flags = [np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v).reshape(-1) != 0 for v in valid]
    elif valid is not None and valid != "finite":
        raise ValueError('valid must be None, "finite" or a list with one (T_i,) array per track')
    s = StreamSession(model, config, T, resolutions=resolutions, mask_stride=mask_stride, flip=flip, lookahead=lookahead,
                      root_relative=root_relative, graph=graph, missed_detections=valid is not None, fps=fps, model_fps=model_fps, out_fps=out_fps)
    J = int(np.asarray(tracks[0]).shape[1])
    if out_fps is None:
        poses = torch.zeros((ticks, T, J, 3), dtype=torch.float32, device=model.device)
        fresh = torch.zeros((ticks, T), dtype=torch.bool, device=model.device)
    else:                                                             # one block of 32-bit words per tick and slot: the count, then the rows' bits
        R = s.max_out
        words = torch.zeros((ticks, T, 1 + R * J * 3), dtype=torch.int32, device=model.device)
    kp = np.zeros((T, J, 2), np.float32)
    try:
        for k in range(ticks):
            act = np.array([k < n for n in lens])
            for i, t in enumerate(tracks):
                if act[i]:
                    kp[i] = t[k]
            if flags is None:
                p, f = s.push(kp, None if act.all() else act)
            else:
                p, f = s.push(kp, None if act.all() else act, valid=np.array([bool(act[i]) and bool(flags[i][k]) for i in range(T)]))
            if out_fps is None:
                poses[k].copy_(p)
                fresh[k].copy_(f)
            else:
                words[k, :, 0].copy_(f)
                words[k, :, 1:].copy_(p.view(torch.int32).view(T, -1))
        s.check_range()
    finally:
        s.close()
    if out_fps is not None:
        words = words.cpu().numpy()
        counts = words[:, :, 0]
        rows = np.ascontiguousarray(words[:, :, 1:]).view(np.float32).reshape(ticks, T, R, J, 3)
        return ([np.concatenate([rows[k, i, :counts[k, i]] for k in range(n)] + [np.zeros((0, J, 3), np.float32)]) for i, n in enumerate(lens)],
                [counts[:n, i].astype(np.int32) for i, n in enumerate(lens)])
    poses, fresh = poses.cpu().numpy(), fresh.cpu().numpy()
    return [poses[:n, i] for i, n in enumerate(lens)], [fresh[:n, i] for i, n in enumerate(lens)]


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m uplift_upsample_3dhpe_amd.stream", description="Replay the 2D keypoint tracks of an .npz file (one "
                                "(T, J, 2) array per track) tick by tick through a StreamSession -> an .npz with, per track NAME, the pose returned at "
                                "every tick (NAME: (T, J, 3) float32; the pose of frame tick - lookahead where NAME_fresh is set, else the held one).")
    p.add_argument("--config", required=True, help="model config (.json)")
    p.add_argument("--weights", required=True, help="weights (.h5)")
    p.add_argument("--input", required=True, help=".npz with one (T, J, 2) array per track")
    p.add_argument("--output", required=True, help=".npz to write")
    p.add_argument("--lookahead", type=int, default=0, help="frames the answer may lag behind the newest one (default 0)")
    p.add_argument("--resolution", type=float, nargs=2, metavar=("W", "H"), default=None,
                   help="image size in pixels of all tracks; without it the coordinates are taken as normalised already")
    p.add_argument("--mask_missing", action="store_true",
                   help="a frame with a NaN or Inf coordinate is a missed detection: the track grows by it, the network never sees it")
    p.add_argument("--fps", type=_rate_argument, default=None, metavar="F",
                   help="frame rate of the tracks, a float or NUM/DEN (29.97, 30000/1001); without it they are taken at the model's rate.  "
                        "--lookahead then counts frames of the tracks")
    p.add_argument("--out_fps", type=_rate_argument, default=None, metavar="G",
                   help="rate of the poses written, a float or NUM/DEN (needs --fps): NAME then holds every pose the session emitted, in order "
                        "(n_out, J, 3), and NAME_count the number each tick returned")
    args = p.parse_args(argv)
    if args.out_fps is not None and args.fps is None:
        p.error("--out_fps needs --fps")
    return args


def main(argv=None):
    from .net.uplift_upsample_transformer_config import UpliftUpsampleConfig
    args = parse_args(argv)
    config = UpliftUpsampleConfig(args.config)
    with np.load(args.input) as z:
        names = list(z.files)
        tracks = [np.asarray(z[k], np.float32) for k in names]
    if not names:
        raise SystemExit(f"{args.input} holds no arrays")
    for k, t in zip(names, tracks):
        if t.ndim != 3 or t.shape[2] != 2 or t.shape[1] != config.NUM_KEYPOINTS or t.shape[0] < 1:
            raise SystemExit(f"{args.input}[{k}] has shape {t.shape}, expected (T >= 1, {config.NUM_KEYPOINTS}, 2)")
    if args.fps is None and not 0 <= args.lookahead <= max_lookahead(config):
        raise SystemExit(f"--lookahead must be in [0, {max_lookahead(config)}]")
    if args.fps is not None:
        try:
            rate_plan(config, args.fps, args.lookahead, out_fps=args.out_fps)
        except ValueError as e:
            raise SystemExit(f"--fps / --out_fps / --lookahead: {e}") from None
    model = _load_model(config, args.weights)
    poses, fresh = replay_tracks(model, config, tracks, resolutions=None if args.resolution is None else tuple(args.resolution),
                                 lookahead=args.lookahead, **({"valid": "finite"} if args.mask_missing else {}),
                                 **({} if args.fps is None else {"fps": args.fps}), **({} if args.out_fps is None else {"out_fps": args.out_fps}))
    out = {}
    for k, p, f in zip(names, poses, fresh):
        out[k] = np.asarray(p, np.float32)
        if args.out_fps is None:
            out[k + "_fresh"] = np.asarray(f, bool)
        else:
            out[k + "_count"] = np.asarray(f, np.int32)
    np.savez(args.output, **out)
    if args.out_fps is not None:
        print(f"wrote {args.output}: {len(names)} tracks, {sum(len(f) for f in fresh)} ticks, {sum(len(p) for p in poses)} poses at {args.out_fps} fps", flush=True)
        return 0
    print(f"wrote {args.output}: {len(names)} tracks, {sum(len(p) for p in poses)} ticks, {int(sum(f.sum() for f in fresh))} fresh poses", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
