"""GPU: stream.StreamSession(fps=F) -- one source frame in, one pose out, resampled on the device -- against what it is defined to be: a
plain session at the model lookahead a_m fed the model-rate frames of predict.resampled_pose_table, read between its keyframes by
evaluation.keyframe_plan_at's rule.  Three slots, flip on, pixel tracks at three resolutions, seeded weights."""
import math

import numpy as np
import pytest

from tests import util
from tests.tracks_util import RES, _bits, _model, _model_rate_frames, _pixel_tracks, _plain_keyframes, _run

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
T, J = 3, 17


def _expected(plan, keys, j):
    """What push j must return for all slots, from the plain session's keyframes: (pose, exact) -- exact: a keyframe's own bits."""
    from uplift_upsample_3dhpe_amd import stream
    pp = stream.push_plan(j, plan)
    if pp["k0"] == pp["k1"]:
        return keys[pp["k0"]], True
    a, b, w = keys[pp["k0"]].astype(np.float64), keys[pp["k1"]].astype(np.float64), np.float64(pp["weight"])
    return (a * (1.0 - w) + b * w).astype(np.float32), False


@pytest.mark.parametrize("cfgname,ms,fps,extra", [("h36m_81", 4, 25, 3), ("h36m_81", 4, 24, 2), ("h36m_351", 5, 30, 4), ("h36m_351", 10, 60, 1),
                                                  ("h36m_81", 4, 29.97, 5)])
def test_identity_with_the_plain_session(cfgname, ms, fps, extra):
    """At least 150 source frames, and as many as the ring needs to wrap twice (h36m_351's ring spans more than 175 model frames, so its
    cases take more than 260 source frames).  Keyframe outputs: the plain session's bits.  Interpolated outputs: float32(a (1 - w) + b w)
    from float64 numpy, within ONE float32 ulp -- the device rounds once, and a float64 contraction in front of that rounding can move the
    float32 result by at most one ulp."""
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model(cfgname)
    L = stream.rate_plan(cfg, fps, None, ms).min_lookahead + extra
    plan = stream.rate_plan(cfg, fps, L, ms)
    cap = stream.ring_capacity(cfg, ms, plan.a_m)
    n_src = max(150, math.ceil((2 * cap * ms + 12) * plan.B / plan.A))
    n_model = (n_src - 1) * plan.A // plan.B + 1
    tracks = _pixel_tracks([n_src] * T, seed=61)
    keys, plain_cap = _plain_keyframes(model, cfg, ms, plan.a_m, _model_rate_frames(tracks, fps, n_model), with_capacity=True)
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=L, fps=fps)
    assert s.rate == plan and s.model_lookahead == plan.a_m and s.ring_capacity == plain_cap == cap
    assert s.ring_capacity * ms < n_model // 2                            # the ring wraps at least twice
    poses, fresh = _run(s, tracks, n_src)
    assert s.check_range() is False
    assert s.source_frames.cpu().tolist() == [n_src] * T and s.frames.cpu().tolist() == [n_model] * T and s.captures == 1
    s.close()
    rule = np.arange(n_src) >= L
    assert np.array_equal(fresh, np.repeat(rule[:, None], T, 1)) and not poses[:L].any()
    assert np.isfinite(poses).all() and not poses[:, :, cfg.ROOT_KEYTPOINT].any()
    exact = mixed = 0
    worst = 0.0
    for j in range(L, n_src):
        want, is_key = _expected(plan, keys, j)
        if is_key:
            exact += 1
            assert np.array_equal(_bits(poses[j]), _bits(want)), j
        else:
            mixed += 1
            ulp = np.spacing(np.abs(want))
            worst = max(worst, float((np.abs(poses[j].astype(np.float64) - want.astype(np.float64)) / ulp).max()))
            assert (np.abs(poses[j].astype(np.float64) - want.astype(np.float64)) <= ulp).all(), j
    print(f"{cfgname} s_in {ms} at {fps} fps, lookahead {L} (a_m {plan.a_m}, D {plan.D}): {n_src} pushes, {n_model} model frames, "
          f"{exact} keyframe outputs bit-identical, {mixed} interpolated within {worst:.2f} ulp")
    # (29.97 fps = 2997/100: A = 5000, so only source frame 0 sits on a keyframe within these pushes; 25 fps on P = 2: every frame does)
    assert exact >= (1 if fps == 29.97 else 5) and (mixed > 0 or (fps == 25 and cfgname == "h36m_81"))


def _oracle_poses(cfg, arch, w, norm_tracks, centres, ms):
    """The CPU oracle as the model: the window of frame ``centres[k]`` of track k by the sequence generator (stride masks aligned globally,
    the config's padding), flip as a second call, averaged; root-relative."""
    from oracle import uplift_oracle as O
    from uplift_upsample_3dhpe_amd.data import PoseTable, SequenceGenerator
    c = cfg.copy(); c.MASK_STRIDE = ms
    gen = SequenceGenerator(PoseTable(norm_tracks), seq_len=c.SEQUENCE_LENGTH, subsample=1, stride=c.SEQUENCE_STRIDE, padding_type=c.PADDING_TYPE,
                            flip_augment=False, mask_stride=ms, stride_mask_align_global=True, shuffle=False)
    desc = gen.descriptors()
    starts = np.concatenate([[0], np.cumsum([len(t) for t in norm_tracks])[:-1]])
    run = starts + np.asarray(centres)
    assert np.array_equal(desc[run, 0], np.arange(len(norm_tracks))) and np.array_equal(desc[run, 1], centres)
    b = gen.gather(desc[run], zero_masked=False, with_3d=False)
    x, m = b["kp2d"].cpu().numpy(), b["stride_mask"].cpu().numpy().astype(bool)
    _, cen = O.eval_step_with_flip(util.hp_from_arch(arch), w, x, m, c.AUGM_FLIP_KEYPOINT_ORDER)
    cen = np.asarray(cen, np.float64)
    return cen - cen[:, c.ROOT_KEYTPOINT:c.ROOT_KEYTPOINT + 1]


def _resample_f64(track, res, plan, n_model):
    """The model-rate frames on the host: normalised in float32 as h36m does, mixed in float64, rounded to float32."""
    from uplift_upsample_3dhpe_amd import h36m
    norm = h36m.normalize_screen_coordinates(track, w=res[0], h=res[1]).astype(np.float32).astype(np.float64)
    out = np.zeros((n_model, J, 2), np.float32)
    for k in range(n_model):
        left, rem = divmod(k * plan.B, plan.A)
        wgt = np.float64(rem) / np.float64(plan.A)
        out[k] = norm[left] if rem == 0 else norm[left] * (1.0 - wgt) + norm[left + 1] * wgt
    return out


@pytest.mark.parametrize("cfgname,ms,fps,want_last", [("h36m_351", 5, 30, True), ("h36m_81", 4, 24, False)])
def test_against_predict_tracks_and_the_oracle(cfgname, ms, fps, want_last):
    """A keyframe c can be read back where some source frame q sits exactly on it (q A / B == c): at 30 fps on h36m_351 (A / B = 5 / 3,
    P = 5) every keyframe, at 24 fps on h36m_81 (25 / 12, P = 2) every 25th.  Keyframe c is emitted in the sub-tick that makes model frame
    t = c + a_m, at push j_e = ceil(t B / A).  Where that sub-tick is the push's last one (at 30 fps and P = 5 always: a_m % 5 is 0, 1 or
    3) the reference is predict_tracks(fps=F, out_fps=50) on the SOURCE track cut to j_e + 1 frames; else (the 24 fps case, by the choice
    of the lookahead) predict_tracks on the MODEL-rate track cut to t + 1 frames; and always the CPU oracle on the float64-resampled cut
    track.  (The source cut gives predict_tracks one more model frame where j_e A / B is fractional: a clamped copy of the last source
    frame at index t + 1.  No window token reads it and copy padding does not repeat it unless (a_m + 1) % SEQUENCE_STRIDE == 0, which
    the chosen lookahead avoids.)"""
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg, arch, w, model = _model(cfgname)
    S = cfg.SEQUENCE_STRIDE
    lo = stream.rate_plan(cfg, fps, None, ms).min_lookahead
    last_of = lambda pl, t: t == (-(-t * pl.B // pl.A) * pl.A) // pl.B     # model frame t is the last one its push makes
    n_src = 260

    def observable(pl):
        n_model = (n_src - 1) * pl.A // pl.B + 1
        return [c for c in range(0, n_model, pl.pred_stride) if (c * pl.B) % pl.A == 0 and c * pl.B // pl.A + pl.lookahead < n_src]
    L = next(la for la in range(lo + (4 if want_last else 0), lo + 40) for pl in [stream.rate_plan(cfg, fps, la, ms)]
             if all(last_of(pl, c + pl.a_m) == want_last for c in observable(pl)) and (not want_last or (pl.a_m + 1) % S != 0))
    plan = stream.rate_plan(cfg, fps, L, ms)
    A, B, a_m = plan.A, plan.B, plan.a_m
    tracks = _pixel_tracks([n_src] * T, seed=71)
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=L, fps=fps)
    cap = s.ring_capacity
    poses, fresh = _run(s, tracks, n_src)
    assert s.check_range() is False
    s.close()
    obs = observable(plan)
    after = lambda f: next(c for c in obs if c >= f)
    centres = obs if len(obs) <= 11 else sorted({obs[0], obs[1], obs[4], after(cap * ms), after(2 * cap * ms), obs[-8], obs[-2], obs[-1]})
    assert 8 <= len(centres) <= 11 and centres[-1] > 2 * cap * ms
    cut, res, cs, got, norm = [], [], [], [], []
    for c in centres:
        t = c + a_m
        j_e = -(-t * B // A)
        assert last_of(plan, t) == want_last and j_e < n_src
        j_o = c * B // A + L                                             # the push whose output is keyframe c
        assert stream.push_plan(j_o, plan)["k0"] == stream.push_plan(j_o, plan)["k1"] == c and fresh[j_o].all()
        rate_frames = _model_rate_frames([tr[:j_e + 1] for tr in tracks], fps, t + 1) if not want_last else None
        for i in range(T):
            cut.append(tracks[i][:j_e + 1] if want_last else rate_frames[i])
            res.append(RES[i])
            cs.append(c)
            got.append(poses[j_o, i])
            norm.append(_resample_f64(tracks[i][:j_e + 1], RES[i], plan, t + 1))
    if want_last:
        full = predict.predict_tracks(model, cfg, cut, resolutions=res, mask_stride=ms, flip=True, fps=fps, out_fps=50)
    else:
        full = predict.predict_tracks(model, cfg, cut, resolutions=None, mask_stride=ms, flip=True)
    want = np.stack([full[k][c].cpu().numpy() for k, c in enumerate(cs)])
    orc = _oracle_poses(cfg, arch, w, norm, np.array(cs), ms)
    got = np.stack(got)
    d_pred, d_orc = float(np.abs(got - want).max()), float(np.abs(got - orc).max())
    print(f"{cfgname} at {fps} fps, lookahead {L} (a_m {a_m}), keyframes {centres} emitted at a push's {'last' if want_last else 'earlier'} sub-tick:")
    print(f"  max-abs to predict_tracks on the cut track {d_pred:.3e}, to the oracle pipeline {d_orc:.3e} (bar {util.TOL_MAX_ABS})")
    assert d_pred <= util.TOL_MAX_ABS and d_orc <= util.TOL_MAX_ABS
    assert float(np.abs(want).max()) > 1e-3                             # (poses, not zeros)


def test_extra_replays_are_no_ops_and_device_active_works():
    """h36m_81 at 24 fps (2 or 3 model frames per push, ceil(A / B) = 3), slot 1 pausing: ``active`` as host arrays (exact replays), as
    device tensors (3 replays per push), and without the graph -- the same bits."""
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    n = 120
    tracks = _pixel_tracks([n] * T, seed=81)
    active = lambda k: [True, not 30 <= k < 37, k % 11 != 5]
    runs = []
    for kw in ({}, {"device_active": True}, {"graph": False}):
        s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=4, flip=True, lookahead=4, fps=24, graph=kw.get("graph", True))
        assert s.rate.n_max == 3
        runs.append(_run(s, tracks, n, active=active, device_active=kw.get("device_active", False)))
        assert s.captures == (1 if kw.get("graph", True) else 0) and s.check_range() is False
        counts = s.source_frames.cpu().tolist()
        assert counts == [sum(active(k)[i] for k in range(n)) for i in range(T)]
        assert s.frames.cpu().tolist() == [(c - 1) * 25 // 12 + 1 for c in counts]
        s.close()
    assert runs[0][1].sum() > 300
    for p, f in runs[1:]:
        assert np.array_equal(f, runs[0][1]) and np.array_equal(_bits(p), _bits(runs[0][0]))


def test_staggered_slots_and_reset():
    """h36m_81 at 30 fps: slot 2 starts at push 23, slot 1 pauses for pushes 50 .. 56, slot 0 is reset at push 71.  Every slot's outputs
    equal, bit for bit, those of a session in which its track runs alone in the same slot."""
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    ticks, start2, reset0 = 130, 23, 71
    pause1 = lambda k: 50 <= k < 57
    tracks = _pixel_tracks([ticks] * T, seed=91)
    new = lambda: stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=4, flip=True, lookahead=5, fps=30)
    s = new()

    def before(k, used):
        if k == reset0:
            s.reset([0])
    poses, fresh = _run(s, tracks, ticks, active=lambda k: [True, not pause1(k), k >= start2], before_tick=before)
    assert s.source_frames.cpu().tolist() == [ticks - reset0, ticks - 7, ticks - start2] and s.check_range() is False
    s.close()
    assert not fresh[:start2, 2].any() and not poses[:start2, 2].any() and not fresh[50:57, 1].any()
    assert np.array_equal(_bits(poses[50:57, 1]), _bits(np.repeat(poses[49:50, 1], 7, 0)))      # paused: the previous pose is held
    # (slot, its pushes in the joint run, first frame of the slot's track)
    for slot, when, f0 in ((0, range(0, reset0), 0), (0, range(reset0, ticks), reset0), (1, [k for k in range(ticks) if not pause1(k)], 0),
                           (2, range(start2, ticks), 0)):
        when = list(when)
        alone = new()
        tr = [None] * T
        tr[slot] = tracks[slot][f0:f0 + len(when)]
        p, f = _run(alone, tr, len(when), active=lambda k: [i == slot for i in range(T)])
        alone.close()
        assert np.array_equal(f[:, slot], fresh[when, slot]) and f[:, slot].sum() > 30 and not f[:, [i for i in range(T) if i != slot]].any()
        assert np.array_equal(_bits(p[:, slot]), _bits(poses[when, slot])), slot


def test_missed_detections_at_30_fps():
    """h36m_351 at 30 fps with NaN rows and explicit flags per SOURCE frame: at keyframes the bits of the plain session with
    missed_detections=True fed the resampled frames and uu3d_resample_tracks' resampled validity; the coordinates of a source frame that is
    flagged missing change no output bit."""
    from uplift_upsample_3dhpe_amd import stream
    cfgname, ms, fps = "h36m_351", 5, 30
    cfg, arch, w, model = _model(cfgname)
    L = stream.rate_plan(cfg, fps, None, ms).min_lookahead + 2
    plan = stream.rate_plan(cfg, fps, L, ms)
    n_src = 240
    n_model = (n_src - 1) * plan.A // plan.B + 1
    tracks = _pixel_tracks([n_src] * T, seed=101)
    rng = np.random.default_rng(102)
    flags = [rng.uniform(size=n_src) > 0.15 for _ in range(T)]
    for i in range(T):
        flags[i][[0, 3 + i]] = [i != 1, False]                           # (slot 1 starts on a missing frame; multiples of 3 are whole positions)
        tracks[i][rng.choice(n_src, 12, replace=False), rng.integers(0, J, 12), 0] = np.nan      # missing by the finite test alone
    frames, model_valid = _model_rate_frames(tracks, fps, n_model, valid=[f.astype(np.uint8) for f in flags])
    assert all(0.3 < v.mean() < 0.95 for v in model_valid)
    keys = _plain_keyframes(model, cfg, ms, plan.a_m, frames, valid=model_valid)
    outs = []
    for variant in range(2):
        tr = [t.copy() for t in tracks]
        if variant:
            for i in range(T):
                tr[i][~flags[i]] = rng.uniform(-5000.0, 5000.0, size=tr[i][~flags[i]].shape).astype(np.float32)
        s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=L, fps=fps, missed_detections=True)
        outs.append(_run(s, tr, n_src, valid=flags))
        assert s.check_range() is False and s.frames.cpu().tolist() == [n_model] * T
        s.close()
    poses, fresh = outs[0]
    assert np.array_equal(fresh, np.repeat((np.arange(n_src) >= L)[:, None], T, 1)) and np.isfinite(poses).all()
    exact = 0
    for j in range(L, n_src):
        want, is_key = _expected(plan, keys, j)
        if is_key:
            exact += 1
            assert np.array_equal(_bits(poses[j]), _bits(want)), j
        else:
            assert (np.abs(poses[j].astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all(), j
    assert exact >= 40
    assert np.array_equal(outs[1][1], fresh) and np.array_equal(_bits(outs[1][0]), _bits(poses))


def test_fps_none_and_fps_50():
    """fps=None: the bits of a session built without the argument, the same buffers.  fps=50 at lookahead a = 2 P - 1: the sub-ticks run at
    a_m = a - (P - 1), and because floor(a / P) == floor(a_m / P) the window of keyframe c holds the same frames and the same padding
    either way -- so at the pushes where the plain session at lookahead a is fresh, the fps session returns the plain session's bits."""
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    n, ms = 90, 4
    P = stream.session_strides(cfg, ms)[2]
    a = 2 * P - 1
    tracks = _pixel_tracks([n] * T, seed=111)
    runs = {}
    for name, kw in (("plain", {}), ("none", {"fps": None}), ("fifty", {"fps": 50})):
        s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=a, **kw)
        if name != "fifty":
            assert s.rate is None and s._emit_out is s._out and s._tick_active is s._active and s.source_frames is s.frames
        else:
            assert s.rate.a_m == a - (P - 1) and a // P == s.rate.a_m // P
        runs[name] = _run(s, tracks, n)
        assert s.captures == 1 and s.check_range() is False and s.frames.cpu().tolist() == [n] * T
        s.close()
    (pp, pf), (np_, nf), (fp, ff) = runs["plain"], runs["none"], runs["fifty"]
    assert np.array_equal(pf, nf) and np.array_equal(_bits(pp), _bits(np_))
    assert pf[:, 0].sum() == len(range(a, n, P)) and ff[a:].all() and not ff[:a].any()
    assert np.array_equal(_bits(fp[pf]), _bits(pp[pf]))
    assert not np.array_equal(_bits(fp[~pf & ff]), _bits(pp[~pf & ff]))   # (in between the fps session interpolates, the plain one holds)
