"""GPU: stream.StreamSession -- one 3D pose per pushed frame -- against its one rule, the truncation identity: the pose emitted after the
push that made frame t the newest is the pose predict_tracks (and the CPU oracle pipeline) gives for frame t - lookahead of the track cut
to its first t + 1 frames.  Three slots, flip on, pixel tracks at three resolutions, seeded weights."""
import numpy as np
import pytest

from tests import util
from tests.tracks_util import RES, _bits, _model, _oracle_poses, _pixel_tracks, _run

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
T = 3


def _checked_ticks(L, a, S, cap, s_in):
    """About a dozen fresh ticks: the first, ticks while the window still hangs over the start, the ticks right after the ring wrapped
    (once and twice around), some in the middle, the last fresh one."""
    fresh = [t for t in range(L) if t - a >= 0 and (t - a) % S == 0]
    after = lambda f: next(t for t in fresh if t >= f)
    pick = {fresh[0], fresh[1], fresh[4], fresh[len(fresh) // 4], after(cap * s_in), after(cap * s_in + 1), after(2 * cap * s_in),
            after(2 * cap * s_in + s_in), fresh[len(fresh) // 2], fresh[-7], fresh[-2], fresh[-1]}
    return sorted(pick)


@pytest.mark.parametrize("cfgname,ms,L,a", [("h36m_81", 4, 260, 0), ("h36m_81", 4, 260, 7), ("h36m_351", 5, 420, 0), ("h36m_351", 5, 420, 13),
                                            ("h36m_351", 10, 420, 0), ("h36m_351", 10, 420, 13)])
def test_truncation_identity(cfgname, ms, L, a):
    from uplift_upsample_3dhpe_amd import h36m, predict, stream
    cfg, arch, w, model = _model(cfgname)
    S, N = cfg.SEQUENCE_STRIDE, cfg.SEQUENCE_LENGTH
    assert a == 0 or a % S != 0                                         # (a lookahead that is no multiple of the sequence stride)
    tracks = _pixel_tracks([L] * T, seed=11)
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=a)
    assert s.ring_capacity * ms < L // 2                                 # the ring wraps at least twice
    poses, fresh = _run(s, tracks, L)
    assert s.check_range() is False                                     # a clean range word after the run
    assert s.frames.cpu().tolist() == [L] * T and s.captures == 1
    # fresh equals the rule at every tick; a slot that is not fresh returns its previous pose bit for bit (zeros before its first)
    rule = np.array([stream.emits(t + 1, a, cfg, ms) for t in range(L)])
    assert np.array_equal(rule, np.array([t - a >= 0 and (t - a) % S == 0 for t in range(L)]))
    assert np.array_equal(fresh, np.repeat(rule[:, None], T, 1))
    prev = np.concatenate([np.zeros_like(poses[:1]), poses[:-1]], 0)
    assert np.array_equal(_bits(poses[~rule]), _bits(prev[~rule])) and not poses[:a].any()
    assert np.isfinite(poses).all() and not poses[:, :, cfg.ROOT_KEYTPOINT].any()
    # the checked ticks: truncated tracks through ONE predict_tracks call and through the oracle pipeline
    ticks = _checked_ticks(L, a, S, s.ring_capacity, ms)
    assert 9 <= len(ticks) <= 12
    cut = [tracks[i][:t + 1] for t in ticks for i in range(T)]
    res = [RES[i] for t in ticks for i in range(T)]
    centres = np.array([t - a for t in ticks for i in range(T)])
    got = np.stack([poses[t, i] for t in ticks for i in range(T)])
    full = predict.predict_tracks(model, cfg, cut, resolutions=res, mask_stride=ms, flip=True)
    want = np.stack([full[k][c].cpu().numpy() for k, c in enumerate(centres)])
    norm = [h36m.normalize_screen_coordinates(t_, w=r[0], h=r[1]).astype(np.float32) for t_, r in zip(cut, res)]
    orc = _oracle_poses(cfg, arch, w, norm, centres, ms)
    d_pred, d_orc = np.abs(got - want).reshape(len(ticks), -1).max(1), np.abs(got - orc).reshape(len(ticks), -1).max(1)
    print(f"{cfgname} s_in {ms} lookahead {a}: ticks {ticks}")
    print(f"  max-abs to predict_tracks on the truncated track {d_pred.max():.3e}, to the oracle pipeline {d_orc.max():.3e} (bar {util.TOL_MAX_ABS})")
    assert d_pred.max() <= util.TOL_MAX_ABS and d_orc.max() <= util.TOL_MAX_ABS
    assert float(np.abs(want).max()) > 1e-3                             # (poses, not zeros)
    s.close()


def test_no_cross_talk_between_slots():
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    L = 120
    a_tracks, b_tracks = _pixel_tracks([L] * T, seed=21), _pixel_tracks([L] * T, seed=22)
    b_tracks[1] = a_tracks[1]
    out = []
    for tr in (a_tracks, b_tracks):
        s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=4, flip=True, lookahead=3)
        out.append(_run(s, tr, L))
        s.close()
    (pa, fa), (pb, fb) = out
    assert np.array_equal(fa, fb) and fa.any()
    assert np.array_equal(_bits(pa[:, 1]), _bits(pb[:, 1]))              # slot 1: the same bits at every tick
    assert not np.array_equal(_bits(pa[:, 0]), _bits(pb[:, 0])) and not np.array_equal(_bits(pa[:, 2]), _bits(pb[:, 2]))


def test_staggered_starts_and_reset():
    """Slot 2 turns active at tick 37; slot 0 is reset at tick 90 and starts a new track.  Every track equals itself pushed alone from
    tick 0 into a fresh session of the same shape whose other slots are inactive."""
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    ticks, start2, reset0 = 140, 37, 90
    tracks = _pixel_tracks([ticks] * T, seed=31)
    new = lambda: stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=4, flip=True, lookahead=5)
    s = new()

    def before(k, used):
        if k == reset0:
            s.reset([0])
    poses, fresh = _run(s, tracks, ticks, active=lambda k: [True, True, k >= start2], before_tick=before)
    assert s.frames.cpu().tolist() == [ticks - reset0, ticks, ticks - start2]
    assert not fresh[:start2, 2].any() and not poses[:start2, 2].any()
    s.close()
    # (slot, first tick, ticks, first frame of the slot's track)
    for slot, t0, n, f0 in ((0, 0, reset0, 0), (0, reset0, ticks - reset0, reset0), (1, 0, ticks, 0), (2, start2, ticks - start2, 0)):
        alone = new()
        tr = [None] * T
        tr[slot] = tracks[slot][f0:f0 + n]
        p, f = _run(alone, tr, n, active=lambda k: [i == slot for i in range(T)])
        alone.close()
        assert np.array_equal(f[:, slot], fresh[t0:t0 + n, slot]) and f[:, slot].sum() > 10 and not f[:, [i for i in range(T) if i != slot]].any()
        d = float(np.abs(p[:, slot] - poses[t0:t0 + n, slot]).max())
        same = np.array_equal(_bits(p[:, slot]), _bits(poses[t0:t0 + n, slot]))
        print(f"slot {slot} ticks {t0}..{t0 + n}: max-abs to the track pushed alone {d:.3e} (bar {util.TOL_MAX_ABS}), same bits: {same}")
        assert d <= util.TOL_MAX_ABS


def test_graph_and_repeatability():
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_351")
    L = 150
    tracks = _pixel_tracks([L] * T, seed=41)
    runs = []
    for graph in (True, False, True):
        s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=10, flip=True, lookahead=13, graph=graph)
        runs.append(_run(s, tracks, L))
        assert s.captures == (1 if graph else 0)                         # captured once, whatever the number of ticks
        assert s.check_range() is False
        s.close()
    for p, f in runs[1:]:
        assert np.array_equal(f, runs[0][1]) and np.array_equal(_bits(p), _bits(runs[0][0]))
    assert runs[0][1].sum() == T * len(range(13, L, 5))


def test_push_never_waits_for_the_device():
    """push and reset under torch's sync debug mode "error": host input (through pinned memory), device input, an active mask -- no host
    synchronisation, no copy to the host; with the graph and without."""
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    tracks = _pixel_tracks([12] * T, seed=51)
    host = np.stack([t[0] for t in tracks])
    dev = torch.from_numpy(np.stack([t[1] for t in tracks])).cuda()
    for graph in (True, False):
        s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=4, flip=True, graph=graph)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            s.push(host)
            s.push(dev)
            s.push(torch.from_numpy(host), active=[True, False, True])
            s.reset([1])
            poses, fresh = s.push(host, active=np.array([False, True, True]))
            s.reset()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert poses.is_cuda and tuple(poses.shape) == (T, 17, 3) and poses.dtype == torch.float32
        assert fresh.is_cuda and fresh.dtype == torch.bool and fresh.cpu().tolist() == [False, True, False]     # slot 1: frame 0 of its new track; slot 2: frame 3
        assert s.frames.cpu().tolist() == [0, 0, 0] and bool(torch.isfinite(poses).all())
        assert s.check_range() is False
        s.close()
