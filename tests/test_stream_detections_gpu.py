"""GPU: live per-frame detections, StreamSession(detections=D) (include/uu3d.h, PER-FRAME DETECTIONS), on the scripted scene of
tests/detections_util.py with h36m_81 and seeded weights.
  1. at every tick assignment, track_ids and dropped equal row t of predict.associate_host, and poses and fresh equal, bit for bit, those
     of a second StreamSession(missed_detections=True) driven from the mirror: reset(born), then push(kp2d, active=alive, valid=matched)
     -- graph on and off, inputs on the host and on the device, once more with keypoints="coco17", repair_joints=2; captures == 1
  2. replay_detections against predict_detections by the rule of the truncation identity (the pose of frame t - lookahead is the one of
     the video cut at t)
  3. the refusals"""
import numpy as np
import pytest

from tests import detections_util as du
from tests import util
from tests.detections_util import D, FRAMES, K, RULE, S
from tests.tracks_util import _bits, _model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
_DROPPED = []


@pytest.fixture(scope="module")
def scene():
    from uplift_upsample_3dhpe_amd import predict
    dets, counts, labels = du.scene()
    rule = predict.AssociationHost(S, D, K, **RULE)
    for t in range(FRAMES):
        rule.step(dets[t], counts[t])
        _DROPPED.append(rule.dropped)
    return dets, counts, predict.associate_host(dets, counts, slots=S, **RULE)


@pytest.mark.parametrize("graph,device_inputs,options", [(True, False, {}), (False, False, {}), (True, True, {}),
                                                         (True, False, {"keypoints": "coco17", "repair_joints": 2})],
                         ids=["graph-host", "nograph-host", "graph-device", "graph-coco17-repair2"])
def test_the_session_equals_a_plain_session_driven_by_the_mirror(scene, graph, device_inputs, options):
    from uplift_upsample_3dhpe_amd import stream
    dets, counts, want = scene
    cfg, arch, w, model = _model("h36m_81")
    common = dict(resolutions=du.RESOLUTION, mask_stride=4, flip=True, lookahead=3)
    s = stream.StreamSession(model, cfg, slots=S, graph=graph, detections=D, **RULE, **common, **options)
    ref = stream.StreamSession(model, cfg, slots=S, missed_detections=True, **common, **options)
    kp, valid = du.slot_frames(dets, want, per_joint="repair_joints" in options)
    fresh_seen = 0
    try:
        assert s.missed_detections and s.captures == int(graph)
        for t in range(FRAMES):
            if device_inputs:
                p, f = s.push_detections(torch.from_numpy(dets[t]).cuda(), torch.tensor([counts[t]], dtype=torch.int32, device="cuda"))
            else:
                p, f = s.push_detections(dets[t], int(counts[t]))
            assert s.assignment.cpu().tolist() == want.assignment[t].tolist(), t
            assert s.track_ids.cpu().tolist() == want.track_ids[t].tolist(), t
            assert s.dropped.cpu().tolist() == [_DROPPED[t]], t
            if want.born[t].any():
                ref.reset(slots=np.flatnonzero(want.born[t]))
            q, g = ref.push(kp[t], active=want.alive[t] != 0, valid=valid[t])
            assert np.array_equal(f.cpu().numpy(), g.cpu().numpy()), t
            assert np.array_equal(_bits(p), _bits(q)), t
            fresh_seen += int(f.sum())
        assert s.captures == int(graph) and s.check_range() is False and fresh_seen >= 30
        assert float(np.abs(p.cpu().numpy()).max()) > 1e-3
        # reset(slots=[i]) ends track i and frees the slot; reset() clears the association state
        s.reset(slots=[1])
        assert s.track_ids.cpu().tolist()[1] == -1
        s.push_detections(dets[FRAMES - 1], int(counts[FRAMES - 1]))
        ids = s.track_ids.cpu().tolist()
        assert ids[1] == want.num_tracks and ids[0] == want.track_ids[-1][0] and ids[2] == want.track_ids[-1][2]
        s.reset()
        assert s.track_ids.cpu().tolist() == [-1] * S and s.dropped.cpu().tolist() == [0]
        s.push_detections(dets[0], int(counts[0]))
        assert s.track_ids.cpu().tolist() == want.track_ids[0].tolist() and s.assignment.cpu().tolist() == want.assignment[0].tolist()
    finally:
        s.close()
        ref.close()


def test_replay_detections_against_predict_detections(scene):
    """The rule of the truncation identity (tests/test_stream_gpu.py): the pose a session returns at tick t for a track that has a
    detection at t is the pose of frame t - lookahead of the video cut at t, within the bar of that test."""
    from uplift_upsample_3dhpe_amd import predict, stream
    dets, counts, want = scene
    cfg, arch, w, model = _model("h36m_81")
    a = 3
    common = dict(slots=S, resolutions=du.RESOLUTION, mask_stride=4, flip=True, **RULE)
    live = stream.replay_detections(model, cfg, dets, counts, lookahead=a, **common)
    assert [t[0] for t in live] == [0, 1, 2, 3] and [t[1] for t in live] == [0, 0, 0, du.C_GONE[-1] + 1]
    checked = 0
    for tick in (15, 27, 28, FRAMES - 1):
        cut = predict.predict_detections(model, cfg, [dets[:tick + 1]], [counts[:tick + 1]], **common)[0]
        for tid, first, poses in cut:
            # (the track has no detection at this tick, or its slot emits nothing at it: a slot counts the frames of ITS track)
            if first + len(poses) - 1 != tick or not stream.emits(tick - first + 1, a, cfg, 4):
                continue
            _, born, got, fresh = live[tid]
            assert born == first and fresh[tick - first]
            err = float(np.abs(got[tick - first] - poses[tick - a - first].cpu().numpy()).max())
            assert err <= util.TOL_MAX_ABS, (tick, tid, err)
            checked += 1
    assert checked >= 8


def test_refusals():
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    with pytest.raises(ValueError, match="detections together with fps / out_fps is not supported yet"):
        stream.StreamSession(model, cfg, slots=S, mask_stride=4, lookahead=40, fps=25, detections=D)
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        stream.StreamSession(model, cfg, slots=S, mask_stride=4, detections=65)
    s = stream.StreamSession(model, cfg, slots=S, mask_stride=4, detections=D)
    plain = stream.StreamSession(model, cfg, slots=S, mask_stride=4)
    try:
        with pytest.raises(ValueError, match="takes push_detections"):
            s.push(np.zeros((S, K, 2), np.float32))
        with pytest.raises(ValueError, match="needs a session built with detections=D"):
            plain.push_detections(np.zeros((D, K, 2), np.float32))
        with pytest.raises(ValueError, match="dets must be"):
            s.push_detections(np.zeros((D + 1, K, 2), np.float32))
        with pytest.raises(ValueError, match="valid must be"):
            s.push_detections(np.zeros((D, K, 2), np.float32), valid=np.ones(D + 1, bool))
        with pytest.raises(AttributeError):
            plain.track_ids
    finally:
        s.close()
        plain.close()
