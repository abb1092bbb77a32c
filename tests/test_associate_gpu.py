"""GPU: per-frame detections on the device (include/uu3d.h, PER-FRAME DETECTIONS).  The reference is predict.associate_host, the rule in
numpy, on the scripted scene of tests/detections_util.py (tests/test_associate_cpu.py asserts that the scene takes every branch); every
comparison is exact.
  1. associate_detections equals associate_host at every frame: one video, two videos of different lengths in one call
  2. the capacity corner S = D = K = 64: the LDS bounds and the reduction over all four waves
  3. predict_detections equals predict_tracks on the tracks and flags built from associate_host, bit for bit"""
import numpy as np
import pytest

from tests import detections_util as du
from tests.detections_util import D, K, RULE, S
from tests.tracks_util import _bits, _model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
FIELDS = ("assignment", "track_of", "track_ids", "born", "alive")


@pytest.fixture(scope="module")
def scene():
    from uplift_upsample_3dhpe_amd import predict
    dets, counts, labels = du.scene()
    return dets, counts, predict.associate_host(dets, counts, slots=S, **RULE)


def _same(got, v, want, counters):
    for k in FIELDS:
        assert np.array_equal(getattr(got, k)[v].cpu().numpy(), getattr(want, k)), (v, k)
    assert counters[v].tolist() == [want.num_tracks, want.dropped], v


def test_the_scene_equals_the_mirror(scene):
    from uplift_upsample_3dhpe_amd import predict
    dets, counts, want = scene
    got = predict.associate_detections([dets], [counts], slots=S, **RULE)
    _same(got, 0, want, got.counters.cpu().numpy())
    # two videos of different lengths in one call, one of them from the device, with tensors for the counts
    cut = 25
    got = predict.associate_detections([torch.from_numpy(dets[:cut]).cuda(), dets], [torch.from_numpy(counts[:cut]), counts], slots=S, **RULE)
    counters = got.counters.cpu().numpy()
    _same(got, 1, want, counters)
    _same(got, 0, predict.associate_host(dets[:cut], counts[:cut], slots=S, **RULE), counters)
    # per-joint and per-detection flags
    rng = np.random.default_rng(3)
    joint = rng.uniform(size=dets.shape[:3]) >= 0.2
    frame = rng.uniform(size=dets.shape[:2]) >= 0.1
    for valid in (joint, frame):
        got = predict.associate_detections([dets], [counts], valid=[valid], slots=S, **RULE)
        _same(got, 0, predict.associate_host(dets, counts, valid=valid, slots=S, **RULE), got.counters.cpu().numpy())


def test_the_capacity_corner():
    from uplift_upsample_3dhpe_amd import predict
    n, rng = 64, np.random.default_rng(64)
    body = rng.uniform(-1.0, 1.0, size=(n, 2)) * [50.0, 100.0]
    centres = rng.uniform(0.0, 4000.0, size=(n, 1, 2))
    dets = np.stack([(centres + body + rng.uniform(-5.0, 5.0, size=(n, n, 2)))[rng.permutation(n)] for _ in range(3)]).astype(np.float32)
    dets[1, 5, 7] = np.nan
    counts = np.array([64, 60, 64], np.int32)
    want = predict.associate_host(dets, counts, slots=n)
    assert want.born[0].all() and (want.assignment[1] >= 0).sum() >= 50 and want.alive[2].all()
    got = predict.associate_detections([dets], [counts], slots=n)
    _same(got, 0, want, got.counters.cpu().numpy())
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        predict.associate_detections([np.zeros((2, 65, 17, 2), np.float32)])


@pytest.mark.parametrize("options", [{}, {"keypoints": "coco17", "repair_joints": 2}], ids=["plain", "coco17-repair2"])
def test_predict_detections_equals_predict_tracks_on_the_mirror_tracks(scene, options):
    from uplift_upsample_3dhpe_amd import predict
    dets, counts, want = scene
    cfg, arch, w, model = _model("h36m_81")
    tracks = predict.association_tracks_host(dets, None, want)
    assert len(tracks) == 4 and any(not f.any(axis=1).all() for _, _, _, f in tracks) and any(np.isnan(xy).any() for _, _, xy, _ in tracks)
    got = predict.predict_detections(model, cfg, [dets], [counts], slots=S, resolutions=du.RESOLUTION, mask_stride=4, **RULE, **options)
    ref = predict.predict_tracks(model, cfg, [xy for _, _, xy, _ in tracks], valid=[f for _, _, _, f in tracks], resolutions=du.RESOLUTION,
                                 mask_stride=4, **options)
    assert len(got) == 1 and [(tid, first) for tid, first, _ in got[0]] == [(tid, first) for tid, first, _, _ in tracks]
    for (_, _, p), q in zip(got[0], ref):
        assert p.shape == q.shape and np.array_equal(_bits(p), _bits(q))
        assert float(np.abs(p.cpu().numpy()).max()) > 1e-3              # (poses, not zeros)
