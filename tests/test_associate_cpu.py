"""CPU: per-frame detections (include/uu3d.h, PER-FRAME DETECTIONS) without a GPU -- the rule in numpy (predict.associate_host) on the
scripted scene of tests/detections_util.py: every branch of the rule is really taken there (the GPU tests compare the device with this
mirror on the same scene, so they cannot pass on a scene that skips one), the prefix property, invariance under per-frame permutation,
the ids, the argument checks, the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import util
from tests import detections_util as du
from tests.detections_util import A, B, B_MINUS, B_PLUS, C as PC, D, E, FEW, FRAMES, K, MAX_AGE, RULE, S


def _stub_model(strided=True):
    class Arch(object):
        compiled_dims, num_keypoints = True, 17

    class Model(object):
        arch, has_strided_input, device = Arch(), strided, "cpu"
    return Model()


@pytest.fixture(scope="module")
def host():
    from uplift_upsample_3dhpe_amd import predict
    dets, counts, labels = du.scene()
    return dets, counts, labels, predict.associate_host(dets, counts, slots=S, **RULE)


def _row(labels, t, who):
    return int(np.flatnonzero(labels[t] == who)[0])


def test_the_scene_takes_every_branch(host):
    from uplift_upsample_3dhpe_amd import predict
    dets, counts, labels, r = host
    assert dets.shape == (FRAMES, D, K, 2) and r.assignment.shape == (FRAMES, D) and r.track_ids.shape == (FRAMES, S)
    assert np.array_equal(dets, np.round(dets * 4) / 4, equal_nan=True)           # multiples of 0.25: whole-pixel shifts are exact
    track = lambda t, who: int(r.track_of[t, _row(labels, t, who)])
    slot = lambda t, who: int(r.assignment[t, _row(labels, t, who)])
    # dropped per frame, from the state machine itself
    rule, dropped = predict.AssociationHost(S, D, K, **RULE), []
    for t in range(FRAMES):
        rule.step(dets[t], counts[t])
        dropped.append(rule.dropped)
    dropped = np.diff([0] + dropped)
    assert r.dropped == rule.dropped == int(dropped.sum())
    # two people whose paths cross keep their ids, and they do cross
    a_id, b_id = track(0, A), track(0, B)
    for t in range(FRAMES):
        if t != du.EMPTY:
            assert track(t, A) == a_id and track(t, B if t != du.TIE_FRAME else labels[t][r.track_of[t] == b_id][0]) == b_id, t
    x = lambda t, who: float(np.nanmean(dets[t, _row(labels, t, who), :, 0]))
    assert x(0, A) < x(0, B) and x(FRAMES - 1, A) > x(FRAMES - 1, B)
    # missed for max_age frames: the slot and the id are kept, the frames in between are MISSING
    c_id, c_slot = track(7, PC), slot(7, PC)
    assert len(du.C_MISSED) == MAX_AGE and track(10, PC) == c_id and slot(10, PC) == c_slot
    for t in du.C_MISSED:
        assert r.alive[t, c_slot] == 1 and r.slot_det[t, c_slot] == -1 and r.track_ids[t, c_slot] == c_id
    # missed for max_age + 1 frames: dead at the last of them; back under a new id in the lowest free slot
    assert len(du.C_GONE) == MAX_AGE + 1
    assert [int(r.alive[t, c_slot]) for t in du.C_GONE] == [1] * MAX_AGE + [0] and r.track_ids[du.C_GONE[-1], c_slot] == -1
    back = du.C_GONE[-1] + 1
    assert track(back, PC) == 3 != c_id and slot(back, PC) == c_slot == int(np.flatnonzero(r.alive[back - 1] == 0)[0]) and r.born[back, c_slot] == 1
    assert r.born.sum() == 4 and r.born[0].sum() == 3
    # a fourth person while three slots are full: dropped and counted
    for t in du.E_FRAMES:
        assert r.alive[t].all() and slot(t, E) == -1 and dropped[t] == 1
    # a frame without detections
    assert counts[du.EMPTY] == 0 and (r.assignment[du.EMPTY] == -1).all() and r.alive[du.EMPTY].all() and (r.slot_det[du.EMPTY] == -1).all()
    # a detection with min_common - 1 observed joints is ignored although a slot is free
    few = dets[du.FEW_FRAME, _row(labels, du.FEW_FRAME, FEW)]
    assert np.isfinite(few).all(axis=1).sum() == RULE["min_common"] - 1
    assert slot(du.FEW_FRAME, FEW) == -1 and not r.born[du.FEW_FRAME].any() and dropped[du.FEW_FRAME] == 0 and not r.alive[du.FEW_FRAME].all()
    # NaN joints are not in the common set: the detection is still matched
    assert np.isnan(dets[du.NAN_FRAME, _row(labels, du.NAN_FRAME, A)]).any() and track(du.NAN_FRAME, A) == a_id
    # an exact tie goes to the lower index; with the two rows exchanged the OTHER detection wins, so it is a tie
    t = du.TIE_FRAME
    lo, hi = sorted((_row(labels, t, B_PLUS), _row(labels, t, B_MINUS)))
    assert r.track_of[t, lo] == b_id and r.assignment[t, hi] == -1 and dropped[t] == 1
    dets2, counts2, labels2 = du.scene(swap_tie=True)
    r2 = predict.associate_host(dets2, counts2, slots=S, **RULE)
    assert labels2[t, lo] != labels[t, lo] and {labels2[t, lo], labels[t, lo]} == {B_PLUS, B_MINUS}
    assert r2.track_of[t, lo] == b_id and r2.assignment[t, hi] == -1
    assert sorted(np.flatnonzero(dropped).tolist()) == sorted(list(du.E_FRAMES) + [du.TIE_FRAME])
    # the rows of every frame are permuted, differently per frame; rows beyond the count are never read
    orders = {tuple(labels[t, :counts[t]]) for t in range(FRAMES) if counts[t] == 3}
    assert len(orders) >= 4
    other = dets.copy()
    for t in range(FRAMES):
        other[t, counts[t]:] = 12345.0
    r3 = predict.associate_host(other, counts, slots=S, **RULE)
    assert np.array_equal(r3.track_of, r.track_of) and np.array_equal(r3.assignment, r.assignment)


def test_prefix_property(host):
    from uplift_upsample_3dhpe_amd import predict
    dets, counts, labels, r = host
    for t in (1, 9, 10, 23, 31, FRAMES):
        p = predict.associate_host(dets[:t], counts[:t], slots=S, **RULE)
        for k in ("assignment", "track_of", "track_ids", "born", "alive", "slot_det", "slot_full"):
            assert np.array_equal(getattr(p, k), getattr(r, k)[:t]), (t, k)


def test_tracks_do_not_depend_on_the_order_of_the_rows(host):
    from uplift_upsample_3dhpe_amd import predict
    dets, counts, labels, r = host
    want = du.tracks_as_sets(labels, r.track_of)
    assert len(want) == 4
    for seed in (1, 2):
        dets2, counts2, labels2 = du.scene(seed=seed)
        assert not np.array_equal(labels2, labels) and np.array_equal(labels2[du.TIE_FRAME], labels[du.TIE_FRAME])
        r2 = predict.associate_host(dets2, counts2, slots=S, **RULE)
        assert du.tracks_as_sets(labels2, r2.track_of) == want and r2.dropped == r.dropped


def test_track_ids_are_consecutive_from_zero(host):
    from uplift_upsample_3dhpe_amd import predict
    dets, counts, labels, r = host
    ids = np.unique(r.track_of[r.track_of >= 0])
    assert ids.tolist() == list(range(r.num_tracks)) == [0, 1, 2, 3]
    first = [int(np.nonzero(r.track_of == i)[0][0]) for i in ids]
    assert first == sorted(first)                                     # handed out in the order of birth
    tracks = predict.association_tracks_host(dets, None, r)
    assert [t[0] for t in tracks] == [0, 1, 2, 3] and [t[1] for t in tracks] == first
    for tid, start, xy, flags in tracks:
        frames = np.nonzero(r.track_of == tid)[0]
        assert len(xy) == frames[-1] - frames[0] + 1 and flags[0].all() and flags[-1].all()
        assert (flags.any(axis=1) == np.isin(np.arange(start, start + len(xy)), frames)).all()


def test_flags(host):
    """(T, D) flags take a detection out; (T, D, K) flags take joints out: a detection with too few flagged joints is no candidate."""
    from uplift_upsample_3dhpe_amd import predict
    dets, counts, labels, r = host
    frame = np.ones((FRAMES, D), bool)
    frame[3, _row(labels, 3, PC)] = False
    r1 = predict.associate_host(dets, counts, valid=frame, slots=S, **RULE)
    assert r1.assignment[3, _row(labels, 3, PC)] == -1 and np.array_equal(r1.track_of[4:], r.track_of[4:])
    joint = np.ones((FRAMES, D, K), bool)
    joint[3, _row(labels, 3, PC), 2:] = False
    joint[5, _row(labels, 5, A), 4] = False
    r2 = predict.associate_host(dets, counts, valid=joint, slots=S, **RULE)
    assert r2.assignment[3, _row(labels, 3, PC)] == -1 and np.array_equal(r2.track_of[4:], r.track_of[4:])
    a_slot = r2.assignment[5, _row(labels, 5, A)]
    assert a_slot >= 0 and not r2.slot_full[5, a_slot] and r2.slot_full[6, a_slot]
    with pytest.raises(ValueError, match="valid must be"):
        predict.associate_host(dets, counts, valid=np.ones((FRAMES, D + 1), bool), slots=S)


def test_capacity_and_argument_checks():
    from uplift_upsample_3dhpe_amd import predict
    ok = np.zeros((2, 4, 17, 2), np.float32)
    for shape in ((2, 65, 17, 2), (2, 4, 65, 2)):
        with pytest.raises(ValueError, match=r"\[1, 64\]"):
            predict.associate_host(np.zeros(shape, np.float32))
    with pytest.raises(ValueError, match=r"slots must be an int in \[1, 64\]"):
        predict.associate_host(ok, slots=65)
    with pytest.raises(ValueError, match="slots"):
        predict.associate_host(ok, slots=0)
    with pytest.raises(ValueError, match=r"\(T, D, K, 2\)"):
        predict.associate_host(np.zeros((2, 4, 17), np.float32))
    with pytest.raises(ValueError, match="counts"):
        predict.associate_host(ok, counts=[1, 2, 3])
    for bad in ({"max_age": -1}, {"max_age": 1.5}, {"max_dist": -0.1}, {"max_dist": float("nan")}, {"min_common": 0}, {"min_common": True}):
        with pytest.raises(ValueError, match=list(bad)[0]):
            predict.associate_host(ok, **bad)
    assert predict.ASSOCIATION_DEFAULTS == {"max_age": 10, "max_dist": 0.5, "min_common": 3}
    r = predict.associate_host(ok)                                      # slots = D; all-zero people have no extent: never matched, born anew
    assert r.track_ids.shape == (2, 4) and r.num_tracks == 4 and r.dropped == 4


def test_symbols_and_the_c_abi_refusals():
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    for s in ("uu3d_associate_state_bytes", "uu3d_associate_reset", "uu3d_associate_detections", "uu3d_stream_associate"):
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert "typedef struct uu3d_associate_params" in header and C.sizeof(_capi.Uu3dAssociateParams) == 32
    assert lib.uu3d_associate_state_bytes(3, 17) > 0 and lib.uu3d_associate_state_bytes(3, 17) % 256 == 0
    assert lib.uu3d_associate_state_bytes(64, 64) >= 64 * 64 * 8
    assert lib.uu3d_associate_state_bytes(65, 17) == 0 and lib.uu3d_associate_state_bytes(3, 65) == 0 and lib.uu3d_associate_state_bytes(0, 17) == 0
    # capacities beyond 64: UU3D_ERR_UNSUPPORTED, before any pointer is looked at and before anything is launched
    for shape in ((65, 4, 17), (3, 65, 17), (3, 4, 65)):
        p = _capi.Uu3dAssociateParams(*shape, 2, 3, 0, 0.5)
        assert lib.uu3d_associate_reset(C.byref(p), None, None, None) == _capi.UU3D_ERR_UNSUPPORTED
        assert lib.uu3d_associate_detections(C.byref(p), None, None, None, 0, None, 1, 1, *([None] * 8)) == _capi.UU3D_ERR_UNSUPPORTED
        assert lib.uu3d_stream_associate(C.byref(p), None, None, None, None, 0, None, None, 0, *([None] * 6)) == _capi.UU3D_ERR_UNSUPPORTED
    p = _capi.Uu3dAssociateParams(3, 4, 17, 2, 3, 0, 0.5)
    assert lib.uu3d_associate_reset(C.byref(p), None, None, None) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_stream_associate(C.byref(p), None, None, None, None, 0, None, None, 0, *([None] * 6)) == _capi.UU3D_ERR_INVALID_ARGUMENT
    for bad in ((3, 4, 17, -1, 3, 0, 0.5), (3, 4, 17, 2, 0, 0, 0.5), (3, 4, 17, 2, 3, 0, -1.0)):
        assert lib.uu3d_associate_reset(C.byref(_capi.Uu3dAssociateParams(*bad)), None, None, None) == _capi.UU3D_ERR_INVALID_ARGUMENT


def test_session_and_predict_detections_argument_checks():
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg = util.load_config("h36m_81")
    new = lambda **kw: stream.StreamSession(_stub_model(), cfg, slots=kw.pop("slots", 3), mask_stride=4, **kw)
    for rate in ({"fps": 25, "lookahead": 40}, {"fps": 25, "out_fps": 50, "lookahead": 40}):
        with pytest.raises(ValueError, match="detections together with fps / out_fps is not supported yet"):
            new(detections=4, **rate)
    with pytest.raises(ValueError, match=r"detections per frame must be an int in \[1, 64\]"):
        new(detections=65)
    with pytest.raises(ValueError, match=r"slots must be an int in \[1, 64\]"):
        new(detections=4, slots=65)
    with pytest.raises(ValueError, match="detections per frame"):
        new(detections=0)
    with pytest.raises(ValueError, match="max_dist"):
        new(detections=4, max_dist=-1.0)
    with pytest.raises(ValueError, match="need detections=D"):
        new(max_age=3)
    with pytest.raises(ValueError, match="strided input"):
        stream.StreamSession(_stub_model(strided=False), cfg, slots=3, mask_stride=4, detections=4)
    with pytest.raises(TypeError, match="unexpected keyword argument 'detection'"):
        new(detection=4)
    with pytest.raises(TypeError, match="unexpected keyword argument 'detections'"):
        stream.replay_tracks(_stub_model(), cfg, [np.zeros((4, 17, 2), np.float32)], detections=4)
    # the plan: detections imply missed detections and keep the rule's parameters; without them the plan is what it was
    s = object.__new__(stream.StreamSession)
    s._init_plan(_stub_model(), cfg, 3, None, 4, True, 5, True, False, None, 50, None, detections=4, rule={"max_age": 2, "max_dist": None, "min_common": None})
    assert s.detections == 4 and s.missed_detections is True and s.association == {"max_age": 2, "max_dist": 0.5, "min_common": 3}
    s = object.__new__(stream.StreamSession)
    s._init_plan(_stub_model(), cfg, 3, None, 4, True, 5, True, False, None, 50, None)
    assert s.detections is None and s.association is None and s.missed_detections is False
    # push / push_detections refuse the other kind of session before they touch a device
    s.model = _stub_model()
    s._torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="push_detections needs a session built with detections=D"):
        s.push_detections(np.zeros((4, 17, 2), np.float32))
    s.detections = 4
    with pytest.raises(ValueError, match="takes push_detections"):
        s.push(np.zeros((3, 17, 2), np.float32))
    s._state = None                                                     # (nothing to close)
    # predict_detections
    dets = [np.zeros((5, 4, 17, 2), np.float32)]
    with pytest.raises(ValueError, match="strided input"):
        predict.predict_detections(_stub_model(strided=False), cfg, dets)
    with pytest.raises(ValueError, match="does not take keyframes_only"):
        predict.predict_detections(_stub_model(), cfg, dets, keyframes_only=True)
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        predict.predict_detections(_stub_model(), cfg, [np.zeros((5, 65, 17, 2), np.float32)])
    with pytest.raises(ValueError, match="max_age"):
        predict.predict_detections(_stub_model(), cfg, dets, max_age=-2)
