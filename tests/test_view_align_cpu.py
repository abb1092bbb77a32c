"""CPU: the rules of ONE CLOCK in numpy (include/uu3d.h; views.py) -- the mirrors the device is held to, bit for bit, in
tests/test_view_align_gpu.py.
  1. view_lag_sums_host: the slice at lag 0 on tracks of equal length is view_pair_sums_host; a lag whose overlap is empty has no terms;
     dropping k leading frames of a track moves its profile by k, exactly
  2. view_offsets_host: the tie rule, a standing person, same_index against the unrestricted rule, the view that cannot be aligned
  3. crop_views: the windows, no copies, the refusals; every ValueError of the new calls
  4. recovery: the true offsets of the seeded scenes come back, and decisively so"""
import numpy as np
import pytest

from tests import view_align_util as AU
from tests import view_match_util as MU

L6 = 6


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. lag sums ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T, J", [(40, 5), (300, 17)])
def test_lag_zero_of_equal_tracks_is_the_pair_sum(T, J):
    from uplift_upsample_3dhpe_amd import predict
    cams, views, _, valid = MU.scene((2, 3, 1), 3, T, J, 7 * T + J)
    kp, view_of, flags = MU.stacked(views, valid)
    for fl in (flags, None):
        pair_s, pair_n = predict.view_pair_sums_host(kp, view_of, cams, fl)
        lag_s, lag_n = predict.view_lag_sums_host(list(kp), view_of, cams, None, L6, None if fl is None else list(fl))
        assert lag_s.shape == (2, 6, 2 * L6 + 1) and lag_s.dtype == np.float64 and lag_n.dtype == np.int32
        assert _bits(lag_s[:, :, L6], pair_s[:2]) and _bits(lag_n[:, :, L6], pair_n[:2]) and pair_n[:2, 2:].all()
        assert not lag_s[:, :2].any() and not lag_n[:, :2].any()         # the columns of the reference view
        flat = predict.view_lag_sums_host(kp.reshape(-1, J, 2), view_of, cams, [T] * 6, L6, None if fl is None else fl.reshape(-1, J))
        assert _bits(flat[0], lag_s) and _bits(flat[1], lag_n)           # the flat form is the list form


def test_a_lag_without_overlap_has_no_terms():
    from uplift_upsample_3dhpe_amd import predict
    cams, views, _, _ = AU.scene([0, 0], [40, 3], 1, 5, 5, lost=0.0)
    sums, terms = predict.view_lag_sums_host([views[0][0], views[1][0]], [0, 1], cams, None, L6)
    # frame f of p pairs with g = f - l in 0 .. 2: l = -6 .. -3 leave no f >= 0; l = -2 leaves f = 0; l >= 0 leaves three frames
    assert terms[0, 1].tolist() == [0, 0, 0, 0, 5, 10] + [15] * 7 and not sums[0, 1, :4].any() and (sums[0, 1, 4:] > 0).all()
    back = predict.view_lag_sums_host([views[1][0], views[0][0]], [0, 1], cams, None, L6)      # the short track as the reference
    assert back[1][0, 1].tolist() == [15] * 7 + [10, 5, 0, 0, 0, 0]    # g = f - l >= 0 needs l <= f <= 2
    twin = [cams[0], cams[0]]                                            # coincident cameras: no terms at any lag
    assert not predict.view_lag_sums_host([views[0][0], views[1][0]], [0, 1], twin, None, L6)[1].any()


@pytest.mark.parametrize("k", [1, 4])
def test_dropping_k_leading_frames_moves_the_profile_by_k(k):
    from uplift_upsample_3dhpe_amd import predict
    cams, views, _, valid = AU.scene([0, 2], [300, 290], 1, 5, 17)
    p, q = views[0][0], views[1][0].copy()
    q[:k] = np.nan                                                       # the frames that go carry no term: the same frame pairs remain
    a_s, a_n = predict.view_lag_sums_host([p, q], [0, 1], cams, None, L6, [valid[0][0], valid[1][0]])
    b_s, b_n = predict.view_lag_sums_host([p, q[k:]], [0, 1], cams, None, L6, [valid[0][0], valid[1][0][k:]])
    assert a_n[0, 1].all()
    assert _bits(b_s[0, 1, k:], a_s[0, 1, :2 * L6 + 1 - k]) and _bits(b_n[0, 1, k:], a_n[0, 1, :2 * L6 + 1 - k])       # lag l + k of the cut track = lag l
    off_a = predict.view_offsets_host(a_s, a_n, [0, 1], 2, L6, 50)
    off_b = predict.view_offsets_host(b_s, b_n, [0, 1], 2, L6, 50)
    assert off_a[0].tolist() == [0, 2] and off_b[0].tolist() == [0, 2 + k] and off_a[2][1] == off_b[2][1]


# ---- 2. offsets ----------------------------------------------------------------------------------------------------------------------------
def _tables(n_ref, M, L, fill):
    sums, terms = np.zeros((n_ref, M, 2 * L + 1)), np.zeros((n_ref, M, 2 * L + 1), np.int32)
    for (p, q, l), (s, n) in fill.items():
        sums[p, q, l + L], terms[p, q, l + L] = s, n
    return sums, terms


def test_offset_ties_go_to_the_smaller_shift_then_the_smaller_lag():
    from uplift_upsample_3dhpe_amd import predict
    view_of = [0, 1]
    every = {(0, 1, l): (2.0, 100) for l in range(-3, 4)}
    off, state, score = predict.view_offsets_host(*_tables(1, 2, 3, every), view_of, 2, 3, 50)
    assert off.tolist() == [0, 0] and state.tolist() == [1, 1] and score.tolist() == [0.0, 0.02]             # all lags equal: no shift
    off, _, _ = predict.view_offsets_host(*_tables(1, 2, 3, {(0, 1, -2): (1.0, 100), (0, 1, 2): (1.0, 100), (0, 1, 3): (1.0, 100)}), view_of, 2, 3, 50)
    assert off.tolist() == [0, -2]                                       # |l| equal: the smaller l; the larger |l| loses
    off, _, _ = predict.view_offsets_host(*_tables(1, 2, 3, {(0, 1, -2): (1.0, 100), (0, 1, 1): (2.0, 200), (0, 1, 3): (1.5, 100)}), view_of, 2, 3, 50)
    assert off.tolist() == [0, 1]                                        # equal means from other sums and terms
    off, _, score = predict.view_offsets_host(*_tables(1, 2, 3, {(0, 1, 0): (5.0, 100), (0, 1, 3): (4.0, 100), (0, 1, -1): (1.0, 49)}), view_of, 2, 3, 50)
    assert off.tolist() == [0, 3] and score[1] == 0.04                   # the smaller score wins whatever its shift; 49 terms do not speak
    # two reference tracks: per lag each takes its best partner (ties to the smaller q), S and n add up over p
    fill = {(0, 2, 1): (1.0, 100), (0, 3, 1): (1.0, 100), (1, 2, 1): (9.0, 100), (1, 3, 1): (3.0, 100), (0, 2, 0): (2.5, 100)}
    t = _tables(2, 4, 1, fill)
    off, state, score = predict.view_offsets_host(*t, [0, 0, 1, 1], 2, 1, 50)
    assert off.tolist() == [0, 1] and score[1] == (1.0 + 3.0) / 200.0
    off, state, score = predict.view_offsets_host(*t, [0, 0, 1, 1], 2, 1, 50, same_index=True)
    assert off.tolist() == [0, 1] and score[1] == (1.0 + 3.0) / 200.0   # p = 0 with q = 2, p = 1 with q = 3
    fill[(1, 3, 1)] = (3.0, 10)
    off, state, score = predict.view_offsets_host(*_tables(2, 4, 1, fill), [0, 0, 1, 1], 2, 1, 50, same_index=True)
    assert off.tolist() == [0, 1] and score[1] == 0.01                   # p = 1 has no candidate at lag 1: p = 0 alone, 1 / 100 < 2.5 / 100


def test_a_standing_person_gives_offset_zero():
    from uplift_upsample_3dhpe_amd import predict
    cams, views, _, _ = AU.scene([0, 0], [40, 40], 1, 5, 9, still=True)
    p, q = views[0][0].copy(), views[1][0]
    assert (p == p[0]).all() and (q == q[0]).all()
    p[:L6], p[40 - L6:] = np.nan, np.nan                                 # every lag pairs the same 28 frames of p with the same frame of q
    off, state, score, sums, terms = predict.align_views_host([[p], [q]], cams, max_lag=L6, min_terms=50)
    assert (terms[0, 1] == 28 * 5).all() and len(set(sums[0, 1].tolist())) == 1
    assert off.tolist() == [0, 0] and state.tolist() == [1, 1]


def test_same_index_against_the_unrestricted_rule_on_shuffled_tracks():
    from uplift_upsample_3dhpe_amd import predict
    offsets, lengths = [0, 4, -2], [90, 80, 100]
    cams, views, _, valid = AU.scene(offsets, lengths, 2, 5, 23)
    same = predict.align_views_host(views, cams, valid, L6, 50, same_index=True)
    free = predict.align_views_host(views, cams, valid, L6, 50, same_index=False)
    assert same[0].tolist() == free[0].tolist() == offsets and _bits(same[2], free[2])       # in order: the best partner is the same index
    swapped = [views[0], views[1][::-1], views[2]]
    flags = [valid[0], valid[1][::-1], valid[2]]
    free2 = predict.align_views_host(swapped, cams, flags, L6, 50, same_index=False)
    assert free2[0].tolist() == offsets and _bits(free2[2], free[2])     # the same pairs are found: the same sums in the same order
    same2 = predict.align_views_host(swapped, cams, flags, L6, 50, same_index=True)
    assert same2[1].tolist() == [1, 1, 1] and same2[2][1] > 100 * free[2][1] and _bits(same2[2][2], free[2][2])      # two persons taken for one
    with pytest.raises(ValueError):
        predict.align_views_host([views[0], views[1][:1], views[2]], cams, None, L6, 50, same_index=True)
    assert predict.align_views_host([views[0], views[1][:1], views[2]], cams, None, L6, 50)[1].tolist() == [1, 1, 1]     # unrestricted: any counts


def test_a_view_that_cannot_be_aligned_has_state_zero():
    from uplift_upsample_3dhpe_amd import predict
    cams, views, _, _ = AU.scene([0, 1, 2, 0], [60, 60, 8, 60], 1, 5, 31, lost=0.0)
    gone = np.full_like(views[1][0], np.nan)
    off, state, score, sums, terms = predict.align_views_host([[], views[0], [gone], views[2], []], [cams[0]] + cams, max_lag=L6, min_terms=50)
    # view 0 is empty, view 1 the reference, view 2 all NaN, view 3 too short for 50 terms (8 frames of 5 joints), view 4 empty
    assert off.tolist() == [0] * 5 and state.tolist() == [1, 1, 0, 0, 1] and not score.any() and terms.shape == (1, 3, 13)
    assert not terms[0, 1].any() and terms[0, 2].max() == 40
    off, state, score = predict.view_offsets_host(sums, terms, [1, 2, 3], 5, L6, 40)
    assert off.tolist() == [0, 0, 0, 2, 0] and state.tolist() == [1, 1, 0, 1, 1] and score[3] > 0


# ---- 3. crop_views and the refusals --------------------------------------------------------------------------------------------------------
def test_crop_views_windows_and_refusals():
    from uplift_upsample_3dhpe_amd import predict
    a, b, c = (np.arange(T * 2 * 2, dtype=np.float32).reshape(T, 2, 2) for T in (10, 12, 8))
    fa, fb, fc = np.ones(10, np.uint8), np.ones((12, 2), np.uint8), np.ones(8, np.uint8)
    views, valid = [[a, a], [b], [], [c]], [[fa, None], [fb], [], ["finite"]]
    cropped, kept, first = predict.crop_views(views, [0, -3, 7, 2], valid)
    # common times: view 0 covers 0 .. 9, view 1 -3 .. 8, view 3 2 .. 9: the window is 2 .. 8
    assert first == [2, 5, 0, 0] and [[len(t) for t in v] for v in cropped] == [[7, 7], [7], [], [7]]
    assert np.shares_memory(cropped[0][0], a) and np.array_equal(cropped[0][1], a[2:9]) and np.array_equal(cropped[1][0], b[5:12])
    assert np.array_equal(cropped[3][0], c[:7]) and kept[0][1] is None and kept[3][0] == "finite"
    assert kept[0][0].shape == (7,) and kept[1][0].shape == (7, 2) and np.shares_memory(kept[1][0], fb)
    assert predict.crop_views(views, [0, -3, 7, 2], "finite")[1] == "finite" and predict.crop_views(views, [0, -3, 7, 2])[1] is None
    assert predict.crop_views([[a]], [5])[2] == [0] and len(predict.crop_views([[a], [c]], [0, 9])[0][0][0]) == 1
    for bad in (dict(views=[[a], [c]], offsets=[0, 10]),                  # the views share no frame
                dict(views=[[a], [c]], offsets=[0]), dict(views=[[a], [c]], offsets=[0, 1.5]), dict(views=[[a], [c]], offsets=[0, True]),
                dict(views=[[a, b]], offsets=[0]),                       # a view whose tracks differ in length
                dict(views=[[], []], offsets=[0, 0]), dict(views=[a], offsets=[0]),
                dict(views=[[a], [c]], offsets=[0, 0], valid=[[fa]]), dict(views=[[a], [c]], offsets=[0, 0], valid=[[fa], [fa]])):
        with pytest.raises(ValueError):
            predict.crop_views(**bad)


def test_refusals_of_the_new_calls():
    from uplift_upsample_3dhpe_amd import predict
    cams, views, _, valid = AU.scene([0, 1], [30, 40], 2, 5, 3)
    kp, view_of, frames, flags = AU.stacked(views, valid)
    assert predict.check_align(None) is None and predict.check_align(False) is None and predict.check_align([0, np.int64(-2)]) == [0, -2]
    assert (predict.check_align(True).max_lag, predict.check_align(True).min_terms) == (50, 50) == tuple(predict.ALIGN_DEFAULTS.values())
    for bad in ("yes", 3, [0.5, 1], [], [True, 0], predict.MatchViews()):
        with pytest.raises(ValueError):
            predict.check_align(bad)
    for bad in (dict(max_lag=0), dict(max_lag=513), dict(max_lag=2.0), dict(max_lag=True), dict(min_terms=0), dict(min_terms=1.5)):
        with pytest.raises(ValueError):
            predict.AlignViews(**bad)
    assert predict.AlignViews(512, 1).max_lag == predict.MAX_ALIGN_LAG
    for bad in (dict(kp=kp, frames=None), dict(kp=kp, frames=frames[:-1]), dict(kp=kp, frames=frames + 1), dict(kp=kp, frames=frames, max_lag=0),
                dict(kp=kp, frames=frames, max_lag=513), dict(kp=kp, frames=frames, flags=flags[:-1]), dict(kp=kp, frames=frames, view_of=view_of[::-1]),
                dict(kp=kp[None], frames=frames), dict(kp=list(views[0]) + list(views[1]), frames=[30, 30, 40, 41]),
                dict(kp=np.zeros((4, 65, 2), np.float32), frames=[1, 1, 1, 1])):
        args = dict(view_of=view_of, cameras=cams, max_lag=L6)
        args.update(bad)
        with pytest.raises(ValueError):
            predict.view_lag_sums_host(**args)
    sums, terms = predict.view_lag_sums_host(kp, view_of, cams, frames, L6, flags)
    for bad in (dict(max_lag=5), dict(min_terms=0), dict(view_of=[0, 0, 0, 1]), dict(view_of=[0, 0, 0, 1], same_index=True), dict(terms=terms[:1])):
        args = dict(sums=sums, terms=terms, view_of=view_of, views=2, max_lag=L6, min_terms=50)
        args.update(bad)
        with pytest.raises(ValueError):
            predict.view_offsets_host(**args)
    for bad in (dict(views=[[], []]), dict(views=[views[0], [views[1][0][:, :4]]]), dict(views=views, valid=[valid[0]]), dict(views=views, max_lag=0),
                dict(views=views, cameras=cams[:1]), dict(views=[views[0], views[1][:1]], same_index=True)):
        args = dict(cameras=cams)
        args.update(bad)
        with pytest.raises(ValueError):
            predict.align_views_host(**args)


def test_refusals_of_predict_views_with_align_need_no_device():
    from uplift_upsample_3dhpe_amd import predict
    cams, views, _, valid = AU.scene([0, 1], [30, 40], 2, 17, 3)
    ragged = [views[0], [views[1][0], views[1][1][:35]]]
    for bad, word in ((dict(align=True, keyframes_only=True), "keyframes_only"), (dict(align=[0, 1], out_fps=25), "out_fps"),
                      (dict(align=[0, 1], fps=[50, 50]), "fps"), (dict(align=True, fps=[50, 50]), "fps"),
                      (dict(align=[0, 1], views=ragged), "view 1"), (dict(align=True, views=ragged), "view 1"),
                      (dict(align=predict.AlignViews(max_lag=60)), "max_lag"), (dict(align=[0, 1, 2]), "offset"), (dict(align=[0, 40]), "no frame"),
                      (dict(align="yes"), "align"), (dict(align=[0, 1], views=[views[0], views[1][:1]]), "same persons"),
                      (dict(align=[0, 1], valid=[valid[0]]), "valid")):
        args = dict(views=views, cameras=cams)
        args.update(bad)
        with pytest.raises(ValueError, match=word):
            predict.predict_views(None, None, **args)


# ---- 4. recovery ---------------------------------------------------------------------------------------------------------------------------
RECOVERY_FLOOR = 7.98


@pytest.mark.parametrize("seed", [3, 11, 29])
def test_the_true_offsets_come_back_decisively(seed):
    """3 ring cameras, 2 swaying persons, 5 joints, 0.5 px of noise, 4 % of the joints lost as NaN and 4 % as cleared flags; views of
    90 / 100 / 80 frames with offsets 0 / -3 / +5, ``max_lag`` 6, ``min_terms`` 50, ``same_index``.  The ratio between the best wrong
    lag's score and the true lag's score, per later view, measured with the numpy mirror:
        seed  3: 80.3 and 31.9      seed 11: 82.7 and 95.9      seed 29: 76.6 and 103.0
    (the true lag's root-mean-square line distance is 2.5 to 2.7 mm).  ``RECOVERY_FLOOR`` is a quarter of the smallest, 31.93 / 4: the
    minimum has to be decisive, not accidental."""
    from uplift_upsample_3dhpe_amd import predict
    offsets, lengths = [0, -3, 5], [90, 100, 80]
    cams, views, _, valid = AU.scene(offsets, lengths, 2, 5, seed)
    for same_index in (True, False):
        off, state, score, sums, terms = predict.align_views_host(views, cams, valid, max_lag=L6, min_terms=50, same_index=same_index)
        assert off.tolist() == offsets and state.tolist() == [1, 1, 1] and score[0] == 0.0 and (np.sqrt(score[1:]) < 0.004).all()
        _, view_of, _, _ = AU.stacked(views)
        ratios = AU.score_ratio(sums, terms, view_of, 3, L6, 50, same_index, offsets)
        print(f"seed {seed}, same_index {same_index}: offsets {off.tolist()}, rms {np.sqrt(score[1:]).tolist()}, wrong / true {ratios}")
        assert min(ratios) > RECOVERY_FLOOR, ratios
    cropped, _, first = predict.crop_views(views, off.tolist())
    assert first == [5, 8, 0] and {len(t) for v in cropped for t in v} == {80}      # common times 5 .. 84
