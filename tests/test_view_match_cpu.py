"""CPU: who is who across cameras (include/uu3d.h, WHO IS WHO; views.py) -- the rules in numpy (``predict.view_pair_sums_host``,
``predict.group_views_host``, ``predict.gather_view_tracks_host``, ``predict.match_views_host``), the refusals and the C ABI.
  1. the mirrors agree, on the bits, with a plain double loop over Python floats that follows the header statement by statement: the order
     of operations, the strided lanes and the tree.
  2. on the seeded scenes of tests/view_match_util.py ``match_views_host`` returns exactly the true partition with the defaults.  This is
     a condition on the SCENES (persons 1.2 m apart on steps of 0.6 m, 0.5 px of pixel noise): the true pairs' root-mean-square line
     distance stays below 0.004 m and every wrong pair's above 0.3 m, against ``max_dist`` = 0.2 m.
  3. the fixed cases: a person one camera sees, an empty view, twin cameras, an all-NaN track, a pair below ``min_terms``, parallel rays,
     exact ties, the view-order rule.
  4. refusals, before any device is touched; the C ABI: exported, declared, guarded."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import util
from tests import view_match_util as MU
from tests import views_util as VU

SCENES = [((3, 2, 2), 3, 30, 17, 5), ((2, 3, 1), 3, 70, 17, 7), ((0, 2, 2), 3, 30, 5, 9), ((4, 4, 3, 2), 4, 40, 17, 13), ((1,) * 8, 1, 20, 17, 3),
          ((2, 0, 3), 3, 257, 5, 21)]


def _per_view(person, counts):
    starts = np.concatenate([[0], np.cumsum(counts)])
    return [[int(k) for k in person[starts[v]:starts[v + 1]]] for v in range(len(counts))]


# ---- 1. the order of operations ----------------------------------------------------------------------------------------------------------
def _scalar_pair(kp, flags, p, q, cp, cq):
    """sums[p][q], terms[p][q] in Python floats (IEEE float64, every operation rounded once), the header's statements one by one."""
    fin = lambda x: x == x and abs(x) != float("inf")
    o = [float(cq[13 + i]) - float(cp[13 + i]) for i in range(3)]
    oo = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]
    if not fin(oo) or not oo > 0.0:
        return 0.0, 0
    T, J = kp.shape[1:3]
    s_f, n_f = [], []
    for f in range(T):
        s, n = 0.0, 0
        for j in range(J):
            rays = []
            for m, c in ((p, cp), (q, cq)):
                u, v = float(kp[m, f, j, 0]), float(kp[m, f, j, 1])
                if (flags is not None and flags[m, f, j] == 0) or not fin(u) or not fin(v):
                    break
                c = [float(x) for x in c]
                a, b = (u - c[2]) / c[0], (v - c[3]) / c[1]
                rays.append([(c[4 + i] * a + c[7 + i] * b) + c[10 + i] for i in range(3)])
            if len(rays) < 2:
                continue
            dp, dq = rays
            c0, c1, c2 = dp[1] * dq[2] - dp[2] * dq[1], dp[2] * dq[0] - dp[0] * dq[2], dp[0] * dq[1] - dp[1] * dq[0]
            cc = (c0 * c0 + c1 * c1) + c2 * c2
            pp = (dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2]
            qq = (dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2]
            oc = (o[0] * c0 + o[1] * c1) + o[2] * c2
            if cc == 0.0:
                continue
            e = (oc * oc) / cc
            if cc > 2.0 ** -20 * (pp * qq) and fin(e):
                s, n = s + e, n + 1
        s_f.append(s)
        n_f.append(n)
    x = [0.0] * 256
    for l in range(256):
        for f in range(l, T, 256):
            x[l] = x[l] + s_f[f]
    stride = 128
    while stride >= 1:
        for l in range(stride):
            x[l] = x[l] + x[l + stride]
        stride //= 2
    return x[0], sum(n_f)


def test_the_mirror_is_the_scalar_rule():
    from uplift_upsample_3dhpe_amd import predict
    cams, views, _, valid = MU.scene((2, 1, 1), 2, 261, 3, 31)
    kp, view_of, flags = MU.stacked(views, valid)
    rows = predict.view_rows(cams)
    for fl in (flags, None):
        sums, terms = predict.view_pair_sums_host(kp, view_of, cams, fl)
        assert sums.dtype == np.float64 and terms.dtype == np.int32 and sums.shape == terms.shape == (4, 4)
        for p in range(4):
            for q in range(4):
                want = (0.0, 0) if view_of[p] == view_of[q] else _scalar_pair(kp, fl, min(p, q), max(p, q), rows[view_of[min(p, q)]], rows[view_of[max(p, q)]])
                assert np.float64(want[0]).view(np.uint64) == sums[p, q].view(np.uint64) and want[1] == terms[p, q], (p, q)
        assert (terms[0, 2:] > 100).all() and terms[0, 1] == 0
    again = predict.view_pair_sums_host(kp, view_of, rows, flags)       # the rows themselves are taken as well
    assert np.array_equal(again[0], predict.view_pair_sums_host(kp, view_of, cams, flags)[0])


# ---- 2. the seeded scenes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SCENES, ids=lambda c: "-".join(str(n) for n in c[0]) + f"-T{c[2]}-K{c[3]}")
def test_the_seeded_scenes_come_out_as_the_true_partition(case):
    from uplift_upsample_3dhpe_amd import predict
    counts, P, T, K, seed = case
    cams, views, truth, valid = MU.scene(counts, P, T, K, seed)
    person, n, table, sums, terms = predict.match_views_host(views, cams, valid)
    M = sum(counts)
    assert person.dtype == n.dtype == table.dtype == np.int32 and person.shape == (M,) and n.shape == (1,) and table.shape == (len(counts), M)
    flat = [k for v in truth for k in v]
    with np.errstate(all="ignore"):
        rms = np.sqrt(sums / terms)
    right = [rms[p, q] for p in range(M) for q in range(p + 1, M) if terms[p, q] > 0 and flat[p] == flat[q]]
    wrong = [rms[p, q] for p in range(M) for q in range(p + 1, M) if terms[p, q] > 0 and flat[p] != flat[q]]
    print(f"{counts}: {int(n[0])} persons, true pairs' rms <= {max(right or [0.0]):.4f} m, wrong pairs' >= {min(wrong or [np.inf]):.4f} m")
    assert MU.same_partition(_per_view(person, counts), truth)
    assert int(n[0]) == len(set(flat))
    # the table is the inverse of person; the columns behind n_persons are -1
    for v in range(len(counts)):
        for k in range(M):
            m = table[v, k]
            assert (m == -1) if k >= n[0] else (m == -1 or (person[m] == k and np.repeat(np.arange(len(counts)), counts)[m] == v))
    assert sorted(int(m) for m in table[table >= 0]) == list(range(M))
    assert np.array_equal(sums, sums.T) and np.array_equal(terms, terms.T) and not sums.diagonal().any()
    # without the flags (the finite test alone) and with "finite": the same partition
    for v in (None, "finite"):
        assert MU.same_partition(_per_view(predict.match_views_host(views, cams, v)[0], counts), truth)


# ---- 3. the fixed cases -----------------------------------------------------------------------------------------------------------------
def test_a_person_one_camera_sees_an_empty_view_and_an_all_nan_track():
    from uplift_upsample_3dhpe_amd import predict
    cams, views, truth, _ = MU.scene((3, 0, 2), 3, 30, 17, 41)
    only = [i for i in truth[0] if i not in truth[2]]
    assert len(only) == 1                                                # one person only camera 0 sees; view 1 is empty
    person, n, table, _, terms = predict.match_views_host(views, cams)
    per = _per_view(person, (3, 0, 2))
    assert MU.same_partition(per, truth) and n[0] == 3 and per[1] == [] and (table[1] == -1).all()
    lonely = per[0][truth[0].index(only[0])]
    assert table[2, lonely] == -1 and (table[0, :3] >= 0).all()
    views[2][1][:] = np.nan                                              # a track of all-NaN frames: no terms, a person of its own
    person, n, table, _, terms = predict.match_views_host(views, cams, "finite")
    assert n[0] == 4 and person[4] == 3 and not terms[4].any() and list(table[:, 3]) == [-1, -1, 4]


def test_twin_cameras_have_no_terms_between_them():
    from uplift_upsample_3dhpe_amd import predict
    cams, views, truth, _ = MU.scene((2, 2, 2), 2, 30, 17, 43, twin=True)
    assert cams[1] is cams[0]
    person, n, table, sums, terms = predict.match_views_host(views, cams)
    assert not terms[:2, 2:4].any() and not sums[:2, 2:4].any() and terms[:2, 4:].all() and terms[2:4, 4:].all()
    # views 0 and 1 cannot be matched by geometry: view 1's tracks are new persons; view 2 then joins each person's track of view 0 and
    # the twin's persons stay with one view, whatever the truth is
    assert list(person[:4]) == [0, 1, 2, 3] and n[0] == 4
    assert [truth[0][person[4]], truth[0][person[5]]] == truth[2]


def test_min_terms_and_parallel_rays():
    from uplift_upsample_3dhpe_amd import predict
    cams, views, truth, _ = MU.scene((1, 1), 1, 7, 7, 47, lost=0.0)     # 49 terms: one below the default
    person, n, _, sums, terms = predict.match_views_host(views, cams)
    assert terms[0, 1] == 49 and np.sqrt(sums[0, 1] / 49) < 0.01 and list(person) == [0, 1] and n[0] == 2
    person, n, _, _, _ = predict.match_views_host(views, cams, min_terms=49)
    assert list(person) == [0, 0] and n[0] == 1
    person, n, _, _, _ = predict.match_views_host(views, cams, min_terms=49, max_dist=1e-5)      # allowed needs the distance as well
    assert list(person) == [0, 1]
    cams = VU.ring_cameras(2, 49)
    a, b = MU.vanishing_tracks(cams, 30, 17, 51)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    person, n, _, sums, terms = predict.match_views_host([[a], [b]], cams)
    assert terms[0, 1] == 0 and sums[0, 1] == 0.0 and list(person) == [0, 1]


def test_ties_and_the_view_order_rule():
    from uplift_upsample_3dhpe_amd import predict
    cams, views, truth, _ = MU.scene((1, 1, 1), 1, 30, 17, 53)
    # a duplicated TRACK in view 1: both candidates cost the same, the smaller track index gets the person
    dup = [views[0], [views[1][0], views[1][0].copy()], views[2]]
    person, n, table, sums, terms = predict.match_views_host(dup, cams)
    assert sums[0, 1].view(np.uint64) == sums[0, 2].view(np.uint64) and terms[0, 1] == terms[0, 2] > 0
    assert list(person) == [0, 0, 1, 0] and n[0] == 2 and list(table[1, :2]) == [1, 2]
    # a duplicated PERSON (view 0 holds the same track twice): the smaller person id gets view 1's track
    dup = [[views[0][0], views[0][0].copy()], views[1], views[2]]
    person, n, table, _, _ = predict.match_views_host(dup, cams)
    assert list(person[:3]) == [0, 1, 0] and n[0] == 2
    # on the tables themselves: smallest cost first, then smaller k, then smaller b; persons born in a step do not compete in it
    view_of = np.array([0, 0, 1, 1, 2], np.int32)
    sums = np.zeros((5, 5))
    terms = np.zeros((5, 5), np.int32)
    for p, q, s in ((0, 2, 4.0), (0, 3, 1.0), (1, 2, 1.0), (1, 3, 1.0), (2, 4, 0.5), (3, 4, 0.5), (0, 4, 100.0), (1, 4, 100.0)):
        sums[p, q] = sums[q, p] = s
        terms[p, q] = terms[q, p] = 100
    person, n, table = predict.group_views_host(sums, terms, view_of, 3, max_dist=0.5, min_terms=50)
    # step 1: costs 0.04 / 0.01 / 0.01 / 0.01 -> (k 0, b 3) wins the tie, then (k 1, b 2); step 2: person 0 = {0, 3}: (100 + 0.5) / 200 >
    # 0.25, person 1 = {1, 2} likewise: track 4 is a new person
    assert list(person) == [0, 1, 1, 0, 2] and n[0] == 3 and table[:, :3].tolist() == [[0, 1, -1], [3, 2, -1], [-1, -1, 4]]
    person, n, _ = predict.group_views_host(sums, terms, view_of, 3, max_dist=1.0, min_terms=50)
    assert list(person) == [0, 1, 1, 0, 0]                                # both persons cost 0.5025: the smaller id
    person, n, _ = predict.group_views_host(sums, terms, view_of, 3, max_dist=1.0, min_terms=201)
    assert list(person) == [0, 1, 2, 3, 4] and n[0] == 5
    # the order of the views matters: the same tracks with the views swapped group differently when a middle view is the only link
    chain = np.zeros((3, 3))
    chain[0, 1] = chain[1, 0] = chain[1, 2] = chain[2, 1] = 1.0
    chain[0, 2] = chain[2, 0] = 1e4
    t = np.full((3, 3), 100, np.int32)
    np.fill_diagonal(t, 0)
    assert list(predict.group_views_host(chain, t, [0, 1, 2], 3, max_dist=0.2)[0]) == [0, 0, 1]       # {0, 1}: (1 + 1e4) / 200 > 0.04
    swapped = chain[[0, 2, 1]][:, [0, 2, 1]]
    assert list(predict.group_views_host(swapped, t, [0, 1, 2], 3, max_dist=0.2)[0]) == [0, 1, 0]


def test_gather_lays_the_tracks_out_per_person():
    from uplift_upsample_3dhpe_amd import predict
    rng = np.random.default_rng(3)
    M, T, J = 3, 4, 5
    poses = rng.normal(size=(M * T, J, 3)).astype(np.float32)
    kp = rng.normal(size=(M * T, J, 2)).astype(np.float32)
    kp[5, 2] = np.nan
    flags = (rng.uniform(size=(M * T, J)) > 0.3).astype(np.uint8)
    src = np.array([[2, -1], [0, 1]], np.int32)
    p, k, f = predict.gather_view_tracks_host(src, poses, kp, flags, T)
    assert p.shape == (2, 2 * T, J, 3) and k.shape == (2, 2 * T, J, 2) and f.shape == (2, 2 * T, J) and f.dtype == np.uint8
    assert np.array_equal(p[0, :T], poses[2 * T:]) and np.array_equal(f[1, T:], flags[T:2 * T]) and np.array_equal(k[1, :T], kp[:T])
    assert not p[0, T:].any() and np.isnan(k[0, T:]).all() and not f[0, T:].any()
    assert np.array_equal(p[0, T:].view(np.uint32), np.zeros((T, J, 3), np.uint32))                    # +0.0
    ones = predict.gather_view_tracks_host(src, poses, kp, None, T)[2]
    assert ones[0, :T].all() and not ones[0, T:].any() and ones[1].all()
    with pytest.raises(ValueError, match="poses must be"):
        predict.gather_view_tracks_host(src, poses[:-1], kp, flags, T)
    with pytest.raises(ValueError, match="kp2d must be"):
        predict.gather_view_tracks_host(src, poses, kp, flags, 5)


# ---- 4. refusals and the C ABI --------------------------------------------------------------------------------------------------------------
def test_refusals_need_no_device():
    from uplift_upsample_3dhpe_amd import predict
    cams, views, _, _ = MU.scene((2, 1), 2, 12, 17, 61)
    cfg = util.load_config("h36m_81")
    host = predict.match_views_host
    with pytest.raises(ValueError, match="one common number of frames"):
        host([views[0], [views[1][0][:-1]]], cams)
    with pytest.raises(ValueError, match="at most 64 tracks"):
        host([[views[0][0]] * 33, [views[1][0]] * 32], cams)
    with pytest.raises(ValueError, match="needs extrinsics"):
        host(views, [c.without(extrinsics=True) for c in cams])
    with pytest.raises(ValueError, match="one Camera per view"):
        host(views, cams[:1])
    with pytest.raises(ValueError, match="at least one view must hold a track"):
        host([[], []], cams)
    with pytest.raises(ValueError, match="a list of 2 lists"):
        host(views, cams, valid=[np.ones(12)])
    with pytest.raises(ValueError, match="max_dist must be"):
        host(views, cams, max_dist=float("nan"))
    with pytest.raises(ValueError, match="min_terms must be"):
        host(views, cams, min_terms=0)
    kp, view_of, _ = MU.stacked(views)
    with pytest.raises(ValueError, match="view_of must ascend"):
        predict.view_pair_sums_host(kp, [0, 1, 0], cams)
    with pytest.raises(ValueError, match="one view per track"):
        predict.view_pair_sums_host(kp, [0, 1], cams)
    with pytest.raises(ValueError, match="match must be None, True or a MatchViews"):
        predict.predict_views(None, cfg, views, cams, match="yes")
    assert predict.check_match(None) is None and predict.check_match(True).min_terms == 50 and predict.check_match(True).max_dist == 0.2
    assert predict.MATCH_DEFAULTS == dict(max_dist=0.2, min_terms=50) and predict.VIEW_PARALLEL == 2.0 ** -20 and predict.MAX_MATCH_TRACKS == 64
    # predict_views(match=True): refused before the model (None here) is touched
    call = lambda v, c, **kw: predict.predict_views(None, cfg, v, c, match=True, **kw)
    with pytest.raises(ValueError, match="one common number of frames"):
        call([views[0], [views[1][0][:-1]]], cams)
    with pytest.raises(ValueError, match="bones as a per-person list"):
        call(views, cams, bones=[np.ones(17), np.ones(17)])
    with pytest.raises(ValueError, match="at most 64 tracks"):
        call([[views[0][0]] * 65, []], cams)
    with pytest.raises(ValueError, match="needs extrinsics"):
        call(views, [c.without(extrinsics=True) for c in cams])
    with pytest.raises(ValueError, match="one fps for all tracks"):
        call(views, cams, fps=[25, 25, 25])
    with pytest.raises(ValueError, match="does not take out_fps"):
        call(views, cams, fps=25, out_fps=50)
    with pytest.raises(ValueError, match="does not take keyframes_only"):
        call(views, cams, keyframes_only=True)
    with pytest.raises(ValueError, match="interpolation must be one of"):
        call(views, cams, interpolation="spline")
    with pytest.raises(ValueError, match="every view must hold the same persons"):
        predict.predict_views(None, cfg, views, cams)                    # without match the old precondition stands


def test_entry_points_are_declared_bound_and_guarded():
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    for s in ("uu3d_view_pair_sums", "uu3d_group_views", "uu3d_gather_view_tracks"):
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s) and re.search(r"\b" + s + r"\s*\(", header)
    assert header.index("SEVERAL VIEWS") < header.index("WHO IS WHO")
    api = open(os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc", "uu3d_api.hip")).read()
    assert '#include "uu3d_view_match.h"' in api and '#include "uu3d_view_match_api.inc"' in api
    text = open(os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc", "uu3d_view_match.h")).read()
    assert "kViewParallel = 0x1p-20" in text and "1e-3 rad" in text and "atomic" not in re.sub(r"//[^\n]*", "", text).lower()
    buf = (C.c_double * 512)()                                          # 8-byte aligned host memory: every call below returns before a launch
    a = C.addressof(buf)
    p = lambda off=0: C.c_void_p(a + off)
    vo = lambda *v: (C.c_int32 * len(v))(*v)
    bad, unsupported = _capi.UU3D_ERR_INVALID_ARGUMENT, _capi.UU3D_ERR_UNSUPPORTED
    pair = lib.uu3d_view_pair_sums
    #    kp, flags, view_of (host), tracks, frames, J, views, cameras, sums, terms, stream
    assert pair(p(), None, vo(0, 1, 1), 3, 4, 17, 9, p(512), p(1024), p(2048), None) == unsupported
    assert pair(p(), None, vo(*([0] * 65)), 65, 4, 17, 2, p(512), p(1024), p(2048), None) == unsupported
    assert pair(p(), None, vo(0, 1, 1), 3, 4, 65, 2, p(512), p(1024), p(2048), None) == unsupported
    assert pair(p(), None, vo(0, 1, 0), 3, 4, 17, 2, p(512), p(1024), p(2048), None) == bad               # view_of does not ascend
    assert pair(p(), None, vo(0, 1, 2), 3, 4, 17, 2, p(512), p(1024), p(2048), None) == bad               # no such view
    assert pair(p(), None, vo(-1, 0, 1), 3, 4, 17, 2, p(512), p(1024), p(2048), None) == bad
    assert pair(p(), None, None, 3, 4, 17, 2, p(512), p(1024), p(2048), None) == bad
    assert pair(p(), None, vo(0, 1, 1), 0, 4, 17, 2, p(512), p(1024), p(2048), None) == bad
    assert pair(p(), None, vo(0, 1, 1), 3, 0, 17, 2, p(512), p(1024), p(2048), None) == bad
    assert pair(p(), None, vo(0, 1, 1), 3, 4, 0, 2, p(512), p(1024), p(2048), None) == bad
    assert pair(p(), None, vo(0, 1, 1), 3, 4, 17, 0, p(512), p(1024), p(2048), None) == bad
    assert pair(p(), None, vo(0, 1, 1), 3, 2 ** 31 // 17 + 1, 17, 2, p(512), p(1024), p(2048), None) == bad   # T * J could overflow the terms
    assert pair(None, None, vo(0, 1, 1), 3, 4, 17, 2, p(512), p(1024), p(2048), None) == bad
    assert pair(p(), None, vo(0, 1, 1), 3, 4, 17, 2, None, p(1024), p(2048), None) == bad
    assert pair(p(), None, vo(0, 1, 1), 3, 4, 17, 2, p(512), None, p(2048), None) == bad
    assert pair(p(), None, vo(0, 1, 1), 3, 4, 17, 2, p(512), p(1024), None, None) == bad
    assert pair(p(4), None, vo(0, 1, 1), 3, 4, 17, 2, p(512), p(1024), p(2048), None) == bad              # 8-byte loads of the pixels
    assert pair(p(), None, vo(0, 1, 1), 3, 4, 17, 2, p(516), p(1024), p(2048), None) == bad
    assert pair(p(), None, vo(0, 1, 1), 3, 4, 17, 2, p(512), p(1028), p(2048), None) == bad
    assert pair(p(), None, vo(0, 1, 1), 3, 4, 17, 2, p(512), p(1024), p(2050), None) == bad
    group = lib.uu3d_group_views
    #    sums, terms, view_of (host), tracks, views, max_dist, min_terms, person, n_persons, table, stream
    assert group(p(), p(512), vo(0, 1, 1), 3, 9, 0.2, 50, p(1024), p(1100), p(1200), None) == unsupported
    assert group(p(), p(512), vo(*([0] * 65)), 65, 2, 0.2, 50, p(1024), p(1100), p(1200), None) == unsupported
    assert group(p(), p(512), vo(1, 0, 1), 3, 2, 0.2, 50, p(1024), p(1100), p(1200), None) == bad
    assert group(p(), p(512), None, 3, 2, 0.2, 50, p(1024), p(1100), p(1200), None) == bad
    assert group(p(), p(512), vo(0, 1, 1), 3, 2, -1.0, 50, p(1024), p(1100), p(1200), None) == bad
    assert group(p(), p(512), vo(0, 1, 1), 3, 2, float("nan"), 50, p(1024), p(1100), p(1200), None) == bad
    assert group(p(), p(512), vo(0, 1, 1), 3, 2, 0.2, 0, p(1024), p(1100), p(1200), None) == bad
    assert group(None, p(512), vo(0, 1, 1), 3, 2, 0.2, 50, p(1024), p(1100), p(1200), None) == bad
    assert group(p(), None, vo(0, 1, 1), 3, 2, 0.2, 50, p(1024), p(1100), p(1200), None) == bad
    assert group(p(), p(512), vo(0, 1, 1), 3, 2, 0.2, 50, None, p(1100), p(1200), None) == bad
    assert group(p(), p(512), vo(0, 1, 1), 3, 2, 0.2, 50, p(1024), None, p(1200), None) == bad
    assert group(p(), p(512), vo(0, 1, 1), 3, 2, 0.2, 50, p(1024), p(1100), None, None) == bad
    assert group(p(4), p(512), vo(0, 1, 1), 3, 2, 0.2, 50, p(1024), p(1100), p(1200), None) == bad
    assert group(p(), p(514), vo(0, 1, 1), 3, 2, 0.2, 50, p(1024), p(1100), p(1200), None) == bad
    gather = lib.uu3d_gather_view_tracks
    #    src, poses, kp2d, flags, views, persons, frames, J, tracks, out_poses, out_kp2d, out_flags, stream
    assert gather(p(), p(512), p(1024), None, 9, 2, 4, 17, 3, p(2048), p(3072), p(4000), None) == unsupported
    assert gather(p(), p(512), p(1024), None, 2, 65, 4, 17, 3, p(2048), p(3072), p(4000), None) == unsupported
    assert gather(p(), p(512), p(1024), None, 2, 2, 4, 65, 3, p(2048), p(3072), p(4000), None) == unsupported
    assert gather(p(), p(512), p(1024), None, 2, 2, 4, 17, 65, p(2048), p(3072), p(4000), None) == unsupported
    assert gather(p(), p(512), p(1024), None, 0, 2, 4, 17, 3, p(2048), p(3072), p(4000), None) == bad
    assert gather(p(), p(512), p(1024), None, 2, 0, 4, 17, 3, p(2048), p(3072), p(4000), None) == bad
    assert gather(p(), p(512), p(1024), None, 2, 2, 0, 17, 3, p(2048), p(3072), p(4000), None) == bad
    assert gather(p(), p(512), p(1024), None, 2, 2, 4, 0, 3, p(2048), p(3072), p(4000), None) == bad
    assert gather(p(), p(512), p(1024), None, 2, 2, 4, 17, 0, p(2048), p(3072), p(4000), None) == bad
    assert gather(p(), p(512), p(1024), None, 2, 2, 2 ** 31, 17, 3, p(2048), p(3072), p(4000), None) == bad
    assert gather(None, p(512), p(1024), None, 2, 2, 4, 17, 3, p(2048), p(3072), p(4000), None) == bad
    assert gather(p(), None, p(1024), None, 2, 2, 4, 17, 3, p(2048), p(3072), p(4000), None) == bad
    assert gather(p(), p(512), None, None, 2, 2, 4, 17, 3, p(2048), p(3072), p(4000), None) == bad
    assert gather(p(), p(512), p(1024), None, 2, 2, 4, 17, 3, None, p(3072), p(4000), None) == bad
    assert gather(p(), p(512), p(1024), None, 2, 2, 4, 17, 3, p(2048), None, p(4000), None) == bad
    assert gather(p(), p(512), p(1024), None, 2, 2, 4, 17, 3, p(2048), p(3072), None, None) == bad
    assert gather(p(), p(512), p(1024), None, 2, 2, 4, 17, 3, p(512), p(3072), p(4000), None) == bad       # in place
    assert gather(p(), p(512), p(1028), None, 2, 2, 4, 17, 3, p(2048), p(3072), p(4000), None) == bad
    assert gather(p(2), p(512), p(1024), None, 2, 2, 4, 17, 3, p(2048), p(3072), p(4000), None) == bad
