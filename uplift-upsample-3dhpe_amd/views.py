"""The multi-view stage of the track pipeline: several calibrated cameras, one scene (include/uu3d.h, SEVERAL VIEWS).  Wraps
uu3d_fuse_views (``fuse_views``; the rule in numpy: ``fuse_views_host``) and uu3d_solve_view_roots (``solve_view_roots``;
``solve_view_roots_host``); ``predict_views`` is the call that runs V views of the same persons through one pipeline.

Several views -- ``predict_views(model, config, views, cameras)``: ``Camera(orientation=, translation=)`` puts every camera's output into
one world frame, but two cameras that see the same person still return two scenes, each with its own monocular root, and the model's scale
error goes 1:1 into each depth.  With V time-synchronised views of the same persons (``views[v][i]``: person i in camera v; the same index
is the same person, and person i has the same number of frames in every view) the call
  1. runs all V N tracks, view-major, through ONE front, ONE set of forwards and ONE assembly (``predict._assembled_tracks``, the part of
     ``predict_tracks`` up to uu3d_assemble_tracks: all views share batches),
  2. takes every view's poses to world axes (uu3d_camera_to_world, poses only, one row of extrinsics per view block),
  3. FUSES them per frame, joint and channel: the float64 mean over the views that SEE the frame, rounded once (uu3d_fuse_views),
  4. runs ``bones`` on the fused poses of the N persons (a mean of rigid skeletons is not rigid, so the fix comes behind the fusion),
  5. solves ONE world root per frame from all seeing views' used joints at once (uu3d_solve_view_roots: a 3 x 3 linear least-squares
     problem; with one view it is the monocular rule of ``solve_roots_host`` taken to world axes, in another algebra),
  6. joins each person's solved frames to a trajectory (uu3d_root_trajectory, unchanged) and runs ``smooth`` and ``rotations`` on the
     fused world scene, with the launches and in the order of ``predict_tracks``.
View v SEES frame f iff at least ``min_root_joints`` of its joints are USED there: the joint's flag is set and its raw coordinates are
finite; a joint ``repair_joints`` filled is not used, exactly as in uu3d_solve_roots.  A view that does not see a person at a frame
passes NaN coordinates (with ``valid="finite"``) or cleared flags there.

Who is who -- ``predict_views(..., match=True)`` / ``match_views(views, cameras)``: every camera's tracker numbers people in the order it
meets them, so the same index is NOT the same person.  With ``match`` the views may hold different numbers of tracks in any order (all of
one length T, on one clock -- see ``align`` below for cameras that are not), and in front of everything above
  0a. uu3d_view_pair_sums measures every pair of tracks of different views: the mean squared distance between the LINES through the two
      cameras and the pixels of the same joint at the same frame, in float64 with a fixed order of summation (``view_pair_sums_host``),
  0b. uu3d_group_views groups the tracks to persons, greedily and view by view (``group_views_host``),
  0c. ONE small copy tells the host who is who (it shapes every buffer behind it), all M tracks run through the one front as given -- no
      forward is spent on a view that did not see a person --, and uu3d_gather_view_tracks lays the world poses, keypoints and flags out
      per person, view-major; a (view, person) pair without a track is NaN keypoints and cleared flags, which the fusion does not SEE.
The lines are not half-lines (a meeting point behind a camera is not rejected), the grouping depends on the order of the views, and
``MATCH_DEFAULTS`` are conveniences for metres, not tuned values: no matching accuracy is claimed.

One clock -- ``predict_views(..., align=True)`` / ``align_views(views, cameras)`` / ``crop_views``: cameras started by hand are seconds
apart, so frame f of one view is not frame f of another.  With ``align`` every view has its own length and clock, and in front of
everything above
  -a. uu3d_view_lag_sums sums the same squared line distance for every track of the reference view (the first non-empty one), every
      track of a later view and every lag in -L .. L, after writing every joint's ray once (``view_lag_sums_host``),
  -b. uu3d_view_offsets takes, per view, the lag of the smallest mean (``view_offsets_host``),
  -c. ONE small copy (2 V int32) tells the host the offsets, and ``crop_views`` slices every view to the common time window.
Whole frames, against the reference view only, one common frame rate; ``ALIGN_DEFAULTS`` are conveniences, not tuned values: no alignment
accuracy is claimed.

Where rays meet -- ``predict_views(..., triangulate=True)`` / ``triangulate_joints`` / ``place_joints``: the fused pose of step 3 is a
mean of V monocular lifts, and the model's scale and depth errors, which all views share, stay in it.  With ``triangulate``, directly
behind the fusion and in front of ``bones``,
  3a. uu3d_triangulate_joints solves every joint that at least ``min_views`` seeing cameras observed from their rays alone: two weighted
      3 x 3 solves per round, the view of the largest reprojection residual dropped between rounds until all that remain agree within
      ``max_residual`` pixels (``triangulate_joints_host``),
  3b. uu3d_place_joints writes the HYBRID pose: X_j - X_root where both are triangulated, the fused lift's bits for every other joint --
      one camera saw it, the frame's root joint is lost, one camera saw the person (``place_joints_host``).
Everything behind (``bones``, the root solve, the trajectory, ``smooth``, ``rotations``) runs unchanged on that pose, and ``joint_views``
says per frame and joint how many cameras placed it (0: the lift).  With two views an error along the epipolar line cannot be seen; with
three views and an outlier the honest view can be the one dropped; the lines are lines apart from the z > 0 test; a kept lifted joint
stays relative to the root, not to its triangulated parent, so bones across the seam can stretch (``bones`` fixes lengths behind the
stage).  ``TRIANGULATE_DEFAULTS`` are conveniences, not tuned values.

Where the cameras stand -- ``predict_views(..., calibrate=True)`` / ``calibrate_views`` / ``calibrated_cameras``: everything above needs
every camera's extrinsics, and nobody who puts two phones and a webcam on tripods has them.  With ``calibrate`` cameras 1 .. V - 1 come
without extrinsics (camera 0 may keep its own, which then define the world; without, the world is camera 0's own space), and behind step
1, in front of step 2,
  1a. uu3d_view_moment_sums sums p_v (x) p_0 over the rows view 0 and view v both see -- every view's lift is the same skeleton in that
      camera's own axes, so the rotation between two cameras is the rotation between their lifts (``view_moment_sums_host``),
  1b. uu3d_solve_view_pose takes the quaternion from Horn's 4 x 4 matrix by a fixed number of Jacobi sweeps (``solve_view_pose_host``),
  1c. uu3d_view_position_sums adds, per row, both cameras' normal equations of the root solve with the row's unknown root eliminated --
      the rays and the lifts' metric size fix where the second camera stands (``view_position_sums_host``),
  1d. uu3d_solve_view_pose, its second stage, solves the 3 x 3 system for the position,
  1e. ONE small copy (V x 9 float64: quaternion, position, state, terms) tells the host the poses: ``Camera`` is a host object, and every
      buffer behind it is shaped by it.
The rig comes out at the MODEL's scale: lifts scaled by s put every camera s times too far away, and ``bones`` with known lengths, which
runs behind the stage, does not rescale it.  Calibration is against view 0 only, without chaining through a third camera; every term has
unit weight in an algebraic error, so near and far frames count alike; a person who only stands still fixes the position poorly; the
view-dependent depth errors of real lifts are not modelled.  ``VIEW_CALIBRATE_DEFAULTS`` is a convenience, not a tuned value.

Who is who without a world -- ``predict_views(..., match=MatchLifts(...))`` / ``match_lifts`` / ``lift_pair_sums``: ``match=True`` compares
pixel rays in world axes, and cameras that ``calibrate`` has yet to place share no world.  Matching does not need rays: every view's lift
is the same skeleton in that camera's own axes, so two tracks of different views are the same person iff their lifts agree up to ONE
rotation over the whole track.  With a ``MatchLifts``, with or without ``calibrate``, the M tracks run through the one front as given, and
  1'. uu3d_lift_pair_sums sums, per pair of tracks of different views and over the frames both see, p (x) q, |p|^2 + |q|^2 and the frames;
      Horn's largest eigenvalue (the Jacobi sweeps of step 1b) gives the squared joint distance left after the best common rotation in
      closed form (``lift_pair_sums_host``),
  2'. uu3d_group_views groups the tracks as in step 0b, ``min_terms`` counting frames, and the ONE copy of step 0c tells the host,
  3'. uu3d_gather_view_tracks lays the lifts out per person while they are still in camera axes; ``calibrate`` then runs steps 1a to 1e
      on those buffers -- a (view, person) pair without a track is rows the view does not SEE --, and the lifts go to world axes.
Two persons with one body who move alike cannot be told apart, and short or noisy tracks close the gap between a true and a wrong pair;
``LIFT_MATCH_DEFAULTS`` are conveniences for metres and frames, not tuned values: no matching accuracy is claimed.

Out of scope: estimating ``align`` without a world, sub-frame offsets and per-camera frame rates, per-view confidence weights, rescaling a calibrated rig to known lengths,
calibration chained through a third camera, estimating intrinsics, command-line flags.  The live form of the fusion and the root solve is ``StreamSession(views=V)`` (``live_views.py``); ``match``, ``align``, ``triangulate`` and ``calibrate`` have none.  No accuracy is claimed."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import ptr as _ptr
from .camera import Camera, _rotate_f64, camera_to_world_rows, undistort_rows
from .roots import DEFAULT_MIN_ROOT_JOINTS, MAX_ROOT_JOINTS, check_min_root_joints
from .tracks import _device_tracks, _host_array, _shape, _upload

MAX_VIEWS = 8                                                          # kViewsMax
VIEW_RANK = 2.0 ** -40                                                 # kViewRank
MAX_MATCH_TRACKS = 64                                                  # kMatchMaxTracks: the tracks of all views together
MATCH_LANES = 256                                                      # kMatchLanes: part of the rule's order of summation
VIEW_PARALLEL = 2.0 ** -20                                             # kViewParallel: sin^2 of 1e-3 rad -- closer rays carry no distance information
MATCH_DEFAULTS = dict(max_dist=0.2, min_terms=50)                      # conveniences for metres, not tuned values
MAX_ALIGN_LAG = 512                                                    # kAlignMaxLag: the largest clock offset looked for, in frames
ALIGN_DEFAULTS = dict(max_lag=50, min_terms=50)                        # conveniences for 50 Hz and metres, not tuned values
MIN_TRIANGULATE_VIEWS = 2                                              # kTriangulateMinViews: two lines meet in a point, one does not
TRIANGULATE_DEFAULTS = dict(max_residual=8.0, min_views=2)             # pixels of the tracks as given; conveniences, not tuned values
VIEW_CALIBRATE_DEFAULTS = dict(min_terms=50)                           # rows view 0 and a view must both see; a convenience, not a tuned value
CALIBRATE_CHUNK = 4096                                                 # kCalibrateChunk: rows per workgroup, part of the rule's order of summation
CALIBRATE_SUMS = 10                                                    # kCalibrateSums: nine sums and the number of terms per (view, chunk)
CALIBRATE_SWEEPS = 10                                                  # kCalibrateSweeps: cyclic Jacobi sweeps of the 4 x 4, no early exit
CALIBRATE_POSE = 8                                                     # kCalibratePose: the quaternion, the position, the state
CALIBRATE_GAP = 2.0 ** -20                                             # kCalibrateGap: the two largest eigenvalues must differ by this share
LIFT_MATCH_DEFAULTS = dict(max_dist=0.1, min_terms=50)                 # metres and frames; conveniences, not tuned values
LIFT_PAIR_SUMS = 11                                                    # kLiftPairSums: nine moment products, the squared size, 1.0


def check_view_cameras(cameras, views=None):
    """``cameras`` of the multi-view calls -> the list of V ``Camera`` objects, each with extrinsics (with or without distortion), one per
    view.  Anything else -- no list, a plain tuple among them, a ``Camera`` without extrinsics, another count than ``views`` -- is a
    ValueError."""
    if not isinstance(cameras, (list, tuple)) or not all(isinstance(c, Camera) for c in cameras):
        raise ValueError("cameras must be a list of Camera objects with extrinsics, one per view, not plain (fx, fy, cx, cy) tuples or a mix")
    if not 1 <= len(cameras) <= MAX_VIEWS:
        raise ValueError(f"cameras: between 1 and {MAX_VIEWS} views are taken, got {len(cameras)}")
    if not all(c.has_extrinsics for c in cameras):
        raise ValueError("cameras: every view's Camera needs extrinsics (orientation=, translation=): the views meet in the world frame")
    if views is not None and len(cameras) != int(views):
        raise ValueError(f"cameras must hold one Camera per view ({int(views)}), got {len(cameras)}")
    return list(cameras)


def view_rows(cameras):
    """The (V, 16) float64 rows of uu3d_solve_view_roots: fx, fy, cx, cy, then the camera's axes in world coordinates r1, r2, r3 -- the
    rotation of WORLD SPACE (``camera._rotate_f64``) applied to e_1, e_2, e_3 on the normalised quaternion --, then its position t."""
    rows = []
    one, zero = np.float64(1.0), np.float64(0.0)
    for c in check_view_cameras(cameras):
        q = [np.float64(v) for v in c.orientation]
        axes = [np.array(_rotate_f64(q, *e), np.float64) for e in ((one, zero, zero), (zero, one, zero), (zero, zero, one))]
        rows.append(np.concatenate([np.asarray(c.intrinsics, np.float64), *axes, np.asarray(c.translation, np.float64)]))
    return np.ascontiguousarray(np.stack(rows))


def _view_arrays(poses, kp2d, flags, fused):
    """The host arrays of a mirror, checked: ``poses`` (V, R, J, 3) -- ``fused``: (R, J, 3) --, ``kp2d`` (V, R, J, 2), ``flags`` None or
    (V, R, J) -> (poses f32, kp2d f32, used (V, R, J) bool)."""
    P = np.asarray(_host_array(poses), np.float32)
    uv = np.asarray(_host_array(kp2d), np.float32)
    if uv.ndim != 4 or uv.shape[3] != 2 or not 1 <= uv.shape[0] <= MAX_VIEWS or not 1 <= uv.shape[2] <= MAX_ROOT_JOINTS:
        raise ValueError(f"kp2d must be (V, R, J, 2) with V <= {MAX_VIEWS} and J <= {MAX_ROOT_JOINTS}, got {uv.shape}")
    want = uv.shape[1:3] + (3,) if fused else uv.shape[:3] + (3,)
    if P.shape != want:
        raise ValueError(f"poses must be {want} beside kp2d {uv.shape}, got {P.shape}")
    used = np.isfinite(uv).all(axis=3)
    if flags is not None:
        f = np.asarray(_host_array(flags)) != 0
        if f.shape != uv.shape[:3]:
            raise ValueError(f"flags must be {uv.shape[:3]}, got {f.shape}")
        used &= f
    return P, uv, used


def fuse_views_host(poses, kp2d, flags=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS):
    """The fusion rule of SEVERAL VIEWS (include/uu3d.h) in numpy, written to be read: what uu3d_fuse_views computes, bit for bit.
    ``poses`` (V, R, J, 3): every view's pose of every frame in world axes (read as float32); ``kp2d`` (V, R, J, 2): the raw 2D keypoints
    in the model's layout; ``flags``: None or (V, R, J), non-zero = the joint was observed
    -> (fused (R, J, 3) float32, view_count (R,) uint8, sees (V, R) uint8).
    A joint is USED iff its flag is set and both coordinates are finite; view v SEES frame f iff at least ``min_root_joints`` joints are
    used there.  Per frame, joint and channel, in float64: s = 0.0; for v ascending over the seeing views s = s + pose_v; the result is
    float32(s / n), n the number of seeing views = ``view_count``.  No view sees the frame: the same mean over ALL views, ``view_count`` 0.
    The root joint's zeros stay +0.0; NaN in, NaN out."""
    P, uv, used = _view_arrays(poses, kp2d, flags, False)
    m = check_min_root_joints(min_root_joints)
    V, R = P.shape[:2]
    sees = used.sum(axis=2) >= m                                        # (V, R)
    count = sees.sum(axis=0)                                            # (R,)
    take = np.where(count[None] > 0, sees, True)
    n = np.where(count > 0, count, V).astype(np.float64)
    s = np.zeros(P.shape[1:], np.float64)
    with np.errstate(all="ignore"):
        for v in range(V):
            s = np.where(take[v][:, None, None], s + P[v].astype(np.float64), s)
        fused = (s / n[:, None, None]).astype(np.float32)
    return fused, count.astype(np.uint8), sees.astype(np.uint8)


def solve_view_roots_host(poses, kp2d, cameras, flags=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS):
    """The root rule of SEVERAL VIEWS (include/uu3d.h) in numpy, written to be read: what uu3d_solve_view_roots computes, bit for bit.
    ``poses`` (R, J, 3): the fused world pose of every frame, root-relative (read as float32); ``kp2d`` (V, R, J, 2) and ``flags`` as
    ``fuse_views_host`` takes them; ``cameras``: V ``Camera`` objects with extrinsics
    -> (roots (R, 3) float64 in world coordinates, solved (R,) bool); the root of a frame that is not solved is zeros.
    Everything in float64, every operation rounded once.  Per view a row of ``view_rows``: fx, fy, cx, cy, the camera's axes in world
    coordinates r1, r2, r3 and its position t.  Over the seeing views in ascending order and their used joints in ascending order, with
    P_j the fused pose:
        a = (u - cx) / fx;  b = (v - cy) / fy;  n = r1 - a r3;  m = r2 - b r3;  d = t - P_j
        e = (n0 d0 + n1 d1) + n2 d2;  g = (m0 d0 + m1 d1) + m2 d2
        A_ik += (n_i n_k + m_i m_k) for ik = 00, 01, 02, 11, 12, 22;  B_i += (n_i e + m_i g)
    -- the normal equations of n . (T + P_j - t) = 0 and m . (T + P_j - t) = 0: the joint lies on the ray of its pixel --, solved by
    cofactors:
        c00 = A11 A22 - A12 A12;  c01 = A02 A12 - A01 A22;  c02 = A01 A12 - A02 A11
        c11 = A00 A22 - A02 A02;  c12 = A01 A02 - A00 A12;  c22 = A00 A11 - A01 A01
        det = (A00 c00 + A01 c01) + A02 c02
        x0 = (c00 B0 + c01 B1) + c02 B2;  x1 = (c01 B0 + c11 B1) + c12 B2;  x2 = (c02 B0 + c12 B1) + c22 B2;  T_i = x_i / det
    SOLVED iff at least one view sees the frame, det is finite and > 0, det > ``VIEW_RANK`` * ((A00 A11) A22), T is finite, and every
    used joint of every seeing view lies in front of its camera: with w = (T + P_j) - t, (r3_0 w0 + r3_1 w1) + r3_2 w2 > 0.
    The RANK GUARD: when all rays are one ray -- a single seeing view whose used joints share one pixel -- A has rank 2 and det is zero in
    exact arithmetic, but in float64 it is rounding noise of either sign, about 2^-52 of Hadamard's bound A00 A11 A22 (every cofactor is a
    difference of two rounded products of that size): ``det > 0`` alone would pass half of such frames with a root metres away.
    ``VIEW_RANK`` = 2^-40 stands 4000 times above that noise; a real person seen by one camera from 4 m gives 4e-3 or more of the bound,
    two views 0.4 or more."""
    P, uv, used = _view_arrays(poses, kp2d, flags, True)
    m_ = check_min_root_joints(min_root_joints)
    V, R, J = uv.shape[:3]
    cam = view_rows(check_view_cameras(cameras, V))
    sees = used.sum(axis=2) >= m_
    P64, uv64 = P.astype(np.float64), uv.astype(np.float64)
    a00, a01, a02, a11, a12, a22, b0, b1, b2 = (np.zeros(R, np.float64) for _ in range(9))
    with np.errstate(all="ignore"):
        for v in range(V):
            fx, fy, cx, cy = cam[v, :4]
            r1, r2, r3, t = cam[v, 4:7], cam[v, 7:10], cam[v, 10:13], cam[v, 13:16]
            for j in range(J):
                a = (uv64[v, :, j, 0] - cx) / fx
                b = (uv64[v, :, j, 1] - cy) / fy
                n0, n1, n2 = r1[0] - a * r3[0], r1[1] - a * r3[1], r1[2] - a * r3[2]
                m0, m1, m2 = r2[0] - b * r3[0], r2[1] - b * r3[1], r2[2] - b * r3[2]
                d0, d1, d2 = t[0] - P64[:, j, 0], t[1] - P64[:, j, 1], t[2] - P64[:, j, 2]
                e = (n0 * d0 + n1 * d1) + n2 * d2
                g = (m0 * d0 + m1 * d1) + m2 * d2
                u = sees[v] & used[v, :, j]
                a00 = np.where(u, a00 + (n0 * n0 + m0 * m0), a00)
                a01 = np.where(u, a01 + (n0 * n1 + m0 * m1), a01)
                a02 = np.where(u, a02 + (n0 * n2 + m0 * m2), a02)
                a11 = np.where(u, a11 + (n1 * n1 + m1 * m1), a11)
                a12 = np.where(u, a12 + (n1 * n2 + m1 * m2), a12)
                a22 = np.where(u, a22 + (n2 * n2 + m2 * m2), a22)
                b0 = np.where(u, b0 + (n0 * e + m0 * g), b0)
                b1 = np.where(u, b1 + (n1 * e + m1 * g), b1)
                b2 = np.where(u, b2 + (n2 * e + m2 * g), b2)
        c00 = a11 * a22 - a12 * a12
        c01 = a02 * a12 - a01 * a22
        c02 = a01 * a12 - a02 * a11
        c11 = a00 * a22 - a02 * a02
        c12 = a01 * a02 - a00 * a12
        c22 = a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        x0 = (c00 * b0 + c01 * b1) + c02 * b2
        x1 = (c01 * b0 + c11 * b1) + c12 * b2
        x2 = (c02 * b0 + c12 * b1) + c22 * b2
        T0, T1, T2 = x0 / det, x1 / det, x2 / det
        solved = sees.any(axis=0) & np.isfinite(det) & (det > 0) & (det > VIEW_RANK * ((a00 * a11) * a22))
        solved &= np.isfinite(T0) & np.isfinite(T1) & np.isfinite(T2)
        for v in range(V):                                              # every used joint of every seeing view in front of its camera
            r3, t = cam[v, 10:13], cam[v, 13:16]
            for j in range(J):
                w0 = (T0 + P64[:, j, 0]) - t[0]
                w1 = (T1 + P64[:, j, 1]) - t[1]
                w2 = (T2 + P64[:, j, 2]) - t[2]
                z = (r3[0] * w0 + r3[1] * w1) + r3[2] * w2
                solved &= ~(sees[v] & used[v, :, j]) | (z > 0)
    roots = np.zeros((R, 3), np.float64)
    roots[solved] = np.stack([T0, T1, T2], axis=1)[solved]
    return roots, solved


def _view_tensors(poses, kp2d, flags, fused):
    """The device tensors of a launch, checked -> (V, R, J, flags as uint8 or None)."""
    import torch
    if not isinstance(kp2d, torch.Tensor) or not kp2d.is_cuda or kp2d.dim() != 4 or kp2d.shape[3] != 2 or kp2d.dtype != torch.float32 or not kp2d.is_contiguous():
        raise ValueError(f"kp2d must be a contiguous (V, R, J, 2) float32 device tensor, got {tuple(getattr(kp2d, 'shape', ()))}")
    V, R, J = (int(n) for n in kp2d.shape[:3])
    if not 1 <= V <= MAX_VIEWS or not 1 <= J <= MAX_ROOT_JOINTS:
        raise ValueError(f"between 1 and {MAX_VIEWS} views and 1 and {MAX_ROOT_JOINTS} joints are taken, got {V} and {J}")
    want = (R, J, 3) if fused else (V, R, J, 3)
    if not isinstance(poses, torch.Tensor) or tuple(poses.shape) != want or poses.dtype != torch.float32 or not poses.is_contiguous() or poses.device != kp2d.device:
        raise ValueError(f"poses must be a contiguous {want} float32 tensor on kp2d's device, got {tuple(getattr(poses, 'shape', ()))}")
    if flags is not None:
        if not isinstance(flags, torch.Tensor) or tuple(flags.shape) != (V, R, J) or flags.dtype not in (torch.uint8, torch.bool) or not flags.is_contiguous() \
                or flags.device != kp2d.device:
            raise ValueError(f"flags must be a contiguous ({V}, {R}, {J}) uint8 or bool tensor on kp2d's device")
        flags = flags.view(torch.uint8)
    return V, R, J, flags


def fuse_views(poses, kp2d, flags=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS):
    """uu3d_fuse_views on the current stream: ``fuse_views_host`` on device tensors, one launch, nothing copies to the host or waits.
    ``poses`` (V, R, J, 3) float32 and ``kp2d`` (V, R, J, 2) float32 on the device, contiguous (only read); ``flags`` (V, R, J) uint8 /
    bool on the device or None -> (fused (R, J, 3) float32, view_count (R,) uint8, sees (V, R) uint8), fresh device buffers.  Needs no
    model."""
    import torch
    lib = _capi.load_library()
    V, R, J, flags = _view_tensors(poses, kp2d, flags, False)
    m = check_min_root_joints(min_root_joints)
    dev = kp2d.device
    fused = torch.empty((R, J, 3), dtype=torch.float32, device=dev)
    count = torch.empty((R,), dtype=torch.uint8, device=dev)
    sees = torch.empty((V, R), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_fuse_views(_ptr(poses), _ptr(kp2d), _ptr(flags), V, R, J, m, _ptr(fused), _ptr(count), _ptr(sees),
                                             C.c_void_p(stream)), None)
    return fused, count, sees


def solve_view_roots(poses, kp2d, cameras, flags=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS):
    """uu3d_solve_view_roots on the current stream: ``solve_view_roots_host`` on device tensors, one launch, nothing copies to the host or
    waits (the V camera rows go up pinned and asynchronously).  ``poses`` (R, J, 3) float32: the fused world poses; ``kp2d`` / ``flags``
    as ``fuse_views`` takes them; ``cameras``: V ``Camera`` objects with extrinsics -> (roots (R, 3) float64, solved (R,) bool), fresh
    device buffers: what ``root_trajectory`` takes.  Needs no model."""
    import torch
    lib = _capi.load_library()
    V, R, J, flags = _view_tensors(poses, kp2d, flags, True)
    m = check_min_root_joints(min_root_joints)
    dev = kp2d.device
    cams = _upload(view_rows(check_view_cameras(cameras, V)), np.float64, dev)
    roots = torch.empty((R, 3), dtype=torch.float64, device=dev)
    solved = torch.empty((R,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_solve_view_roots(_ptr(poses), _ptr(kp2d), _ptr(flags), V, R, J, _ptr(cams), m, _ptr(roots), _ptr(solved),
                                                   C.c_void_p(stream)), None)
    return roots, solved.view(torch.bool)


# ---- where rays meet: joints placed by geometry where two or more cameras agree (include/uu3d.h, WHERE RAYS MEET) ------------------------
class Triangulate(object):
    """The parameters of ``predict_views(triangulate=...)`` / ``triangulate_joints``: ``max_residual``, the largest reprojection error, in
    pixels of the tracks as given, a view may show at a triangulated joint (finite, > 0), and ``min_views``, the least number of cameras
    that must agree on a joint (an int in 2 .. 8).  The defaults are conveniences, not tuned values."""

    def __init__(self, max_residual=TRIANGULATE_DEFAULTS["max_residual"], min_views=TRIANGULATE_DEFAULTS["min_views"]):
        self.max_residual, self.min_views = _triangulate_parameters(max_residual, min_views)

    def __repr__(self):
        return f"Triangulate(max_residual={self.max_residual!r}, min_views={self.min_views!r})"


def _triangulate_parameters(max_residual, min_views):
    try:
        r = float(max_residual)
    except (TypeError, ValueError):
        raise ValueError(f"max_residual must be a finite number > 0, got {max_residual!r}") from None
    if isinstance(max_residual, bool) or not np.isfinite(r) or not r > 0:
        raise ValueError(f"max_residual must be a finite number > 0, got {max_residual!r}")
    if isinstance(min_views, bool) or not isinstance(min_views, (int, np.integer)) or not MIN_TRIANGULATE_VIEWS <= int(min_views) <= MAX_VIEWS:
        raise ValueError(f"min_views must be an int in {MIN_TRIANGULATE_VIEWS} .. {MAX_VIEWS}, got {min_views!r}")
    return r, int(min_views)


def check_triangulate(triangulate):
    """``predict_views(triangulate=...)`` -> None (the fused lifts stay as they are) or a ``Triangulate``; True is the defaults."""
    if triangulate is None:
        return None
    if triangulate is True:
        return Triangulate()
    if not isinstance(triangulate, Triangulate):
        raise ValueError(f"triangulate must be None, True or a Triangulate(max_residual=, min_views=), got {triangulate!r}")
    return triangulate


def _check_root_joint(root, J):
    if isinstance(root, bool) or not isinstance(root, (int, np.integer)) or not 0 <= int(root) < J:
        raise ValueError(f"root must be a joint in 0 .. {J - 1}, got {root!r}")
    return int(root)


def _weighted_solve(uv64, cam, cand, q):
    """One pass of ``triangulate_joints_host``: ``uv64`` (V, R, J, 2), ``cam`` the ``view_rows``, ``cand`` (V, R, J) bool, ``q`` (V, R, J)
    -> (X (R, J, 3), accepted (R, J)).  The cofactor statements are those of ``solve_view_roots_host``, term for term."""
    a00, a01, a02, a11, a12, a22, b0, b1, b2 = (np.zeros(cand.shape[1:], np.float64) for _ in range(9))
    for v in range(cand.shape[0]):
        fx, fy, cx, cy = cam[v, :4]
        r1, r2, r3, t = cam[v, 4:7], cam[v, 7:10], cam[v, 10:13], cam[v, 13:16]
        a = (uv64[v, :, :, 0] - cx) / fx
        b = (uv64[v, :, :, 1] - cy) / fy
        n0, n1, n2 = (r1[0] - a * r3[0]) * q[v], (r1[1] - a * r3[1]) * q[v], (r1[2] - a * r3[2]) * q[v]
        m0, m1, m2 = (r2[0] - b * r3[0]) * q[v], (r2[1] - b * r3[1]) * q[v], (r2[2] - b * r3[2]) * q[v]
        e = (n0 * t[0] + n1 * t[1]) + n2 * t[2]
        g = (m0 * t[0] + m1 * t[1]) + m2 * t[2]
        u = cand[v]
        a00 = np.where(u, a00 + (n0 * n0 + m0 * m0), a00)
        a01 = np.where(u, a01 + (n0 * n1 + m0 * m1), a01)
        a02 = np.where(u, a02 + (n0 * n2 + m0 * m2), a02)
        a11 = np.where(u, a11 + (n1 * n1 + m1 * m1), a11)
        a12 = np.where(u, a12 + (n1 * n2 + m1 * m2), a12)
        a22 = np.where(u, a22 + (n2 * n2 + m2 * m2), a22)
        b0 = np.where(u, b0 + (n0 * e + m0 * g), b0)
        b1 = np.where(u, b1 + (n1 * e + m1 * g), b1)
        b2 = np.where(u, b2 + (n2 * e + m2 * g), b2)
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    c11 = a00 * a22 - a02 * a02
    c12 = a01 * a02 - a00 * a12
    c22 = a00 * a11 - a01 * a01
    det = (a00 * c00 + a01 * c01) + a02 * c02
    x0 = (c00 * b0 + c01 * b1) + c02 * b2
    x1 = (c01 * b0 + c11 * b1) + c12 * b2
    x2 = (c02 * b0 + c12 * b1) + c22 * b2
    X = np.stack([x0 / det, x1 / det, x2 / det], axis=-1)
    accepted = np.isfinite(det) & (det > 0) & (det > VIEW_PARALLEL * ((a00 * a11) * a22)) & np.isfinite(X).all(axis=-1)
    return X, accepted


def _view_depths(X, cam):
    """z_v = (r3_0 w0 + r3_1 w1) + r3_2 w2 with w = X - t, for every view -> (z (V, R, J), w (V, R, J, 3))."""
    w = X[None] - cam[:, None, None, 13:16]
    r3 = cam[:, None, None, 10:13]
    return (r3[..., 0] * w[..., 0] + r3[..., 1] * w[..., 1]) + r3[..., 2] * w[..., 2], w


def triangulate_joints_host(kp2d, cameras, sees, flags=None, max_residual=TRIANGULATE_DEFAULTS["max_residual"],
                            min_views=TRIANGULATE_DEFAULTS["min_views"]):
    """The triangulation of WHERE RAYS MEET (include/uu3d.h) in numpy, written to be read: what uu3d_triangulate_joints computes, bit for
    bit.  ``kp2d`` (V, R, J, 2): the raw 2D keypoints in the model's layout, undistorted (read as float32); ``cameras``: V ``Camera``
    objects with extrinsics; ``sees`` (V, R): the third output of ``fuse_views_host``; ``flags``: None or (V, R, J)
    -> (X (R, J, 3) float64 in world coordinates, count (R, J) uint8: the cameras that agree on the joint, 0 = not triangulated, X zeros).
    Everything in float64, every operation rounded once; per view a row of ``view_rows``.  Per frame and joint the candidate set C holds
    the views that SEE the frame and in which the joint is USED (the definitions of ``fuse_views_host``).  A round:
      * fewer than ``min_views`` candidates: not triangulated.
      * pass 1, over the candidates in ascending order, with q_v = 1.0:
            a = (u - cx) / fx;  b = (v - cy) / fy;  n_i = (r1_i - a r3_i) q_v;  m_i = (r2_i - b r3_i) q_v
            e = (n0 t0 + n1 t1) + n2 t2;  g = (m0 t0 + m1 t1) + m2 t2
            A_ik += (n_i n_k + m_i m_k) for ik = 00, 01, 02, 11, 12, 22;  B_i += (n_i e + m_i g)
        -- n . (X - t) = 0 and m . (X - t) = 0: the joint lies on the line of its pixel --, solved by the cofactors of
        ``solve_view_roots_host``.  ACCEPTED iff det is finite and > 0, det > ``VIEW_PARALLEL`` * ((A00 A11) A22) and X is finite: 2^-20
        with the meaning it has in ``view_pair_sums_host`` -- rays closer than about 1e-3 rad carry no distance information; two
        coincident cameras give rounding noise, ring cameras 0.037 or more with three views and 0.49 with two.  With w = X - t,
        z_v = (r3_0 w0 + r3_1 w1) + r3_2 w2 must be > 0 for every candidate, else the joint is not triangulated: no view is dropped for
        lying behind.
      * pass 2: the same statements with q_v = 1.0 / z_v -- the depth-weighted algebraic error becomes one in normalised image units --,
        the same guards, z_v from the new X.
      * the residual per candidate: xc = (r1_0 w0 + r1_1 w1) + r1_2 w2, yc with r2; du = |(fx (xc / z_v) + cx) - u|, dv likewise;
        rho_v = max(du, dv), +inf if either is NaN.
      * every rho_v <= ``max_residual``: triangulated, X with count = |C|.  Otherwise the view of the largest rho_v leaves C (ties: the
        larger view index) and the next round runs.
    At most V - min_views + 1 rounds of exactly two passes, without an early exit (the spirit of ``Camera.ITERATIONS``).  With exactly
    two views an error along the epipolar line cannot be seen; the lines are lines apart from the z > 0 test."""
    uv = np.asarray(_host_array(kp2d), np.float32)
    if uv.ndim != 4 or uv.shape[3] != 2 or not 1 <= uv.shape[0] <= MAX_VIEWS or not 1 <= uv.shape[2] <= MAX_ROOT_JOINTS:
        raise ValueError(f"kp2d must be (V, R, J, 2) with V <= {MAX_VIEWS} and J <= {MAX_ROOT_JOINTS}, got {uv.shape}")
    V, R, J = uv.shape[:3]
    max_residual, min_views = _triangulate_parameters(max_residual, min_views)
    cam = view_rows(check_view_cameras(cameras, V))
    S = np.asarray(_host_array(sees)) != 0
    if S.shape != (V, R):
        raise ValueError(f"sees must be ({V}, {R}), got {S.shape}")
    used = np.isfinite(uv).all(axis=3)
    if flags is not None:
        f = np.asarray(_host_array(flags)) != 0
        if f.shape != (V, R, J):
            raise ValueError(f"flags must be ({V}, {R}, {J}), got {f.shape}")
        used &= f
    cand = used & S[:, :, None]
    uv64 = uv.astype(np.float64)
    X = np.zeros((R, J, 3), np.float64)
    count = np.zeros((R, J), np.uint8)
    open_ = np.ones((R, J), bool)                                        # neither triangulated nor given up
    with np.errstate(all="ignore"):
        for _ in range(V - min_views + 1):
            size = cand.sum(axis=0)
            open_ &= size >= min_views
            if not open_.any():
                break
            X1, ok = _weighted_solve(uv64, cam, cand, np.ones(cand.shape, np.float64))
            z, _ = _view_depths(X1, cam)
            ok &= (~cand | (z > 0)).all(axis=0)
            X2, ok2 = _weighted_solve(uv64, cam, cand, 1.0 / z)
            z, w = _view_depths(X2, cam)
            ok &= ok2 & (~cand | (z > 0)).all(axis=0)
            r1, r2 = cam[:, None, None, 4:7], cam[:, None, None, 7:10]
            xc = (r1[..., 0] * w[..., 0] + r1[..., 1] * w[..., 1]) + r1[..., 2] * w[..., 2]
            yc = (r2[..., 0] * w[..., 0] + r2[..., 1] * w[..., 1]) + r2[..., 2] * w[..., 2]
            du = np.abs((cam[:, None, None, 0] * (xc / z) + cam[:, None, None, 2]) - uv64[..., 0])
            dv = np.abs((cam[:, None, None, 1] * (yc / z) + cam[:, None, None, 3]) - uv64[..., 1])
            rho = np.where(np.isnan(du) | np.isnan(dv), np.inf, np.maximum(du, dv))
            rho = np.where(cand, rho, -1.0)                              # (the residuals are >= 0)
            fits = (rho <= max_residual).all(axis=0)
            done = open_ & ok & fits
            X[done], count[done] = X2[done], size[done]
            open_ &= ok & ~fits                                          # a refused solve or a joint behind a camera: given up
            drop = V - 1 - np.argmax(rho[::-1], axis=0)                  # the largest residual, ties to the larger view index
            cand &= ~(open_[None] & (np.arange(V)[:, None, None] == drop[None]))
    return X, count


def place_joints_host(fused, points, count, root=0):
    """The placement of WHERE RAYS MEET (include/uu3d.h) in numpy: what uu3d_place_joints computes, bit for bit.  ``fused`` (R, J, 3): the
    fused world pose of every frame, root-relative (read as float32); ``points`` (R, J, 3) float64 and ``count`` (R, J) of
    ``triangulate_joints_host``; ``root``: the root joint -> (placed (R, J, 3) float32, joint_views (R, J) uint8).
    Where both the joint and the frame's root joint are triangulated the pose is float32(X_j - X_root) per channel -- +0.0 for the root
    joint itself -- and joint_views is the joint's count; every other joint keeps the fused pose's bits, NaN included, and joint_views 0.
    A frame without a triangulated root joint stays lifted as a whole.  A kept lifted joint stays relative to the root, not to its
    triangulated parent: bones across the seam can stretch, and ``bones`` runs behind this stage."""
    P = np.ascontiguousarray(np.asarray(_host_array(fused), np.float32))
    X = np.asarray(_host_array(points), np.float64)
    n = np.asarray(_host_array(count), np.uint8)
    if P.ndim != 3 or P.shape[2] != 3 or not 1 <= P.shape[1] <= MAX_ROOT_JOINTS or X.shape != P.shape or n.shape != P.shape[:2]:
        raise ValueError(f"fused and points must be (R, J, 3) with J <= {MAX_ROOT_JOINTS} and count (R, J), got {P.shape}, {X.shape} and {n.shape}")
    root = _check_root_joint(root, P.shape[1])
    take = (n > 0) & (n[:, root] > 0)[:, None]
    with np.errstate(all="ignore"):
        moved = (X - X[:, root][:, None, :]).astype(np.float32)
    moved[:, root] = 0.0
    placed = np.where(take[:, :, None], moved, P)
    return placed, np.where(take, n, 0).astype(np.uint8)


def triangulate_joints(kp2d, cameras, sees, flags=None, max_residual=TRIANGULATE_DEFAULTS["max_residual"],
                       min_views=TRIANGULATE_DEFAULTS["min_views"]):
    """uu3d_triangulate_joints on the current stream: ``triangulate_joints_host`` on device tensors, one launch, nothing copies to the
    host or waits (the V camera rows go up pinned and asynchronously).  ``kp2d`` (V, R, J, 2) float32, ``sees`` (V, R) uint8 / bool and
    ``flags`` (V, R, J) uint8 / bool or None on the device, contiguous (only read) -> (X (R, J, 3) float64, count (R, J) uint8), fresh
    device buffers.  Needs no model."""
    import torch
    lib = _capi.load_library()
    if not _is_device(kp2d, torch.float32) or kp2d.dim() != 4 or kp2d.shape[3] != 2:
        raise ValueError(f"kp2d must be a contiguous (V, R, J, 2) float32 device tensor, got {tuple(getattr(kp2d, 'shape', ()))}")
    V, R, J = (int(n) for n in kp2d.shape[:3])
    if not 1 <= V <= MAX_VIEWS or not 1 <= J <= MAX_ROOT_JOINTS:
        raise ValueError(f"between 1 and {MAX_VIEWS} views and 1 and {MAX_ROOT_JOINTS} joints are taken, got {V} and {J}")
    dev = kp2d.device
    if not _is_device(sees, (torch.uint8, torch.bool), dev) or tuple(sees.shape) != (V, R):
        raise ValueError(f"sees must be a contiguous ({V}, {R}) uint8 or bool tensor on kp2d's device")
    if flags is not None and (not _is_device(flags, (torch.uint8, torch.bool), dev) or tuple(flags.shape) != (V, R, J)):
        raise ValueError(f"flags must be a contiguous ({V}, {R}, {J}) uint8 or bool tensor on kp2d's device")
    max_residual, min_views = _triangulate_parameters(max_residual, min_views)
    cams = _upload(view_rows(check_view_cameras(cameras, V)), np.float64, dev)
    X = torch.empty((R, J, 3), dtype=torch.float64, device=dev)
    count = torch.empty((R, J), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_triangulate_joints(_ptr(kp2d), _ptr(None if flags is None else flags.view(torch.uint8)), _ptr(sees.view(torch.uint8)),
                                                     V, R, J, _ptr(cams), min_views, max_residual, _ptr(X), _ptr(count), C.c_void_p(stream)), None)
    return X, count


def place_joints(fused, points, count, root=0):
    """uu3d_place_joints on the current stream: ``place_joints_host`` on device tensors, one launch, nothing copies to the host or waits.
    ``fused`` (R, J, 3) float32, ``points`` (R, J, 3) float64 and ``count`` (R, J) uint8 on the device, contiguous (only read)
    -> (placed (R, J, 3) float32, joint_views (R, J) uint8), fresh device buffers.  Needs no model."""
    import torch
    lib = _capi.load_library()
    if not _is_device(fused, torch.float32) or fused.dim() != 3 or fused.shape[2] != 3 or not 1 <= fused.shape[1] <= MAX_ROOT_JOINTS:
        raise ValueError(f"fused must be a contiguous (R, J, 3) float32 device tensor with J <= {MAX_ROOT_JOINTS}, got {tuple(getattr(fused, 'shape', ()))}")
    R, J = int(fused.shape[0]), int(fused.shape[1])
    dev = fused.device
    if not _is_device(points, torch.float64, dev) or tuple(points.shape) != (R, J, 3) or not _is_device(count, torch.uint8, dev) or tuple(count.shape) != (R, J):
        raise ValueError(f"points must be a contiguous ({R}, {J}, 3) float64 tensor and count a ({R}, {J}) uint8 one on fused's device")
    root = _check_root_joint(root, J)
    placed = torch.empty((R, J, 3), dtype=torch.float32, device=dev)
    joint_views = torch.empty((R, J), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_place_joints(_ptr(fused), _ptr(points), _ptr(count), R, J, root, _ptr(placed), _ptr(joint_views), C.c_void_p(stream)),
                    None)
    return placed, joint_views


# ---- where the cameras stand: every view's pose against view 0 from lifts and rays (include/uu3d.h, WHERE THE CAMERAS STAND) -------------
class CalibrateViews(object):
    """The parameter of ``predict_views(calibrate=...)`` / ``calibrate_views``: ``min_terms``, the least number of rows (frames) view 0
    and a view must both see for that view to be calibrated (an int >= 1).  The default is a convenience, not a tuned value."""

    def __init__(self, min_terms=VIEW_CALIBRATE_DEFAULTS["min_terms"]):
        self.min_terms = _calibrate_parameters(min_terms)

    def __repr__(self):
        return f"CalibrateViews(min_terms={self.min_terms!r})"


def _calibrate_parameters(min_terms):
    if isinstance(min_terms, (bool, np.bool_)) or not isinstance(min_terms, (int, np.integer)) or not 1 <= int(min_terms) < 2 ** 31:
        raise ValueError(f"min_terms must be an int >= 1, got {min_terms!r}")
    return int(min_terms)


def check_calibrate(calibrate):
    """``predict_views(calibrate=...)`` -> None (every camera comes with extrinsics) or a ``CalibrateViews``; True is the defaults."""
    if calibrate is None:
        return None
    if calibrate is True:
        return CalibrateViews()
    if not isinstance(calibrate, CalibrateViews):
        raise ValueError(f"calibrate must be None, True or a CalibrateViews(min_terms=), got {calibrate!r}")
    return calibrate


def check_calibrate_cameras(cameras, views=None):
    """``cameras`` of ``predict_views(calibrate=...)`` -> the list of V ``Camera`` objects: intrinsics, with or without distortion; camera 0
    with or without extrinsics (with: they define the world; without: the world is camera 0's own space), cameras 1 .. V - 1 WITHOUT --
    extrinsics on one of them is a ValueError that names it, since the call is there to find them."""
    if not isinstance(cameras, (list, tuple)) or not all(isinstance(c, Camera) for c in cameras):
        raise ValueError("calibrate: cameras must be a list of Camera objects (intrinsics, distortion or none), one per view, not plain "
                         "(fx, fy, cx, cy) tuples or a mix")
    if not 1 <= len(cameras) <= MAX_VIEWS:
        raise ValueError(f"cameras: between 1 and {MAX_VIEWS} views are taken, got {len(cameras)}")
    for v, c in enumerate(cameras):
        if v > 0 and c.has_extrinsics:
            raise ValueError(f"calibrate: camera {v} comes with extrinsics (orientation=, translation=); only camera 0 may, and they then define "
                             f"the world -- pass the others without, or call without calibrate")
    if views is not None and len(cameras) != int(views):
        raise ValueError(f"cameras must hold one Camera per view ({int(views)}), got {len(cameras)}")
    return list(cameras)


def _with_identity(camera):
    """A copy of ``camera`` that stands at the origin of the world and looks along its axes."""
    fx, fy, cx, cy = camera.intrinsics
    return Camera(fx, fy, cx, cy, distortion=camera.distortion, tol=camera.tol, orientation=(1.0, 0.0, 0.0, 0.0), translation=(0.0, 0.0, 0.0))


def calibrated_cameras(cameras, pose):
    """The cameras ``predict_views(calibrate=...)`` returns, on the host: ``cameras`` as ``check_calibrate_cameras`` takes them; ``pose``
    (V, 8) float64 of ``calibrate_views`` / ``calibrate_views_host`` (the state is not looked at) -> V ``Camera`` objects with extrinsics.
    Camera 0 without extrinsics: it gets the identity pose, and camera v orientation q_v and translation c_v as they are.  Camera 0 with
    extrinsics (q_0, t_0): it is returned as it is, and camera v gets the Hamilton product q_0 q_v, every component a sum of four products
    added left to right, and ``_rotate_f64(q_0, c_v) + t_0``, in float64.  ``Camera`` normalises the quaternion once more."""
    cams = check_calibrate_cameras(cameras)
    rows = np.asarray(_host_array(pose), np.float64)
    if rows.shape != (len(cams), 8):
        raise ValueError(f"pose must be ({len(cams)}, 8), got {rows.shape}")
    first = cams[0] if cams[0].has_extrinsics else _with_identity(cams[0])
    out = [first]
    for v in range(1, len(cams)):
        q, c = rows[v, :4], rows[v, 4:7]
        if cams[0].has_extrinsics:
            w0, x0, y0, z0 = (np.float64(a) for a in first.orientation)
            w1, x1, y1, z1 = q
            q = np.array([((w0 * w1 - x0 * x1) - y0 * y1) - z0 * z1, ((w0 * x1 + x0 * w1) + y0 * z1) - z0 * y1,
                          ((w0 * y1 - x0 * z1) + y0 * w1) + z0 * x1, ((w0 * z1 + x0 * y1) - y0 * x1) + z0 * w1], np.float64)
            c = np.array(_rotate_f64((w0, x0, y0, z0), c[0], c[1], c[2]), np.float64) + first.translation
        fx, fy, cx, cy = cams[v].intrinsics
        out.append(Camera(fx, fy, cx, cy, distortion=cams[v].distortion, tol=cams[v].tol, orientation=q, translation=c))
    return out


def _intrinsic_rows(cameras, V):
    """V ``Camera`` objects (any extrinsics), or their (V, 4) rows already -> (V, 4) float64: fx, fy, cx, cy."""
    if isinstance(cameras, np.ndarray):
        rows = np.ascontiguousarray(cameras, np.float64)
    else:
        if not isinstance(cameras, (list, tuple)) or not all(isinstance(c, Camera) for c in cameras):
            raise ValueError("cameras must be a list of Camera objects, one per view, or their (V, 4) rows fx, fy, cx, cy")
        rows = np.ascontiguousarray(np.array([c.intrinsics for c in cameras], np.float64).reshape(len(cameras), 4))
    if rows.shape != (V, 4):
        raise ValueError(f"cameras must hold one camera per view ({V}), got {rows.shape[0] if rows.ndim else 0}")
    return rows


def calibrate_chunks(rows):
    """The chunks of ``CALIBRATE_CHUNK`` rows the sums of WHERE THE CAMERAS STAND are cut into."""
    return (int(rows) + CALIBRATE_CHUNK - 1) // CALIBRATE_CHUNK


def _chunk_sums(values, term):
    """The order of summation of WHERE THE CAMERAS STAND: ``values`` (R, 10) float64, ``term`` (R,) bool -> (C, 10) float64.  Per chunk of
    4096 rows, lane l of 256 adds the values of the terms among its rows l, l + 256, ... ascending to 0.0, then the fixed tree."""
    R = values.shape[0]
    out = np.zeros((calibrate_chunks(R), CALIBRATE_SUMS), np.float64)
    for c in range(out.shape[0]):
        out[c] = _lane_sums(values[c * CALIBRATE_CHUNK:(c + 1) * CALIBRATE_CHUNK], term[c * CALIBRATE_CHUNK:(c + 1) * CALIBRATE_CHUNK])
    return out


def _lane_sums(values, term):
    """One workgroup's sums, shared by WHERE THE CAMERAS STAND (per chunk) and WHO IS WHO WITHOUT A WORLD (per pair): ``values`` (R, n)
    float64, ``term`` (R,) bool -> (n,) float64.  Lane l of 256 adds the values of the terms among its rows l, l + 256, ... ascending to
    0.0, then for stride = 128, 64, ..., 1: x[l] = x[l] + x[l + stride] for l < stride."""
    x = np.zeros((MATCH_LANES, values.shape[1]), np.float64)
    with np.errstate(all="ignore"):
        for first in range(0, values.shape[0], MATCH_LANES):
            part, t = values[first:first + MATCH_LANES], term[first:first + MATCH_LANES]
            x[:len(part)] = np.where(t[:, None], x[:len(part)] + part, x[:len(part)])
        stride = MATCH_LANES // 2
        while stride >= 1:                                               # the fixed tree
            x[:stride] = x[:stride] + x[stride:2 * stride]
            stride //= 2
    return x[0].copy()


def _moment_products(a, b):
    """The nine moment products of every row, shared by ``view_moment_sums_host`` and ``lift_pair_sums_host``: ``a``, ``b`` (R, J, 3)
    float64 -> (R, 9): s_ik = 0.0; s_ik = s_ik + a[j][i] * b[j][k] over ALL J joints ascending, ik = 00, 01, 02, 10, ..., 22."""
    s = np.zeros((a.shape[0], 9), np.float64)
    with np.errstate(all="ignore"):
        for j in range(a.shape[1]):
            for i in range(3):
                for k in range(3):
                    s[:, 3 * i + k] = s[:, 3 * i + k] + a[:, j, i] * b[:, j, k]
    return s


def _calibrate_arrays(poses, kp2d, flags, min_root_joints):
    P, uv, used = _view_arrays(poses, kp2d, flags, False)
    m = check_min_root_joints(min_root_joints)
    if not 1 <= P.shape[1] < 2 ** 31:
        raise ValueError(f"between 1 and 2^31 - 1 rows are taken, got {P.shape[1]}")
    return P.astype(np.float64), uv.astype(np.float64), used, used.sum(axis=2) >= m


def view_moment_sums_host(poses, kp2d, flags=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS):
    """The rotation sums of WHERE THE CAMERAS STAND (include/uu3d.h) in numpy, written to be read: what uu3d_view_moment_sums computes, bit
    for bit.  ``poses`` (V, R, J, 3): every view's lift of every row, root-relative, in that camera's OWN axes (read as float32); ``kp2d``
    (V, R, J, 2) and ``flags`` None or (V, R, J) as ``fuse_views_host`` takes them -> partial (V, C, 10) float64, C = ``calibrate_chunks(R)``.
    View v SEES row r iff at least ``min_root_joints`` of its joints are used there (``fuse_views_host``); row r is a TERM of view v >= 1
    iff view 0 and view v both see it.  A term's values: s_ik = 0.0; s_ik = s_ik + p_v[j][i] * p_0[j][k] over ALL J joints ascending (an
    unobserved joint's lift is still read), ik = 00, 01, 02, 10, ..., 22, and 1.0 as the tenth.  The order of summation is fixed: chunks of
    ``CALIBRATE_CHUNK`` = 4096 rows; in a chunk lane l of ``MATCH_LANES`` = 256 adds the values of the terms among its rows l, l + 256, ...
    ascending to 0.0; then for stride = 128, 64, ..., 1: x[l] = x[l] + x[l + stride] for l < stride.  View 0's partials are zeros."""
    P, _, _, sees = _calibrate_arrays(poses, kp2d, flags, min_root_joints)
    V, R, J = P.shape[:3]
    out = np.zeros((V, calibrate_chunks(R), CALIBRATE_SUMS), np.float64)
    with np.errstate(all="ignore"):
        for v in range(1, V):
            s = np.ones((R, CALIBRATE_SUMS), np.float64)                 # (the tenth value: 1.0)
            s[:, :9] = _moment_products(P[v], P[0])
            out[v] = _chunk_sums(s, sees[0] & sees[v])
    return out


def _normal_sums(uv, used, lift, intrinsics, axes):
    """One view's normal equations of every row: ``uv`` (R, J, 2), ``used`` (R, J), ``lift`` (R, J, 3) float64, ``axes`` nine doubles r1, r2,
    r3 -> (A (6, R), B (3, R)); the statements of ``solve_view_roots_host`` with e = n . P_j and g = m . P_j."""
    fx, fy, cx, cy = intrinsics
    R, J = used.shape
    a00, a01, a02, a11, a12, a22, b0, b1, b2 = (np.zeros(R, np.float64) for _ in range(9))
    for j in range(J):
        a = (uv[:, j, 0] - cx) / fx
        b = (uv[:, j, 1] - cy) / fy
        n0, n1, n2 = axes[0] - a * axes[6], axes[1] - a * axes[7], axes[2] - a * axes[8]
        m0, m1, m2 = axes[3] - b * axes[6], axes[4] - b * axes[7], axes[5] - b * axes[8]
        e = (n0 * lift[:, j, 0] + n1 * lift[:, j, 1]) + n2 * lift[:, j, 2]
        g = (m0 * lift[:, j, 0] + m1 * lift[:, j, 1]) + m2 * lift[:, j, 2]
        u = used[:, j]
        a00 = np.where(u, a00 + (n0 * n0 + m0 * m0), a00)
        a01 = np.where(u, a01 + (n0 * n1 + m0 * m1), a01)
        a02 = np.where(u, a02 + (n0 * n2 + m0 * m2), a02)
        a11 = np.where(u, a11 + (n1 * n1 + m1 * m1), a11)
        a12 = np.where(u, a12 + (n1 * n2 + m1 * m2), a12)
        a22 = np.where(u, a22 + (n2 * n2 + m2 * m2), a22)
        b0 = np.where(u, b0 + (n0 * e + m0 * g), b0)
        b1 = np.where(u, b1 + (n1 * e + m1 * g), b1)
        b2 = np.where(u, b2 + (n2 * e + m2 * g), b2)
    return (a00, a01, a02, a11, a12, a22), (b0, b1, b2)


def _cofactors(a00, a01, a02, a11, a12, a22):
    """The cofactor statements of ``solve_view_roots_host`` -> (c00, c01, c02, c11, c12, c22, det)."""
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    c11 = a00 * a22 - a02 * a02
    c12 = a01 * a02 - a00 * a12
    c22 = a00 * a11 - a01 * a01
    return c00, c01, c02, c11, c12, c22, (a00 * c00 + a01 * c01) + a02 * c02


def _pose_rows(pose, V):
    rows = np.asarray(_host_array(pose), np.float64)
    if rows.shape != (V, CALIBRATE_POSE):
        raise ValueError(f"pose must be ({V}, {CALIBRATE_POSE}), got {rows.shape}")
    return rows


def view_position_sums_host(poses, kp2d, cameras, pose, flags=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS):
    """The position sums of WHERE THE CAMERAS STAND (include/uu3d.h) in numpy, written to be read: what uu3d_view_position_sums computes, bit
    for bit.  ``poses``, ``kp2d``, ``flags`` as ``view_moment_sums_host`` takes them; ``cameras``: V ``Camera`` objects, read for their
    intrinsics (or (V, 4) rows fx, fy, cx, cy); ``pose`` (V, 8) float64: the rows of ``solve_view_pose_host``'s first stage
    -> partial (V, C, 10) float64.
    Per term (a row view 0 and view v both see) and per view u in {0, v}, over u's used joints ascending:
        a = (u - cx) / fx;  b = (v - cy) / fy;  n_i = r1_i - a r3_i;  m_i = r2_i - b r3_i
        e = (n0 P0 + n1 P1) + n2 P2;  g = (m0 P0 + m1 P1) + m2 P2;  A_ik += (n_i n_k + m_i m_k);  B_i += (n_i e + m_i g)
    with, for view 0, r1, r2, r3 = e_1, e_2, e_3 and P the view's own lift, and for view v r_i = ``_rotate_f64(q_v, e_i)`` and
    P = ``_rotate_f64(q_v, lift)``.  The row's root T obeys A0 T = -B0 and Av (T - c) = -Bv, c the camera's position; T is eliminated:
        A = A0 + Av; its cofactors and det by ``solve_view_roots_host``'s statements; det not finite, not > 0 or not above
        ``VIEW_RANK`` ((A00 A11) A22): the row is not a term.  K_ik = c_ik / det
        W_ik = (Av_i0 K_0k + Av_i1 K_1k) + Av_i2 K_2k, all nine
        S_ik = Av_ik - ((W_i0 Av_0k + W_i1 Av_1k) + W_i2 Av_2k) for ik = 00, 01, 02, 11, 12, 22
        h = B0 + Bv;  g_i = Bv_i - ((W_i0 h0 + W_i1 h1) + W_i2 h2)
    The ten values S (6), g (3) and 1.0 go through the order of summation of ``view_moment_sums_host``.  View 0, a view whose state is not
    1 and a view whose (or view 0's) intrinsics are not finite with fx, fy > 0 hold zeros."""
    P, uv, used, sees = _calibrate_arrays(poses, kp2d, flags, min_root_joints)
    V, R, J = P.shape[:3]
    intr = _intrinsic_rows(cameras, V)
    rows = _pose_rows(pose, V)
    out = np.zeros((V, calibrate_chunks(R), CALIBRATE_SUMS), np.float64)
    one, zero = np.float64(1.0), np.float64(0.0)
    fine = np.isfinite(intr).all(axis=1) & (intr[:, 0] > 0) & (intr[:, 1] > 0)
    with np.errstate(all="ignore"):
        A0, B0 = _normal_sums(uv[0], used[0], P[0], intr[0], [one, zero, zero, zero, one, zero, zero, zero, one])
        for v in range(1, V):
            if rows[v, 7] != 1.0 or not fine[0] or not fine[v]:
                continue
            q = [np.float64(a) for a in rows[v, :4]]
            axes = [a for e in ((one, zero, zero), (zero, one, zero), (zero, zero, one)) for a in _rotate_f64(q, *e)]
            turned = np.stack(_rotate_f64(q, P[v, :, :, 0], P[v, :, :, 1], P[v, :, :, 2]), axis=-1)
            Av, Bv = _normal_sums(uv[v], used[v], turned, intr[v], axes)
            a = [x + y for x, y in zip(A0, Av)]
            c00, c01, c02, c11, c12, c22, det = _cofactors(*a)
            term = sees[0] & sees[v] & np.isfinite(det) & (det > 0) & (det > VIEW_RANK * ((a[0] * a[3]) * a[5]))
            k00, k01, k02, k11, k12, k22 = c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det
            v00, v01, v02, v11, v12, v22 = Av
            w00 = (v00 * k00 + v01 * k01) + v02 * k02
            w01 = (v00 * k01 + v01 * k11) + v02 * k12
            w02 = (v00 * k02 + v01 * k12) + v02 * k22
            w10 = (v01 * k00 + v11 * k01) + v12 * k02
            w11 = (v01 * k01 + v11 * k11) + v12 * k12
            w12 = (v01 * k02 + v11 * k12) + v12 * k22
            w20 = (v02 * k00 + v12 * k01) + v22 * k02
            w21 = (v02 * k01 + v12 * k11) + v22 * k12
            w22 = (v02 * k02 + v12 * k12) + v22 * k22
            h0, h1, h2 = B0[0] + Bv[0], B0[1] + Bv[1], B0[2] + Bv[2]
            s = np.stack([v00 - ((w00 * v00 + w01 * v01) + w02 * v02),
                          v01 - ((w00 * v01 + w01 * v11) + w02 * v12),
                          v02 - ((w00 * v02 + w01 * v12) + w02 * v22),
                          v11 - ((w10 * v01 + w11 * v11) + w12 * v12),
                          v12 - ((w10 * v02 + w11 * v12) + w12 * v22),
                          v22 - ((w20 * v02 + w21 * v12) + w22 * v22),
                          Bv[0] - ((w00 * h0 + w01 * h1) + w02 * h2),
                          Bv[1] - ((w10 * h0 + w11 * h1) + w12 * h2),
                          Bv[2] - ((w20 * h0 + w21 * h1) + w22 * h2),
                          np.ones(R, np.float64)], axis=1)
            out[v] = _chunk_sums(s, term)
    return out


_JACOBI_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def horn_matrix(M):
    """Horn's symmetric 4 x 4 matrix of M = sum of p_v (x) p_0, nine doubles M00, M01, ..., M22 -> (4, 4) float64: its largest eigenvector
    is the quaternion (w, x, y, z) that turns the p_v onto the p_0."""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (np.float64(a) for a in M)
    N = np.zeros((4, 4), np.float64)
    with np.errstate(all="ignore"):
        N[0, 0], N[0, 1], N[0, 2], N[0, 3] = (m00 + m11) + m22, m12 - m21, m20 - m02, m01 - m10
        N[1, 1], N[1, 2], N[1, 3] = (m00 - m11) - m22, m01 + m10, m20 + m02
        N[2, 2], N[2, 3] = (m11 - m00) - m22, m12 + m21
        N[3, 3] = (m22 - m00) - m11
    return N + np.triu(N, 1).T


def jacobi_eigen4(N, sweeps=None):
    """Cyclic Jacobi on a symmetric (4, 4) float64 matrix, ``CALIBRATE_SWEEPS`` sweeps (or ``sweeps``) without an early exit, the pairs in
    the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), every operation rounded once -> (eigenvalues (4,), eigenvectors (4, 4), a column each).
    A rotation in the plane (p, q): th = (Nqq - Npp) / (2.0 Npq); tt = (1.0 if th >= 0.0 else -1.0) / (|th| + sqrt(th th + 1.0)); t = 0.0
    if Npq == 0.0 else tt; c = 1.0 / sqrt(t t + 1.0); s = t c; Npp = Npp - t Npq; Nqq = Nqq + t Npq; Npq = 0.0; for the two other indices
    r: (Nrp, Nrq) = (c Nrp - s Nrq, s Nrp + c Nrq); for every row i of E the same."""
    b = np.array(N, np.float64)
    E = np.eye(4, dtype=np.float64)
    two, one = np.float64(2.0), np.float64(1.0)
    with np.errstate(all="ignore"):
        for _ in range(CALIBRATE_SWEEPS if sweeps is None else int(sweeps)):
            for p, q in _JACOBI_PAIRS:
                bpq = b[min(p, q), max(p, q)]
                th = (b[q, q] - b[p, p]) / (two * bpq)
                tt = (one if th >= 0.0 else -one) / (np.abs(th) + np.sqrt(th * th + one))
                t = np.float64(0.0) if bpq == 0.0 else tt
                c = one / np.sqrt(t * t + one)
                s = t * c
                b[p, p] = b[p, p] - t * bpq
                b[q, q] = b[q, q] + t * bpq
                b[p, q] = b[q, p] = 0.0
                for r in range(4):
                    if r in (p, q):
                        continue
                    x, y = b[r, p], b[r, q]
                    b[r, p] = b[p, r] = c * x - s * y
                    b[r, q] = b[q, r] = s * x + c * y
                for i in range(4):
                    x, y = E[i, p], E[i, q]
                    E[i, p] = c * x - s * y
                    E[i, q] = s * x + c * y
    return np.diag(b).copy(), E


def solve_view_pose_host(sums, pose=None, min_terms=VIEW_CALIBRATE_DEFAULTS["min_terms"], sweeps=None):
    """The two solves of WHERE THE CAMERAS STAND (include/uu3d.h) in numpy, written to be read: what uu3d_solve_view_pose computes, bit for
    bit.  ``sums`` (V, C, 10) float64: the partials of ``view_moment_sums_host`` (``pose`` None: the first stage) or of
    ``view_position_sums_host`` (``pose``: the first stage's rows: the second stage) -> (pose (V, 8) float64: the quaternion (w, x, y, z),
    the position, the state as 1.0 / 0.0; terms (V,) int32: the terms of the sums).  A view's chunks are added ascending to 0.0.
    FIRST STAGE.  ``horn_matrix`` of the nine sums, ``jacobi_eigen4``, the column e of the largest eigenvalue (ties: the smaller index),
    len = sqrt(((e0 e0 + e1 e1) + e2 e2) + e3 e3), q = e / len, negated as a whole when q0 < 0.0; X_0 = qrot(q, X_v).  The view is REFUSED
    -- state 0, the identity quaternion -- when its terms are fewer than ``min_terms``, an eigenvalue or q is not finite, or
    top - next > ``CALIBRATE_GAP`` |top| does not hold for the two largest eigenvalues: the lifts then do not fix a rotation.  Row 0 is the
    identity, zeros and state 1; its terms are 0.
    SECOND STAGE.  For a view whose state is 1: S c = g by the cofactors of ``solve_view_roots_host``, c_i = x_i / det; det not finite, not
    > 0, not above ``VIEW_RANK`` ((S00 S11) S22), or c not finite: state 0 and zeros; the quaternion stays either way."""
    S = np.asarray(_host_array(sums), np.float64)
    if S.ndim != 3 or S.shape[2] != CALIBRATE_SUMS or not 1 <= S.shape[0] <= MAX_VIEWS or S.shape[1] < 1:
        raise ValueError(f"sums must be (V, C, {CALIBRATE_SUMS}) with V <= {MAX_VIEWS} and C >= 1, got {S.shape}")
    V = S.shape[0]
    min_terms = _calibrate_parameters(min_terms)
    x = np.zeros((V, CALIBRATE_SUMS), np.float64)
    with np.errstate(all="ignore"):
        for c in range(S.shape[1]):
            x = x + S[:, c]
    terms = x[:, 9].astype(np.int32)
    out = np.zeros((V, CALIBRATE_POSE), np.float64)
    if pose is not None:
        out[:] = _pose_rows(pose, V)
        with np.errstate(all="ignore"):
            for v in range(1, V):
                if out[v, 7] != 1.0:
                    continue
                a = [np.float64(t) for t in x[v, :6]]
                b0, b1, b2 = (np.float64(t) for t in x[v, 6:9])
                c00, c01, c02, c11, c12, c22, det = _cofactors(*a)
                y0 = (c00 * b0 + c01 * b1) + c02 * b2
                y1 = (c01 * b0 + c11 * b1) + c12 * b2
                y2 = (c02 * b0 + c12 * b1) + c22 * b2
                c = np.array([y0 / det, y1 / det, y2 / det], np.float64)
                ok = np.isfinite(det) and det > 0 and det > VIEW_RANK * ((a[0] * a[3]) * a[5]) and np.isfinite(c).all()
                out[v, 4:7] = c if ok else 0.0
                out[v, 7] = 1.0 if ok else 0.0
        return out, terms
    out[:, 0] = 1.0
    out[0, 7] = 1.0
    with np.errstate(all="ignore"):
        for v in range(1, V):
            lam, E = jacobi_eigen4(horn_matrix(x[v, :9]), sweeps)
            k = 0
            for i in range(1, 4):
                if lam[i] > lam[k]:
                    k = i
            nxt = -np.inf
            for i in range(4):
                if i != k and lam[i] > nxt:
                    nxt = lam[i]
            e = E[:, k]
            q = e / np.sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3])
            if q[0] < 0.0:
                q = -q
            ok = int(terms[v]) >= min_terms and np.isfinite(lam).all() and np.isfinite(q).all() and bool(lam[k] - nxt > CALIBRATE_GAP * np.abs(lam[k]))
            if ok:
                out[v, :4], out[v, 7] = q, 1.0
    return out, terms


def calibrate_views_host(poses, kp2d, cameras, flags=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS, min_terms=VIEW_CALIBRATE_DEFAULTS["min_terms"]):
    """``calibrate_views`` built from the mirrors -- ``view_moment_sums_host``, ``solve_view_pose_host``, ``view_position_sums_host``,
    ``solve_view_pose_host`` once more -- on host arrays -> (pose (V, 8) float64, terms (V,) int32: the rows view 0 and the view both see)."""
    first, terms = solve_view_pose_host(view_moment_sums_host(poses, kp2d, flags, min_root_joints), None, min_terms)
    placed, _ = solve_view_pose_host(view_position_sums_host(poses, kp2d, cameras, first, flags, min_root_joints), first, min_terms)
    return placed, terms


def _calibrate_tensors(poses, kp2d, flags, min_root_joints):
    V, R, J, flags = _view_tensors(poses, kp2d, flags, False)
    if not 1 <= R < 2 ** 31:
        raise ValueError(f"between 1 and 2^31 - 1 rows are taken, got {R}")
    return V, R, J, flags, check_min_root_joints(min_root_joints)


def view_moment_sums(poses, kp2d, flags=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS):
    """uu3d_view_moment_sums on the current stream: ``view_moment_sums_host`` on device tensors, one launch, nothing copies to the host or
    waits.  ``poses`` (V, R, J, 3) float32 and ``kp2d`` (V, R, J, 2) float32 on the device, contiguous (only read); ``flags`` (V, R, J)
    uint8 / bool on the device or None -> partial (V, C, 10) float64, a fresh device buffer.  Needs no model."""
    import torch
    lib = _capi.load_library()
    V, R, J, flags, m = _calibrate_tensors(poses, kp2d, flags, min_root_joints)
    partial = torch.empty((V, calibrate_chunks(R), CALIBRATE_SUMS), dtype=torch.float64, device=kp2d.device)
    with torch.cuda.device(kp2d.device):
        stream = torch.cuda.current_stream(kp2d.device).cuda_stream
        _capi.check(lib, lib.uu3d_view_moment_sums(_ptr(poses), _ptr(kp2d), _ptr(flags), V, R, J, m, _ptr(partial), C.c_void_p(stream)), None)
    return partial


def view_position_sums(poses, kp2d, cameras, pose, flags=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS):
    """uu3d_view_position_sums on the current stream: ``view_position_sums_host`` on device tensors, one launch, nothing copies to the host
    or waits (the V intrinsics go up pinned and asynchronously).  ``pose`` (V, 8) float64 on the device: the first stage of
    ``solve_view_pose`` (only read) -> partial (V, C, 10) float64, a fresh device buffer.  Needs no model."""
    import torch
    lib = _capi.load_library()
    V, R, J, flags, m = _calibrate_tensors(poses, kp2d, flags, min_root_joints)
    dev = kp2d.device
    if not _is_device(pose, torch.float64, dev) or tuple(pose.shape) != (V, CALIBRATE_POSE):
        raise ValueError(f"pose must be a contiguous ({V}, {CALIBRATE_POSE}) float64 tensor on kp2d's device")
    intr = _upload(_intrinsic_rows(cameras, V), np.float64, dev)
    partial = torch.empty((V, calibrate_chunks(R), CALIBRATE_SUMS), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_view_position_sums(_ptr(poses), _ptr(kp2d), _ptr(flags), V, R, J, _ptr(intr), m, _ptr(pose), _ptr(partial),
                                                     C.c_void_p(stream)), None)
    return partial


def solve_view_pose(sums, pose=None, min_terms=VIEW_CALIBRATE_DEFAULTS["min_terms"]):
    """uu3d_solve_view_pose on the current stream: ``solve_view_pose_host`` on device tensors, one launch of one wave, nothing copies to
    the host or waits.  ``sums`` (V, C, 10) float64 on the device, contiguous (only read); ``pose`` None (the first stage, on the moment
    sums) or the first stage's (V, 8) float64 rows (the second stage, on the position sums; only read)
    -> (pose (V, 8) float64, terms (V,) int32), fresh device buffers.  Needs no model."""
    import torch
    lib = _capi.load_library()
    if not _is_device(sums, torch.float64) or sums.dim() != 3 or sums.shape[2] != CALIBRATE_SUMS or not 1 <= sums.shape[0] <= MAX_VIEWS or sums.shape[1] < 1:
        raise ValueError(f"sums must be a contiguous (V, C, {CALIBRATE_SUMS}) float64 device tensor with V <= {MAX_VIEWS} and C >= 1, "
                         f"got {tuple(getattr(sums, 'shape', ()))}")
    V, chunks = int(sums.shape[0]), int(sums.shape[1])
    dev = sums.device
    if pose is not None and (not _is_device(pose, torch.float64, dev) or tuple(pose.shape) != (V, CALIBRATE_POSE)):
        raise ValueError(f"pose must be None or a contiguous ({V}, {CALIBRATE_POSE}) float64 tensor on the sums' device")
    min_terms = _calibrate_parameters(min_terms)
    out = torch.empty((V, CALIBRATE_POSE), dtype=torch.float64, device=dev)
    terms = torch.empty((V,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_solve_view_pose(_ptr(sums), V, chunks, 0 if pose is None else 1, min_terms, _ptr(pose), _ptr(out), _ptr(terms),
                                                  C.c_void_p(stream)), None)
    return out, terms


def calibrate_views(poses, kp2d, cameras, flags=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS, min_terms=VIEW_CALIBRATE_DEFAULTS["min_terms"]):
    """Where the cameras stand, on the device: the pose of views 1 .. V - 1 in the space of view 0 from every view's lifts and rays --
    uu3d_view_moment_sums, uu3d_solve_view_pose, uu3d_view_position_sums, uu3d_solve_view_pose once more: four launches, nothing copies to
    the host or waits.  ``poses`` (V, R, J, 3) float32: every view's lift of every row, root-relative, in that camera's OWN axes (the output
    of the model, not taken to world axes); ``kp2d`` (V, R, J, 2) float32: the raw 2D keypoints in the model's layout, undistorted;
    ``flags`` (V, R, J) uint8 / bool or None, all on the device, contiguous (only read); ``cameras``: V ``Camera`` objects, read for their
    intrinsics (or (V, 4) rows).  The same row of every view is the same person at the same instant
    -> (pose (V, 8) float64: per view the quaternion (w, x, y, z) and the position with X_0 = qrot(q, X_v) + c, and the state, 1.0 =
    calibrated; terms (V,) int32: the rows view 0 and the view both see), fresh device buffers; ``calibrated_cameras`` turns the rows,
    once on the host, into ``Camera`` objects.  The rules stand in the three mirrors; ``calibrate_views_host`` is the same call on the host,
    and the two agree bit for bit.  The rig comes out at the model's scale, against view 0 only, every term with unit weight; a person who
    stands still fixes the position poorly: no accuracy is claimed.  Needs no model."""
    first, terms = solve_view_pose(view_moment_sums(poses, kp2d, flags, min_root_joints), None, min_terms)
    placed, _ = solve_view_pose(view_position_sums(poses, kp2d, cameras, first, flags, min_root_joints), first, min_terms)
    return placed, terms


# ---- who is who: which track of one camera is which of another (include/uu3d.h, WHO IS WHO) ---------------------------------------------
class MatchViews(object):
    """The parameters of ``predict_views(match=...)`` / ``match_views``: ``max_dist``, the largest root-mean-square distance between the
    joints' rays, in world units, at which two tracks may be one person (finite, >= 0), and ``min_terms``, the least number of (frame,
    joint) terms such a judgement needs (an int >= 1).  The defaults are conveniences for metres, not tuned values."""

    def __init__(self, max_dist=MATCH_DEFAULTS["max_dist"], min_terms=MATCH_DEFAULTS["min_terms"]):
        self.max_dist, self.min_terms = _match_parameters(max_dist, min_terms)

    def __repr__(self):
        return f"MatchViews(max_dist={self.max_dist!r}, min_terms={self.min_terms!r})"


def _match_parameters(max_dist, min_terms):
    try:
        d = float(max_dist)
    except (TypeError, ValueError):
        raise ValueError(f"max_dist must be a finite number >= 0, got {max_dist!r}") from None
    if isinstance(max_dist, bool) or not np.isfinite(d) or d < 0:
        raise ValueError(f"max_dist must be a finite number >= 0, got {max_dist!r}")
    if isinstance(min_terms, bool) or not isinstance(min_terms, (int, np.integer)) or not 1 <= int(min_terms) < 2 ** 31:
        raise ValueError(f"min_terms must be an int >= 1, got {min_terms!r}")
    return d, int(min_terms)


def check_match(match):
    """``predict_views(match=...)`` -> None (the views are given person by person), a ``MatchViews`` (True is its defaults: the rays are
    matched in the world) or a ``MatchLifts`` (the lifts are matched, which needs no world)."""
    if match is None or match is False:
        return None
    if match is True:
        return MatchViews()
    if not isinstance(match, (MatchViews, MatchLifts)):
        raise ValueError(f"match must be None, True or a MatchViews(max_dist=, min_terms=) -- or a MatchLifts(max_dist=, min_terms=), which "
                         f"needs no world --, got {match!r}")
    return match


def check_view_of(view_of, views=None):
    """``view_of`` (M,): the view of every track, view-major -> (int32 array, V).  1 <= M <= ``MAX_MATCH_TRACKS``, ascending, every entry in
    0 .. V - 1 (``views`` = V; None: the last entry + 1); a view may be empty."""
    v = np.asarray(_host_array(view_of))
    if v.ndim != 1 or not 1 <= v.shape[0] or not np.issubdtype(v.dtype, np.integer):
        raise ValueError(f"view_of must be (M,) integers with M >= 1, got {v.dtype} {v.shape}")
    if v.shape[0] > MAX_MATCH_TRACKS:
        raise ValueError(f"at most {MAX_MATCH_TRACKS} tracks in all views together are matched, got {v.shape[0]}")
    V = int(v[-1]) + 1 if views is None else int(views)
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError(f"between 1 and {MAX_VIEWS} views are taken, got {V}")
    if (np.diff(v) < 0).any() or v[0] < 0 or v[-1] >= V:
        raise ValueError(f"view_of must ascend (the tracks are view-major) within 0 .. {V - 1}, got {v.tolist()}")
    return np.ascontiguousarray(v, np.int32), V


def _pair_shapes(kp_shape, flags_shape, view_of, cams_shape):
    """The shapes of a pair-sums call, checked -> (view_of int32, V, M, T, J)."""
    if len(kp_shape) != 4 or kp_shape[3] != 2 or kp_shape[1] < 1 or not 1 <= kp_shape[2] <= MAX_ROOT_JOINTS:
        raise ValueError(f"kp must be (M, T, J, 2) with T >= 1 and 1 <= J <= {MAX_ROOT_JOINTS}, got {tuple(kp_shape)}")
    M, T, J = (int(n) for n in kp_shape[:3])
    view_of, V = check_view_of(view_of, cams_shape[0])
    if len(view_of) != M:
        raise ValueError(f"view_of must hold one view per track ({M}), got {len(view_of)}")
    if T * J >= 2 ** 31:
        raise ValueError(f"T * J must stay below 2^31 (the int32 terms of a pair), got {T} * {J}")
    if flags_shape is not None and tuple(flags_shape) != (M, T, J):
        raise ValueError(f"flags must be ({M}, {T}, {J}), got {tuple(flags_shape)}")
    return view_of, V, M, T, J


def _camera_rows(cameras):
    """V ``Camera`` objects with extrinsics, or their ``view_rows`` already -> (V, 16) float64."""
    if isinstance(cameras, np.ndarray):
        if cameras.ndim != 2 or cameras.shape[1] != 16 or not 1 <= cameras.shape[0] <= MAX_VIEWS:
            raise ValueError(f"camera rows must be (V, 16) with V <= {MAX_VIEWS}, got {cameras.shape}")
        return np.ascontiguousarray(cameras, np.float64)
    return view_rows(cameras)


def view_pair_sums_host(kp, view_of, cameras, flags=None):
    """The geometry test of WHO IS WHO (include/uu3d.h) in numpy, written to be read: what uu3d_view_pair_sums computes, bit for bit.
    ``kp`` (M, T, J, 2): M tracks of T frames, view-major, in the detector's own joints, undistorted (read as float32); ``view_of`` (M,):
    the view of every track, ascending; ``cameras``: V ``Camera`` objects with extrinsics (or their ``view_rows``); ``flags``: None or
    (M, T, J), non-zero = the joint was observed -> (sums (M, M) float64, terms (M, M) int32), both symmetric.
    Everything in float64, every operation rounded once.  A joint is USED in a track iff its flag is set and both coordinates are finite.
    For tracks p < q of different views v, w, with o = t_w - t_v: oo = (o0 o0 + o1 o1) + o2 o2 not finite or not > 0 -- coincident cameras
    cannot be matched by geometry --: no terms.  Else per frame and per joint used in both tracks, per track
        a = (u - cx) / fx;  b = (v - cy) / fy;  d_i = (r1_i a + r2_i b) + r3_i                  (the pixel's ray in world axes)
    and with dp, dq the two rays
        c = dp x dq;  cc = (c0 c0 + c1 c1) + c2 c2;  pp, qq: the same of dp, dq;  oc = (o0 c0 + o1 c1) + o2 c2;  e = (oc oc) / cc
    -- e is the squared distance between the two LINES in world units; the rays are lines, not half-lines, so an intersection behind a
    camera is not rejected.  The term counts iff cc > ``VIEW_PARALLEL`` (pp qq) and e is finite: 2^-20 is sin^2 of 1e-3 rad, and rays
    closer than that carry no distance information.  The order of summation is fixed: per frame s_f = 0.0; s_f = s_f + e over the counted
    joints ascending, n_f their number; lane l of ``MATCH_LANES`` = 256 sums s_f for f = l, l + 256, ... ascending from 0.0; then for
    stride = 128, 64, ..., 1: x[l] = x[l] + x[l + stride] for l < stride.  sums[p][q] = sums[q][p] = x[0]; terms[p][q] = terms[q][p] = the
    sum of n_f.  Same-view pairs, the diagonal and pairs without terms hold 0.0 and 0."""
    uv = np.asarray(_host_array(kp), np.float32)
    cam = _camera_rows(cameras)
    f = None if flags is None else np.asarray(_host_array(flags)) != 0
    view_of, V, M, T, J = _pair_shapes(uv.shape, None if f is None else f.shape, view_of, cam.shape)
    used = np.isfinite(uv).all(axis=3)
    if f is not None:
        used &= f
    sums, terms = np.zeros((M, M), np.float64), np.zeros((M, M), np.int32)
    uv64 = uv.astype(np.float64)
    with np.errstate(all="ignore"):
        rays = np.empty((M, T, J, 3), np.float64)                        # every track's rays, once
        for m in range(M):
            fx, fy, cx, cy = cam[view_of[m], :4]
            r1, r2, r3 = cam[view_of[m], 4:7], cam[view_of[m], 7:10], cam[view_of[m], 10:13]
            a = (uv64[m, :, :, 0] - cx) / fx
            b = (uv64[m, :, :, 1] - cy) / fy
            for i in range(3):
                rays[m, :, :, i] = (r1[i] * a + r2[i] * b) + r3[i]
        for p in range(M):
            for q in range(p + 1, M):
                v, w = view_of[p], view_of[q]
                if v == w:
                    continue
                o = cam[w, 13:16] - cam[v, 13:16]
                oo = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]
                if not np.isfinite(oo) or not oo > 0:
                    continue
                s, n = np.zeros(T, np.float64), np.zeros(T, np.int64)
                for j in range(J):
                    dp, dq = rays[p, :, j], rays[q, :, j]
                    c0 = dp[:, 1] * dq[:, 2] - dp[:, 2] * dq[:, 1]
                    c1 = dp[:, 2] * dq[:, 0] - dp[:, 0] * dq[:, 2]
                    c2 = dp[:, 0] * dq[:, 1] - dp[:, 1] * dq[:, 0]
                    cc = (c0 * c0 + c1 * c1) + c2 * c2
                    pp = (dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1]) + dp[:, 2] * dp[:, 2]
                    qq = (dq[:, 0] * dq[:, 0] + dq[:, 1] * dq[:, 1]) + dq[:, 2] * dq[:, 2]
                    oc = (o[0] * c0 + o[1] * c1) + o[2] * c2
                    e = (oc * oc) / cc
                    counts = used[p, :, j] & used[q, :, j] & (cc > VIEW_PARALLEL * (pp * qq)) & np.isfinite(e)
                    s = np.where(counts, s + e, s)
                    n += counts
                x = np.zeros(MATCH_LANES, np.float64)                    # lane l: frames l, l + 256, ... in ascending order
                for first in range(0, T, MATCH_LANES):
                    part = s[first:first + MATCH_LANES]
                    x[:len(part)] = x[:len(part)] + part
                stride = MATCH_LANES // 2
                while stride >= 1:                                       # the fixed tree
                    x[:stride] = x[:stride] + x[stride:2 * stride]
                    stride //= 2
                sums[p, q] = sums[q, p] = x[0]
                terms[p, q] = terms[q, p] = int(n.sum())
    return sums, terms


def _group_shapes(sums_shape, terms_shape, view_of, views):
    view_of, V = check_view_of(view_of, views)
    M = len(view_of)
    if tuple(sums_shape) != (M, M) or tuple(terms_shape) != (M, M):
        raise ValueError(f"sums and terms must be ({M}, {M}) beside view_of, got {tuple(sums_shape)} and {tuple(terms_shape)}")
    return view_of, V, M


def group_views_host(sums, terms, view_of, views=None, max_dist=MATCH_DEFAULTS["max_dist"], min_terms=MATCH_DEFAULTS["min_terms"]):
    """The grouping of WHO IS WHO (include/uu3d.h) in plain Python, written to be read: what uu3d_group_views computes.
    ``sums`` (M, M) float64 and ``terms`` (M, M) int32 of ``view_pair_sums_host``; ``view_of`` (M,) ascending; ``views`` = V (None: the
    last entry of ``view_of`` + 1) -> (person (M,) int32, n_persons (1,) int32, table (V, M) int32: the track of person k in view v or -1;
    columns >= n_persons are -1).
    Greedy and view by view, in the spirit of ``associate_host``; the result depends on the order of the views.  Persons start as the
    tracks of the first non-empty view, in track order, ids from 0.  For each later view w, ascending: for person k -- members
    m_1 < m_2 < ..., at most one per view -- and track b of view w: S = 0.0; S = S + sums[m][b] over the members with terms[m][b] > 0 in
    ascending order; n = the sum of those terms.  The pair is ALLOWED iff n >= ``min_terms`` and S / float(n) <= max_dist * max_dist.
    Repeatedly the allowed pair (k, b) of smallest S / n among the persons without a track in view w and the unmatched tracks of view w is
    taken; ties go to the smaller k, then the smaller b.  Persons that existed before the step compete, persons born in it do not.  The
    unmatched tracks of view w then become new persons, in ascending track order."""
    S_, N_ = np.asarray(_host_array(sums), np.float64), np.asarray(_host_array(terms), np.int32)
    view_of, V, M = _group_shapes(S_.shape, N_.shape, view_of, views)
    max_dist, min_terms = _match_parameters(max_dist, min_terms)
    limit = np.float64(max_dist) * np.float64(max_dist)
    person = np.full(M, -1, np.int32)
    table = np.full((V, M), -1, np.int32)
    P = 0
    for w in range(V):
        tracks = [int(b) for b in np.flatnonzero(view_of == w)]
        before = P
        cost = {}
        for k in range(before):
            for b in tracks:
                S, n = np.float64(0.0), 0
                for u in range(w):                                       # the members in ascending order: one per earlier view
                    m = int(table[u, k])
                    if m >= 0 and N_[m, b] > 0:
                        S = S + S_[m, b]
                        n += int(N_[m, b])
                if n >= min_terms and n > 0:
                    mean = S / np.float64(n)
                    if mean <= limit:
                        cost[(k, b)] = mean
        free_k, free_b = set(range(before)), set(tracks)
        while True:
            allowed = [(c, k, b) for (k, b), c in cost.items() if k in free_k and b in free_b]
            if not allowed:
                break
            _, k, b = min(allowed)                                       # smallest cost, then smaller k, then smaller b
            person[b], table[w, k] = k, b
            free_k.discard(k)
            free_b.discard(b)
        for b in tracks:
            if b in free_b:
                person[b], table[w, P] = P, b
                P += 1
    return person, np.array([P], np.int32), table


def _gather_shapes(src_shape, poses_shape, kp_shape, flags_shape, frames):
    if len(src_shape) != 2 or not 1 <= src_shape[0] <= MAX_VIEWS or not 1 <= src_shape[1] <= MAX_MATCH_TRACKS:
        raise ValueError(f"src must be (V, P) with V <= {MAX_VIEWS} and P <= {MAX_MATCH_TRACKS}, got {tuple(src_shape)}")
    T = int(frames)
    if len(kp_shape) != 3 or kp_shape[2] != 2 or not 1 <= kp_shape[1] <= MAX_ROOT_JOINTS or T < 1 or kp_shape[0] < T or kp_shape[0] % T:
        raise ValueError(f"kp2d must be (M * {T}, J, 2) with J <= {MAX_ROOT_JOINTS}, got {tuple(kp_shape)}")
    rows, J = int(kp_shape[0]), int(kp_shape[1])
    if rows // T > MAX_MATCH_TRACKS or T * J >= 2 ** 31:
        raise ValueError(f"at most {MAX_MATCH_TRACKS} tracks with T * J below 2^31 are taken, got {rows // T} tracks of {T} frames")
    if tuple(poses_shape) != (rows, J, 3):
        raise ValueError(f"poses must be ({rows}, {J}, 3) beside kp2d, got {tuple(poses_shape)}")
    if flags_shape is not None and tuple(flags_shape) != (rows, J):
        raise ValueError(f"flags must be ({rows}, {J}), got {tuple(flags_shape)}")
    return int(src_shape[0]), int(src_shape[1]), T, J, rows // T


def gather_view_tracks_host(src, poses, kp2d, flags=None, frames=1):
    """The layout step of WHO IS WHO in numpy: what uu3d_gather_view_tracks writes, bit for bit.  ``src`` (V, P) int: the track of person
    k in view v, or -1 (``table[:, :P]`` of ``group_views_host``); ``poses`` (M * T, J, 3), ``kp2d`` (M * T, J, 2) and ``flags`` None or
    (M * T, J): the M tracks back to back, ``frames`` = T each -> the padded view-major buffers of ``fuse_views_host``: (V, P * T, J, 3)
    float32, (V, P * T, J, 2) float32 and (V, P * T, J) uint8.  An absent (view, person) block -- -1, or anything outside 0 .. M - 1 --
    gets zero poses, NaN keypoints and flags 0: that view then does not SEE the frame.  Without ``flags`` a present block's flags are 1."""
    idx = np.asarray(_host_array(src))
    P_, uv = np.asarray(_host_array(poses), np.float32), np.asarray(_host_array(kp2d), np.float32)
    f = None if flags is None else (np.asarray(_host_array(flags)) != 0).astype(np.uint8)
    V, P, T, J, M = _gather_shapes(idx.shape, P_.shape, uv.shape, None if f is None else f.shape, frames)
    out_p = np.zeros((V, P * T, J, 3), np.float32)
    out_k = np.full((V, P * T, J, 2), np.nan, np.float32)
    out_f = np.zeros((V, P * T, J), np.uint8)
    for v in range(V):
        for k in range(P):
            m = int(idx[v, k])
            if 0 <= m < M:
                out_p[v, k * T:(k + 1) * T] = P_[m * T:(m + 1) * T]
                out_k[v, k * T:(k + 1) * T] = uv[m * T:(m + 1) * T]
                out_f[v, k * T:(k + 1) * T] = 1 if f is None else f[m * T:(m + 1) * T]
    return out_p, out_k, out_f


def _is_device(t, dtype, dev=None):
    import torch
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in (dtype if isinstance(dtype, tuple) else (dtype,)) and t.is_contiguous() \
        and (dev is None or t.device == dev)


def view_pair_sums(kp, view_of, cameras, flags=None):
    """uu3d_view_pair_sums on the current stream: ``view_pair_sums_host`` on device tensors, one launch, nothing copies to the host or
    waits (the camera rows go up pinned and asynchronously; ``view_of`` is a host array).  ``kp`` (M, T, J, 2) float32 on the device,
    contiguous (only read); ``flags`` (M, T, J) uint8 / bool on the device or None -> (sums (M, M) float64, terms (M, M) int32), fresh
    device buffers.  Needs no model."""
    import torch
    lib = _capi.load_library()
    if not _is_device(kp, torch.float32):
        raise ValueError(f"kp must be a contiguous (M, T, J, 2) float32 device tensor, got {tuple(getattr(kp, 'shape', ()))}")
    if flags is not None and not _is_device(flags, (torch.uint8, torch.bool), kp.device):
        raise ValueError("flags must be a contiguous (M, T, J) uint8 or bool tensor on kp's device")
    rows = _camera_rows(cameras)
    view_of, V, M, T, J = _pair_shapes(tuple(kp.shape), None if flags is None else tuple(flags.shape), view_of, rows.shape)
    dev = kp.device
    cams = _upload(rows, np.float64, dev)
    sums = torch.empty((M, M), dtype=torch.float64, device=dev)
    terms = torch.empty((M, M), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_view_pair_sums(_ptr(kp), _ptr(None if flags is None else flags.view(torch.uint8)),
                                                 view_of.ctypes.data_as(C.POINTER(C.c_int32)), M, T, J, V, _ptr(cams), _ptr(sums), _ptr(terms),
                                                 C.c_void_p(stream)), None)
    return sums, terms


def group_views(sums, terms, view_of, views=None, max_dist=MATCH_DEFAULTS["max_dist"], min_terms=MATCH_DEFAULTS["min_terms"]):
    """uu3d_group_views on the current stream: ``group_views_host`` on device tensors, one launch of one wave, nothing copies to the host
    or waits.  ``sums`` (M, M) float64 and ``terms`` (M, M) int32 on the device, contiguous (only read)
    -> (person (M,) int32, n_persons (1,) int32, table (V, M) int32), fresh device buffers.  Needs no model."""
    import torch
    lib = _capi.load_library()
    if not _is_device(sums, torch.float64) or not _is_device(terms, torch.int32, sums.device):
        raise ValueError("sums must be a contiguous (M, M) float64 device tensor and terms an int32 one on its device")
    view_of, V, M = _group_shapes(tuple(sums.shape), tuple(terms.shape), view_of, views)
    max_dist, min_terms = _match_parameters(max_dist, min_terms)
    dev = sums.device
    person = torch.empty((M,), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    table = torch.empty((V, M), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_group_views(_ptr(sums), _ptr(terms), view_of.ctypes.data_as(C.POINTER(C.c_int32)), M, V, max_dist, min_terms,
                                              _ptr(person), _ptr(count), _ptr(table), C.c_void_p(stream)), None)
    return person, count, table


def gather_view_tracks(src, poses, kp2d, flags=None, frames=1):
    """uu3d_gather_view_tracks on the current stream: ``gather_view_tracks_host`` on device tensors, one launch, nothing copies to the
    host or waits.  ``src`` (V, P) int32, ``poses`` (M * T, J, 3) float32, ``kp2d`` (M * T, J, 2) float32 and ``flags`` (M * T, J) uint8 /
    bool or None, on the device, contiguous (only read) -> the three padded view-major buffers, fresh.  Needs no model."""
    import torch
    lib = _capi.load_library()
    if not _is_device(kp2d, torch.float32) or not _is_device(poses, torch.float32, kp2d.device) or not _is_device(src, torch.int32, kp2d.device):
        raise ValueError("src (V, P) int32, poses (M * T, J, 3) float32 and kp2d (M * T, J, 2) float32 must be contiguous tensors on one device")
    if flags is not None and not _is_device(flags, (torch.uint8, torch.bool), kp2d.device):
        raise ValueError("flags must be a contiguous (M * T, J) uint8 or bool tensor on kp2d's device")
    V, P, T, J, M = _gather_shapes(tuple(src.shape), tuple(poses.shape), tuple(kp2d.shape), None if flags is None else tuple(flags.shape), frames)
    dev = kp2d.device
    out_p = torch.empty((V, P * T, J, 3), dtype=torch.float32, device=dev)
    out_k = torch.empty((V, P * T, J, 2), dtype=torch.float32, device=dev)
    out_f = torch.empty((V, P * T, J), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_gather_view_tracks(_ptr(src), _ptr(poses), _ptr(kp2d), _ptr(None if flags is None else flags.view(torch.uint8)),
                                                     V, P, T, J, M, _ptr(out_p), _ptr(out_k), _ptr(out_f), C.c_void_p(stream)), None)
    return out_p, out_k, out_f


def _match_inputs(views, cameras, valid, word="match", one_length=True):
    """The refusals of ``match_views`` (and, with ``word`` = "align" and tracks of any length, of ``align_views``) that need no device
    -> (the cameras, tracks per view, the M tracks view-major, their ``valid`` entries or None / "finite", T -- the list of the tracks'
    lengths without ``one_length``)."""
    if not isinstance(views, (list, tuple)) or not 1 <= len(views) <= MAX_VIEWS or not all(isinstance(v, (list, tuple)) for v in views):
        raise ValueError(f"views must be a list of 1 to {MAX_VIEWS} lists of tracks, one list per camera, got "
                         f"{len(views) if isinstance(views, (list, tuple)) else type(views).__name__}")
    cams = check_view_cameras(cameras, len(views))
    counts = [len(v) for v in views]
    flat = [t for tracks in views for t in tracks]
    if not flat:
        raise ValueError(f"{word}: at least one view must hold a track")
    if len(flat) > MAX_MATCH_TRACKS:
        raise ValueError(f"{word}: at most {MAX_MATCH_TRACKS} tracks in all views together are matched, got {len(flat)}")
    shapes = [_shape(t) for t in flat]
    if any(len(s) != 3 or s[2] != 2 for s in shapes):
        raise ValueError(f"a track must be (T, K, 2), got {[tuple(s) for s in shapes if len(s) != 3 or s[2] != 2][0]}")
    if not one_length:
        if any(int(s[0]) < 1 or int(s[0]) * int(s[1]) >= 2 ** 31 for s in shapes):
            raise ValueError(f"{word}: every track needs at least one frame and T * K below 2^31, got {sorted({int(s[0]) for s in shapes})}")
    elif len({int(s[0]) for s in shapes}) != 1 or int(shapes[0][0]) < 1:
        raise ValueError(f"match: all tracks are on one clock and need one common number of frames T >= 1, got {sorted({int(s[0]) for s in shapes})}")
    if len({int(s[1]) for s in shapes}) != 1 or not 1 <= int(shapes[0][1]) <= MAX_ROOT_JOINTS:
        raise ValueError(f"{word}: all tracks need the same 1 to {MAX_ROOT_JOINTS} joints, got {sorted({int(s[1]) for s in shapes})}")
    flat_valid = valid
    if valid is not None and not isinstance(valid, str):
        if not isinstance(valid, (list, tuple)) or len(valid) != len(views) or \
                not all(isinstance(f, (list, tuple)) and len(f) == n for f, n in zip(valid, counts)):
            raise ValueError(f"valid must be None, \"finite\" or a list of {len(views)} lists, one per view, of {counts} entries")
        flat_valid = [f for per_view in valid for f in per_view]
    elif isinstance(valid, str) and valid != "finite":
        raise ValueError(f"valid must be None, \"finite\" or a list of lists, got {valid!r}")
    return cams, counts, flat, flat_valid, int(shapes[0][0]) if one_length else [int(s[0]) for s in shapes]


def _joint_flags_host(flat_valid, T, K):
    """Per-track ``valid`` entries, (T,) or (T, K) -> (M, T, K) uint8, or None without a list (the finite test alone)."""
    if flat_valid is None or isinstance(flat_valid, str):
        return None
    out = []
    for f in flat_valid:
        a = np.asarray(_host_array(f)) != 0
        if a.shape not in ((T,), (T, K)):
            raise ValueError(f"an entry of valid must be ({T},) or ({T}, {K}), got {a.shape}")
        out.append(np.broadcast_to(a[:, None] if a.ndim == 1 else a, (T, K)))
    return np.ascontiguousarray(np.stack(out), np.uint8)


def match_views_host(views, cameras, valid=None, max_dist=MATCH_DEFAULTS["max_dist"], min_terms=MATCH_DEFAULTS["min_terms"]):
    """``match_views`` built from the mirrors -- ``undistort_points_host``, ``view_pair_sums_host``, ``group_views_host`` -- on host arrays
    -> (person (M,) int32, n_persons (1,) int32, table (V, M) int32, sums (M, M) float64, terms (M, M) int32)."""
    from .camera import undistort_points_host
    cams, counts, flat, flat_valid, T = _match_inputs(views, cameras, valid)
    view_of = np.repeat(np.arange(len(cams), dtype=np.int32), counts)
    flat = [undistort_points_host(np.asarray(_host_array(t), np.float32), cams[v]) if cams[v].has_distortion else np.asarray(_host_array(t), np.float32)
            for t, v in zip(flat, view_of)]
    kp = np.stack(flat)
    sums, terms = view_pair_sums_host(kp, view_of, cams, _joint_flags_host(flat_valid, T, kp.shape[2]))
    return group_views_host(sums, terms, view_of, len(cams), max_dist, min_terms) + (sums, terms)


def _undistorted_tracks(flat, cams, counts, device):
    """The M tracks on the device, those of cameras with distortion undistorted by ONE uu3d_undistort_points -> (list of (T, K, 2) tensors,
    frames per track)."""
    import torch
    tr, _, given = _device_tracks(flat, device)
    view_of = np.repeat(np.arange(len(cams)), counts)
    bent = [m for m in range(len(tr)) if cams[view_of[m]].has_distortion]
    if bent:
        src = torch.cat([tr[m] for m in bent], 0).contiguous() if len(bent) > 1 else tr[bent[0]].contiguous()
        src = undistort_rows(src, np.stack([cams[view_of[m]].row() for m in bent]), given[bent])
        for m, t in zip(bent, torch.split(src, [int(n) for n in given[bent]], 0)):
            tr[m] = t
    return tr, given


def _match_device(tr, cams, counts, flat_valid, params):
    """The two launches of ``match_views`` on undistorted device tracks -> (person, n_persons, table, sums, terms)."""
    import torch
    dev = tr[0].device
    kp = torch.stack(tr).contiguous()
    M, T, K = (int(n) for n in kp.shape[:3])
    flags = None
    if flat_valid is not None and not isinstance(flat_valid, str):
        if all(isinstance(f, torch.Tensor) for f in flat_valid):
            per = []
            for f in flat_valid:
                if tuple(f.shape) not in ((T,), (T, K)):
                    raise ValueError(f"an entry of valid must be ({T},) or ({T}, {K}), got {tuple(f.shape)}")
                f = (f.to(dev) != 0).to(torch.uint8)
                per.append(f[:, None].expand(T, K) if f.dim() == 1 else f)
            flags = torch.stack(per).contiguous()
        else:
            flags = _upload(_joint_flags_host(flat_valid, T, K), np.uint8, dev)
    view_of = np.repeat(np.arange(len(cams), dtype=np.int32), counts)
    sums, terms = view_pair_sums(kp, view_of, cams, flags)
    return group_views(sums, terms, view_of, len(cams), params.max_dist, params.min_terms) + (sums, terms)


def match_views(views, cameras, valid=None, max_dist=MATCH_DEFAULTS["max_dist"], min_terms=MATCH_DEFAULTS["min_terms"], device=None):
    """Who is who across V calibrated cameras, on the device: ``views[v]`` is a list of N_v tracks (T, K, 2) -- any number per view, an
    empty view included, in any order, on the host or the device, all of one length T and one clock --, ``cameras`` V ``Camera`` objects
    with extrinsics, ``valid`` as ``predict_views`` takes it (None, "finite" -- the finite test always holds -- or a list of V lists of
    (T,) or (T, K) flags).  The tracks of cameras with distortion are undistorted (uu3d_undistort_points), then uu3d_view_pair_sums and
    uu3d_group_views run -> (person (M,) int32: the person of every track, view-major, n_persons (1,) int32, table (V, M) int32, sums
    (M, M) float64, terms (M, M) int32) on the device; nothing copies to the host or waits.  The rules stand in ``view_pair_sums_host``
    and ``group_views_host``; ``match_views_host`` is the same call on the host, and the two agree bit for bit.  ``max_dist`` (world
    units) and ``min_terms`` default to ``MATCH_DEFAULTS``: conveniences for metres, not tuned values.  Needs no model."""
    import torch
    params = MatchViews(max_dist, min_terms)
    cams, counts, flat, flat_valid, _ = _match_inputs(views, cameras, valid)
    if device is None:
        on = [t.device for t in flat if isinstance(t, torch.Tensor) and t.is_cuda]
        device = on[0] if on else torch.device("cuda", torch.cuda.current_device())
    tr, _ = _undistorted_tracks(flat, cams, counts, torch.device(device))
    return _match_device(tr, cams, counts, flat_valid, params)


# ---- who is who without a world: tracks matched by their lifts (include/uu3d.h, WHO IS WHO WITHOUT A WORLD) ------------------------------
class MatchLifts(object):
    """The parameters of ``predict_views(match=MatchLifts(...))`` / ``match_lifts``: ``max_dist``, the largest root-mean-square distance
    between the joints of two tracks' lifts after the best common rotation, in the poses' units, at which the two may be one person
    (finite, >= 0), and ``min_terms``, the least number of FRAMES both tracks must see (an int >= 1).  The defaults are conveniences for
    metres and frames, not tuned values."""

    def __init__(self, max_dist=LIFT_MATCH_DEFAULTS["max_dist"], min_terms=LIFT_MATCH_DEFAULTS["min_terms"]):
        self.max_dist, self.min_terms = _match_parameters(max_dist, min_terms)

    def __repr__(self):
        return f"MatchLifts(max_dist={self.max_dist!r}, min_terms={self.min_terms!r})"


def _lift_shapes(poses_shape, kp_shape, flags_shape, view_of, views):
    """The shapes of a lift-pair-sums call, checked -> (view_of int32, V, M, T, J)."""
    view_of, V, M, T, J = _pair_shapes(kp_shape, flags_shape, view_of, (views,))
    if tuple(poses_shape) != (M, T, J, 3):
        raise ValueError(f"poses must be ({M}, {T}, {J}, 3) beside kp2d, got {tuple(poses_shape)}")
    return view_of, V, M, T, J


def lift_pair_sums_host(poses, kp2d, view_of, flags=None, views=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS, totals=False):
    """The lift test of WHO IS WHO WITHOUT A WORLD (include/uu3d.h) in numpy, written to be read: what uu3d_lift_pair_sums computes, bit
    for bit.  ``poses`` (M, T, J, 3): M tracks of T frames, view-major, every track's lifts, root-relative, in its camera's OWN axes
    (read as float32); ``kp2d`` (M, T, J, 2): the 2D keypoints in the model's layout; ``view_of`` (M,): the view of every track, ascending;
    ``flags``: None or (M, T, J), non-zero = the joint was observed; ``views`` = V (None: the last entry of ``view_of`` + 1)
    -> (sums (M, M) float64, terms (M, M) int32), both symmetric; with ``totals`` also the eleven sums of every pair p < q, (M, M, 11).
    Everything in float64, every operation rounded once.  Track p SEES frame f iff at least ``min_root_joints`` of its joints are used
    there (``fuse_views_host``).  For tracks p < q of DIFFERENT views, frame f is a TERM iff both see it; its eleven values, a the lift
    of p and b the lift of q: the nine moment products s_ik = sum over ALL J joints ascending of a[j][i] * b[j][k] (the per-term values
    of ``view_moment_sums_host``, the same function); e = 0.0; e = e + (((a0 a0 + a1 a1) + a2 a2) + ((b0 b0 + b1 b1) + b2 b2)) over the
    joints ascending; and 1.0.  The order of summation is that of ``view_pair_sums_host``: lane l of ``MATCH_LANES`` = 256 adds the
    terms among frames l, l + 256, ... ascending to 0.0, then the fixed tree; there are no chunks.  With M (nine), E and n the sums:
    ``horn_matrix`` of M, ``jacobi_eigen4``, top = the largest eigenvalue (top = lam_0; for i = 1, 2, 3: lam_i > top replaces it);
    S = (E - 2.0 top) / float(J); S < 0.0 becomes 0.0; top or S not finite: S = 0.0 and no terms.  sums[p][q] = sums[q][p] = S,
    terms[p][q] = terms[q][p] = n, the number of term FRAMES.  Same-view pairs and the diagonal hold 0.0 and 0.
    S / n is the mean squared joint distance after the best common rotation: sum |a_j - R b_j|^2 = E - 2 max_R sum a_j . R b_j, and
    Horn's largest eigenvalue is that maximum.  Two persons with one body who move alike cannot be told apart."""
    P = np.asarray(_host_array(poses), np.float32)
    uv = np.asarray(_host_array(kp2d), np.float32)
    f = None if flags is None else np.asarray(_host_array(flags)) != 0
    view_of, V, M, T, J = _lift_shapes(P.shape, uv.shape, None if f is None else f.shape, view_of, views)
    m = check_min_root_joints(min_root_joints)
    used = np.isfinite(uv).all(axis=3)
    if f is not None:
        used &= f
    sees = used.sum(axis=2) >= m                                         # (M, T)
    P64 = P.astype(np.float64)
    sums, terms = np.zeros((M, M), np.float64), np.zeros((M, M), np.int32)
    every = np.zeros((M, M, LIFT_PAIR_SUMS), np.float64)
    two = np.float64(2.0)
    with np.errstate(all="ignore"):
        for p in range(M):
            for q in range(p + 1, M):
                if view_of[p] == view_of[q]:
                    continue
                a, b = P64[p], P64[q]
                s = np.ones((T, LIFT_PAIR_SUMS), np.float64)             # (the eleventh value: 1.0)
                s[:, :9] = _moment_products(a, b)
                e = np.zeros(T, np.float64)
                for j in range(J):
                    e = e + (((a[:, j, 0] * a[:, j, 0] + a[:, j, 1] * a[:, j, 1]) + a[:, j, 2] * a[:, j, 2]) +
                             ((b[:, j, 0] * b[:, j, 0] + b[:, j, 1] * b[:, j, 1]) + b[:, j, 2] * b[:, j, 2]))
                s[:, 9] = e
                x = _lane_sums(s, sees[p] & sees[q])
                every[p, q] = x
                lam, _ = jacobi_eigen4(horn_matrix(x[:9]))
                top = lam[0]
                for i in range(1, 4):
                    if lam[i] > top:
                        top = lam[i]
                S = (x[9] - two * top) / np.float64(J)
                if S < 0.0:
                    S = np.float64(0.0)
                n = int(x[10])
                if not np.isfinite(top) or not np.isfinite(S):
                    S, n = np.float64(0.0), 0
                sums[p, q] = sums[q, p] = S
                terms[p, q] = terms[q, p] = n
    return (sums, terms, every) if totals else (sums, terms)


def lift_pair_sums(poses, kp2d, view_of, flags=None, views=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS):
    """uu3d_lift_pair_sums on the current stream: ``lift_pair_sums_host`` on device tensors, one launch, nothing copies to the host or
    waits (``view_of`` is a host array).  ``poses`` (M, T, J, 3) float32 and ``kp2d`` (M, T, J, 2) float32 on the device, contiguous (only
    read); ``flags`` (M, T, J) uint8 / bool on the device or None -> (sums (M, M) float64, terms (M, M) int32), fresh device buffers.
    Needs no model."""
    import torch
    lib = _capi.load_library()
    if not _is_device(kp2d, torch.float32) or not _is_device(poses, torch.float32, kp2d.device):
        raise ValueError(f"poses (M, T, J, 3) and kp2d (M, T, J, 2) must be contiguous float32 tensors on one device, got "
                         f"{tuple(getattr(poses, 'shape', ()))} and {tuple(getattr(kp2d, 'shape', ()))}")
    if flags is not None and not _is_device(flags, (torch.uint8, torch.bool), kp2d.device):
        raise ValueError("flags must be a contiguous (M, T, J) uint8 or bool tensor on kp2d's device")
    view_of, V, M, T, J = _lift_shapes(tuple(poses.shape), tuple(kp2d.shape), None if flags is None else tuple(flags.shape), view_of, views)
    m = check_min_root_joints(min_root_joints)
    dev = kp2d.device
    sums = torch.empty((M, M), dtype=torch.float64, device=dev)
    terms = torch.empty((M, M), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_lift_pair_sums(_ptr(poses), _ptr(kp2d), _ptr(None if flags is None else flags.view(torch.uint8)),
                                                 view_of.ctypes.data_as(C.POINTER(C.c_int32)), M, T, J, V, m, _ptr(sums), _ptr(terms),
                                                 C.c_void_p(stream)), None)
    return sums, terms


def match_lifts_host(poses, kp2d, view_of, flags=None, views=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS,
                     max_dist=LIFT_MATCH_DEFAULTS["max_dist"], min_terms=LIFT_MATCH_DEFAULTS["min_terms"]):
    """``match_lifts`` built from the mirrors -- ``lift_pair_sums_host``, ``group_views_host`` -- on host arrays
    -> (person (M,) int32, n_persons (1,) int32, table (V, M) int32, sums (M, M) float64, terms (M, M) int32)."""
    params = MatchLifts(max_dist, min_terms)
    sums, terms = lift_pair_sums_host(poses, kp2d, view_of, flags, views, min_root_joints)
    return group_views_host(sums, terms, view_of, views, params.max_dist, params.min_terms) + (sums, terms)


def match_lifts(poses, kp2d, view_of, flags=None, views=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS,
                max_dist=LIFT_MATCH_DEFAULTS["max_dist"], min_terms=LIFT_MATCH_DEFAULTS["min_terms"]):
    """Who is who across V cameras that share no world, on the device: uu3d_lift_pair_sums, then uu3d_group_views -- two launches, nothing
    copies to the host or waits.  ``poses`` (M, T, J, 3) float32: the lifts of M tracks of one length and one clock, view-major, each in
    its camera's OWN axes (the output of the model, not taken to world axes); ``kp2d`` (M, T, J, 2) float32 in the model's layout and
    ``flags`` (M, T, J) uint8 / bool or None, on the device, contiguous (only read); ``view_of`` (M,): the view of every track, ascending,
    on the host -> (person (M,) int32: the person of every track, n_persons (1,) int32, table (V, M) int32, sums (M, M) float64, terms
    (M, M) int32) on the device.  The rules stand in ``lift_pair_sums_host`` and ``group_views_host``; ``match_lifts_host`` is the same
    call on the host, and the two agree bit for bit.  ``max_dist`` (the poses' units) and ``min_terms`` (frames) default to
    ``LIFT_MATCH_DEFAULTS``: conveniences, not tuned values; no matching accuracy is claimed.  Needs no model."""
    params = MatchLifts(max_dist, min_terms)
    sums, terms = lift_pair_sums(poses, kp2d, view_of, flags, views, min_root_joints)
    return group_views(sums, terms, view_of, views, params.max_dist, params.min_terms) + (sums, terms)


# ---- one clock: which frame of one camera is which of another (include/uu3d.h, ONE CLOCK) ----------------------------------------------
class AlignViews(object):
    """The parameters of ``predict_views(align=...)`` / ``align_views``: ``max_lag`` = L, the largest clock offset looked for, in frames
    (an int in 1 .. ``MAX_ALIGN_LAG``), and ``min_terms``, the least number of (frame, joint) terms a pair of tracks needs at a lag to
    speak for it (an int >= 1).  The defaults are conveniences for 50 Hz and metres, not tuned values."""

    def __init__(self, max_lag=ALIGN_DEFAULTS["max_lag"], min_terms=ALIGN_DEFAULTS["min_terms"]):
        self.max_lag, self.min_terms = _align_parameters(max_lag, min_terms)

    def __repr__(self):
        return f"AlignViews(max_lag={self.max_lag!r}, min_terms={self.min_terms!r})"


def _is_int(n):
    return isinstance(n, (int, np.integer)) and not isinstance(n, (bool, np.bool_))


def _align_parameters(max_lag, min_terms):
    if not _is_int(max_lag) or not 1 <= int(max_lag) <= MAX_ALIGN_LAG:
        raise ValueError(f"max_lag must be an int in 1 .. {MAX_ALIGN_LAG}, got {max_lag!r}")
    if not _is_int(min_terms) or not 1 <= int(min_terms) < 2 ** 31:
        raise ValueError(f"min_terms must be an int >= 1, got {min_terms!r}")
    return int(max_lag), int(min_terms)


def check_align(align):
    """``predict_views(align=...)`` -> None (the views are on one clock), an ``AlignViews`` (True is the defaults: the offsets are
    estimated) or a list of ints (the known offsets, one per view)."""
    if align is None or align is False:
        return None
    if align is True:
        return AlignViews()
    if isinstance(align, AlignViews):
        return align
    if isinstance(align, (list, tuple, np.ndarray)) and len(align) >= 1 and all(_is_int(o) for o in align):
        return [int(o) for o in align]
    raise ValueError(f"align must be None, True, an AlignViews(max_lag=, min_terms=) or a list of one int offset per view, got {align!r}")


def _reference_view(view_of, V):
    """-> (the first non-empty view r, its number of tracks N_r, the tracks of every view)."""
    counts = np.bincount(view_of, minlength=V)
    r = int(np.flatnonzero(counts)[0])
    return r, int(counts[r]), counts


def _lag_shapes(kp_shape, flags_shape, view_of, cams_shape, frames, max_lag):
    """The shapes of a lag-sums call, checked -> (view_of int32, V, M, J, first_row (M + 1) int64, L)."""
    if len(kp_shape) != 3 or kp_shape[2] != 2 or not 1 <= kp_shape[1] <= MAX_ROOT_JOINTS:
        raise ValueError(f"kp must be (rows, J, 2) with 1 <= J <= {MAX_ROOT_JOINTS}, got {tuple(kp_shape)}")
    rows, J = int(kp_shape[0]), int(kp_shape[1])
    view_of, V = check_view_of(view_of, cams_shape[0])
    M = len(view_of)
    n = np.asarray(frames)
    if n.shape != (M,) or not np.issubdtype(n.dtype, np.integer) or (n < 1).any() or int(n.sum()) != rows:
        raise ValueError(f"frames must hold one length >= 1 per track ({M}) that add up to kp's {rows} rows, got {n.tolist() if n.ndim == 1 else n.shape}")
    if (n.astype(np.int64) * J >= 2 ** 31).any():
        raise ValueError(f"T * J must stay below 2^31 for every track (the int32 terms of a pair), got {int(n.max())} * {J}")
    L, _ = _align_parameters(max_lag, 1)
    if flags_shape is not None and tuple(flags_shape) != (rows, J):
        raise ValueError(f"flags must be ({rows}, {J}), got {tuple(flags_shape)}")
    return view_of, V, M, J, np.concatenate([[0], np.cumsum(n, dtype=np.int64)]).astype(np.int64), L


def _flat_tracks(kp, frames, flags, cat, length):
    """``kp`` / ``flags`` as a list of M tracks or flat already -> (flat kp, frames, flat flags or None)."""
    if isinstance(kp, (list, tuple)):
        lens = [int(length(t)) for t in kp]
        if frames is not None and [int(n) for n in np.asarray(frames).reshape(-1)] != lens:
            raise ValueError(f"frames must be the lengths of the tracks given, {lens}, got {np.asarray(frames).tolist()}")
        kp, frames = cat(list(kp)), np.asarray(lens, np.int64)
    elif frames is None:
        raise ValueError("frames: a flat (rows, J, 2) kp needs the length of every track")
    if isinstance(flags, (list, tuple)):
        flags = cat(list(flags))
    return kp, np.asarray(frames), flags


def view_lag_sums_host(kp, view_of, cameras, frames=None, max_lag=ALIGN_DEFAULTS["max_lag"], flags=None):
    """The lag sums of ONE CLOCK (include/uu3d.h) in numpy, written to be read: what uu3d_view_lag_sums computes, bit for bit.
    ``kp``: a list of M tracks (T_m, J, 2) or their rows back to back, (rows, J, 2), view-major, in the detector's own joints, undistorted
    (read as float32); ``view_of`` (M,) ascending; ``cameras``: V ``Camera`` objects with extrinsics (or their ``view_rows``); ``frames``
    (M,): every track's length (None with a list); ``max_lag`` = L; ``flags``: None, (rows, J) or a list of (T_m, J), non-zero = observed
    -> (sums (N_r, M, 2 L + 1) float64, terms (N_r, M, 2 L + 1) int32), N_r the tracks of the reference view = the first non-empty view.
    Every track starts at frame 0 of its camera's clock; view v's frame f was taken at common time f + o_v.  For track p of the reference
    view, track q of a later view w and lag l in -L .. L (l stands for o_w - o_r), frame f of p pairs with frame g = f - l of q.  Per
    paired frame and per joint used in both, the term is e of ``view_pair_sums_host``: the rays, c, cc, oc, the ``VIEW_PARALLEL`` test,
    the finite test, no terms for coincident cameras.  The order is that of ``view_pair_sums_host`` over p's frames: s_f over the counted
    joints ascending; a frame without a partner (g < 0 or g >= q's length) has s_f = 0.0 and no terms; lane i of ``MATCH_LANES`` sums s_f
    for f = i, i + 256, ... from 0.0; then the fixed tree.  Lag l is index l + L; the columns q of the reference view hold 0.0 and 0.
    For two tracks of equal length the slice at l = 0 is ``view_pair_sums_host``'s element, bit for bit."""
    kp, frames, flags = _flat_tracks(kp, frames, flags, lambda a: np.concatenate([np.asarray(_host_array(t)) for t in a]), lambda t: _shape(t)[0])
    uv = np.asarray(_host_array(kp), np.float32)
    cam = _camera_rows(cameras)
    f = None if flags is None else np.asarray(_host_array(flags)) != 0
    view_of, V, M, J, first, L = _lag_shapes(uv.shape, None if f is None else f.shape, view_of, cam.shape, frames, max_lag)
    r, n_ref, _ = _reference_view(view_of, V)
    used = np.isfinite(uv).all(axis=2)
    if f is not None:
        used &= f
    sums, terms = np.zeros((n_ref, M, 2 * L + 1), np.float64), np.zeros((n_ref, M, 2 * L + 1), np.int32)
    uv64 = uv.astype(np.float64)
    with np.errstate(all="ignore"):
        rays = np.empty(uv.shape[:2] + (3,), np.float64)                 # every joint's ray, once
        for m in range(M):
            rows = slice(first[m], first[m + 1])
            fx, fy, cx, cy = cam[view_of[m], :4]
            r1, r2, r3 = cam[view_of[m], 4:7], cam[view_of[m], 7:10], cam[view_of[m], 10:13]
            a = (uv64[rows, :, 0] - cx) / fx
            b = (uv64[rows, :, 1] - cy) / fy
            for i in range(3):
                rays[rows, :, i] = (r1[i] * a + r2[i] * b) + r3[i]
        for p in range(n_ref):
            Tp = int(first[p + 1] - first[p])
            for q in range(n_ref, M):
                Tq = int(first[q + 1] - first[q])
                o = cam[view_of[q], 13:16] - cam[r, 13:16]
                oo = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]
                if not np.isfinite(oo) or not oo > 0:
                    continue
                for l in range(-L, L + 1):
                    s, n = np.zeros(Tp, np.float64), 0
                    f0, f1 = max(0, l), min(Tp, Tq + l)                  # the frames f of p with a partner g = f - l in 0 .. Tq - 1
                    if f1 > f0:
                        at_p, at_q = slice(first[p] + f0, first[p] + f1), slice(first[q] + f0 - l, first[q] + f1 - l)
                        dp, dq = rays[at_p], rays[at_q]                  # (frames, J, 3)
                        c0 = dp[..., 1] * dq[..., 2] - dp[..., 2] * dq[..., 1]
                        c1 = dp[..., 2] * dq[..., 0] - dp[..., 0] * dq[..., 2]
                        c2 = dp[..., 0] * dq[..., 1] - dp[..., 1] * dq[..., 0]
                        cc = (c0 * c0 + c1 * c1) + c2 * c2
                        pp = (dp[..., 0] * dp[..., 0] + dp[..., 1] * dp[..., 1]) + dp[..., 2] * dp[..., 2]
                        qq = (dq[..., 0] * dq[..., 0] + dq[..., 1] * dq[..., 1]) + dq[..., 2] * dq[..., 2]
                        oc = (o[0] * c0 + o[1] * c1) + o[2] * c2
                        e = (oc * oc) / cc
                        counts = used[at_p] & used[at_q] & (cc > VIEW_PARALLEL * (pp * qq)) & np.isfinite(e)
                        part = np.zeros(f1 - f0, np.float64)
                        for j in range(J):                               # the counted joints in ascending order
                            part = np.where(counts[:, j], part + e[:, j], part)
                        s[f0:f1] = part
                        n = int(counts.sum())
                    x = np.zeros(MATCH_LANES, np.float64)                # lane i: frames i, i + 256, ... in ascending order
                    for start in range(0, Tp, MATCH_LANES):
                        part = s[start:start + MATCH_LANES]
                        x[:len(part)] = x[:len(part)] + part
                    stride = MATCH_LANES // 2
                    while stride >= 1:                                   # the fixed tree
                        x[:stride] = x[:stride] + x[stride:2 * stride]
                        stride //= 2
                    sums[p, q, l + L] = x[0]
                    terms[p, q, l + L] = n
    return sums, terms


def _offset_shapes(sums_shape, terms_shape, view_of, views, max_lag, min_terms, same_index):
    """The shapes of an offsets call, checked -> (view_of int32, V, M, r, N_r, tracks per view, L, min_terms)."""
    view_of, V = check_view_of(view_of, views)
    M = len(view_of)
    L, min_terms = _align_parameters(max_lag, min_terms)
    r, n_ref, counts = _reference_view(view_of, V)
    want = (n_ref, M, 2 * L + 1)
    if tuple(sums_shape) != want or tuple(terms_shape) != want:
        raise ValueError(f"sums and terms must be {want} beside view_of and max_lag, got {tuple(sums_shape)} and {tuple(terms_shape)}")
    if same_index and any(n not in (0, n_ref) for n in counts):
        raise ValueError(f"same_index needs the same number of tracks in every non-empty view, got {[int(n) for n in counts]}")
    return view_of, V, M, r, n_ref, counts, L, min_terms


def _lag_before(a, la, b, lb):
    """(score a, lag la) before (score b, lag lb): the smaller score, then the smaller |l|, then the smaller l."""
    if a < b:
        return True
    if not a == b:
        return False
    return abs(la) < abs(lb) or (abs(la) == abs(lb) and la < lb)


def view_offsets_host(sums, terms, view_of, views=None, max_lag=ALIGN_DEFAULTS["max_lag"], min_terms=ALIGN_DEFAULTS["min_terms"], same_index=False):
    """The offsets of ONE CLOCK (include/uu3d.h) in plain Python, written to be read: what uu3d_view_offsets computes, bit for bit.
    ``sums`` (N_r, M, 2 L + 1) float64 and ``terms`` int32 of ``view_lag_sums_host``; ``view_of`` (M,) ascending; ``views`` = V (None: the
    last entry of ``view_of`` + 1) -> (offset (V,) int32, state (V,) int32, score (V,) float64).
    For each later non-empty view w and each lag: S = 0.0, n = 0; for each reference track p ascending, the candidates are the tracks q
    of w with terms >= ``min_terms`` -- with ``same_index`` only the track with p's index inside its view (every non-empty view then needs
    N_r tracks) --; the candidate of smallest sums / float(terms) is taken, ties to the smaller q, and S = S + sums, n = n + terms.  The
    lag is ALLOWED iff some p had a candidate; its score is S / float(n).  The view takes the allowed lag of smallest score, ties to the
    smaller |l|, then the smaller l: offset l, state 1 and the score.  A view without an allowed lag: offset 0, state 0, score 0.0; the
    reference view and empty views: offset 0, state 1, score 0.0.  Alignment is against the reference view only; periodic or standing
    motion is ambiguous, and the ties then go to the smallest shift."""
    S_, N_ = np.asarray(_host_array(sums), np.float64), np.asarray(_host_array(terms), np.int32)
    view_of, V, M, r, n_ref, counts, L, min_terms = _offset_shapes(S_.shape, N_.shape, view_of, views, max_lag, min_terms, same_index)
    starts = np.concatenate([[0], np.cumsum(counts)])
    offset, state, score = np.zeros(V, np.int32), np.ones(V, np.int32), np.zeros(V, np.float64)
    with np.errstate(all="ignore"):
        for w in range(V):
            lo, nb = int(starts[w]), int(counts[w])
            if w == r or nb == 0:
                continue
            best = None
            for l in range(-L, L + 1):
                S, n, allowed = np.float64(0.0), 0, False
                for p in range(n_ref):
                    bq, bm = -1, None
                    for q in ([lo + p] if same_index else range(lo, lo + nb)):
                        t = int(N_[p, q, l + L])
                        if t < min_terms:
                            continue
                        mean = S_[p, q, l + L] / np.float64(t)
                        if bq < 0 or mean < bm:                          # strict: ties go to the smaller q
                            bq, bm = q, mean
                    if bq < 0:
                        continue
                    S, n, allowed = S + S_[p, bq, l + L], n + int(N_[p, bq, l + L]), True
                if allowed and (best is None or _lag_before(S / np.float64(n), l, best[0], best[1])):
                    best = (S / np.float64(n), l)
            if best is None:
                state[w] = 0
            else:
                score[w], offset[w] = best
    return offset, state, score


def view_lag_sums(kp, view_of, cameras, frames=None, max_lag=ALIGN_DEFAULTS["max_lag"], flags=None):
    """uu3d_view_lag_sums on the current stream: ``view_lag_sums_host`` on device tensors, two launches (every joint's ray once, then one
    workgroup per (p, q, lag)), nothing copies to the host or waits (the camera rows go up pinned and asynchronously; ``view_of`` and
    ``frames`` are host arrays).  ``kp``: a list of M contiguous (T_m, J, 2) float32 device tensors (joined by one ``torch.cat``) or their
    rows back to back, (rows, J, 2) (only read); ``flags``: None, (rows, J) uint8 / bool on the device or a list of (T_m, J)
    -> (sums (N_r, M, 2 L + 1) float64, terms (N_r, M, 2 L + 1) int32), fresh device buffers.  Needs no model."""
    import torch
    lib = _capi.load_library()
    kp, frames, flags = _flat_tracks(kp, frames, flags, lambda a: torch.cat(a, 0), lambda t: t.shape[0])
    if not _is_device(kp, torch.float32):
        raise ValueError(f"kp must be contiguous float32 device tensors, (rows, J, 2) in all, got {tuple(getattr(kp, 'shape', ()))}")
    if flags is not None and not _is_device(flags, (torch.uint8, torch.bool), kp.device):
        raise ValueError("flags must be a contiguous (rows, J) uint8 or bool tensor on kp's device")
    rows = _camera_rows(cameras)
    view_of, V, M, J, first, L = _lag_shapes(tuple(kp.shape), None if flags is None else tuple(flags.shape), view_of, rows.shape, frames, max_lag)
    _, n_ref, _ = _reference_view(view_of, V)
    dev = kp.device
    cams = _upload(rows, np.float64, dev)
    scratch = torch.empty((int(lib.uu3d_view_lag_scratch_bytes(int(first[-1]), J)),), dtype=torch.uint8, device=dev)
    sums = torch.empty((n_ref, M, 2 * L + 1), dtype=torch.float64, device=dev)
    terms = torch.empty((n_ref, M, 2 * L + 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_view_lag_sums(_ptr(kp), _ptr(None if flags is None else flags.view(torch.uint8)),
                                                view_of.ctypes.data_as(C.POINTER(C.c_int32)), first.ctypes.data_as(C.POINTER(C.c_int64)), M, J, V,
                                                _ptr(cams), L, _ptr(scratch), _ptr(sums), _ptr(terms), C.c_void_p(stream)), None)
    return sums, terms


def view_offsets(sums, terms, view_of, views=None, max_lag=ALIGN_DEFAULTS["max_lag"], min_terms=ALIGN_DEFAULTS["min_terms"], same_index=False):
    """uu3d_view_offsets on the current stream: ``view_offsets_host`` on device tensors, one launch of one wave, nothing copies to the
    host or waits.  ``sums`` (N_r, M, 2 L + 1) float64 and ``terms`` int32 on the device, contiguous (only read)
    -> (offset (V,) int32, state (V,) int32, score (V,) float64), fresh device buffers.  Needs no model."""
    import torch
    lib = _capi.load_library()
    if not _is_device(sums, torch.float64) or not _is_device(terms, torch.int32, sums.device):
        raise ValueError("sums must be a contiguous (N_r, M, 2 L + 1) float64 device tensor and terms an int32 one on its device")
    view_of, V, M, _, _, _, L, min_terms = _offset_shapes(tuple(sums.shape), tuple(terms.shape), view_of, views, max_lag, min_terms, same_index)
    dev = sums.device
    offset = torch.empty((V,), dtype=torch.int32, device=dev)
    state = torch.empty((V,), dtype=torch.int32, device=dev)
    score = torch.empty((V,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_view_offsets(_ptr(sums), _ptr(terms), view_of.ctypes.data_as(C.POINTER(C.c_int32)), M, V, L, min_terms,
                                               1 if same_index else 0, _ptr(offset), _ptr(state), _ptr(score), C.c_void_p(stream)), None)
    return offset, state, score


def _joint_flags_rows(flat_valid, frames, K):
    """Per-track ``valid`` entries, (T_m,) or (T_m, K) -> (rows, K) uint8, or None without a list (the finite test alone)."""
    if flat_valid is None or isinstance(flat_valid, str):
        return None
    return np.concatenate([_joint_flags_host([f], T, K)[0] for f, T in zip(flat_valid, frames)])


def align_views_host(views, cameras, valid=None, max_lag=ALIGN_DEFAULTS["max_lag"], min_terms=ALIGN_DEFAULTS["min_terms"], same_index=False):
    """``align_views`` built from the mirrors -- ``undistort_points_host``, ``view_lag_sums_host``, ``view_offsets_host`` -- on host arrays
    -> (offset (V,) int32, state (V,) int32, score (V,) float64, sums (N_r, M, 2 L + 1) float64, terms int32)."""
    from .camera import undistort_points_host
    params = AlignViews(max_lag, min_terms)
    cams, counts, flat, flat_valid, frames = _match_inputs(views, cameras, valid, "align", False)
    view_of = np.repeat(np.arange(len(cams), dtype=np.int32), counts)
    _same_index_counts(counts, same_index)
    flat = [undistort_points_host(np.asarray(_host_array(t), np.float32), cams[v]) if cams[v].has_distortion else np.asarray(_host_array(t), np.float32)
            for t, v in zip(flat, view_of)]
    sums, terms = view_lag_sums_host(flat, view_of, cams, frames, params.max_lag, _joint_flags_rows(flat_valid, frames, flat[0].shape[1]))
    return view_offsets_host(sums, terms, view_of, len(cams), params.max_lag, params.min_terms, same_index) + (sums, terms)


def _align_device(tr, cams, counts, flat_valid, params, same_index):
    """The launches of ``align_views`` on undistorted device tracks -> (offset, state, score, sums, terms)."""
    import torch
    dev = tr[0].device
    frames = [int(t.shape[0]) for t in tr]
    K = int(tr[0].shape[1])
    kp = torch.cat(tr, 0).contiguous() if len(tr) > 1 else tr[0].contiguous()
    flags = None
    if flat_valid is not None and not isinstance(flat_valid, str):
        if all(isinstance(f, torch.Tensor) for f in flat_valid):
            per = []
            for f, T in zip(flat_valid, frames):
                if tuple(f.shape) not in ((T,), (T, K)):
                    raise ValueError(f"an entry of valid must be ({T},) or ({T}, {K}), got {tuple(f.shape)}")
                f = (f.to(dev) != 0).to(torch.uint8)
                per.append(f[:, None].expand(T, K) if f.dim() == 1 else f)
            flags = torch.cat(per, 0).contiguous()
        else:
            flags = _upload(_joint_flags_rows(flat_valid, frames, K), np.uint8, dev)
    view_of = np.repeat(np.arange(len(cams), dtype=np.int32), counts)
    sums, terms = view_lag_sums(kp, view_of, cams, frames, params.max_lag, flags)
    return view_offsets(sums, terms, view_of, len(cams), params.max_lag, params.min_terms, same_index) + (sums, terms)


def _same_index_counts(counts, same_index):
    if same_index and len({n for n in counts if n > 0}) > 1:
        raise ValueError(f"same_index needs the same number of tracks in every non-empty view, got {[int(n) for n in counts]}")


def align_views(views, cameras, valid=None, max_lag=ALIGN_DEFAULTS["max_lag"], min_terms=ALIGN_DEFAULTS["min_terms"], same_index=False, device=None):
    """Every camera's clock offset against the first non-empty view, on the device: ``views[v]`` is a list of N_v tracks (T, K, 2), each
    with its own length and starting at frame 0 of its camera's clock -- any number per view, an empty view included, on the host or the
    device --, ``cameras`` V ``Camera`` objects with extrinsics, ``valid`` as ``match_views`` takes it.  The tracks of cameras with
    distortion are undistorted (uu3d_undistort_points), then uu3d_view_lag_sums and uu3d_view_offsets run
    -> (offset (V,) int32: view v's frame f was taken at common time f + offset[v], state (V,) int32: 0 = no lag of this view had
    ``min_terms`` terms with the reference view, score (V,) float64: the mean squared distance between the lines at the lag taken, sums
    (N_r, M, 2 max_lag + 1) float64, terms int32) on the device; nothing copies to the host or waits.  ``same_index=True``: track i of a
    view is person i of every view (the views then hold the same number of tracks); False: every reference track takes, per lag, its
    best partner in the view (a reference track whose person the view does not hold takes a stranger, which can spoil that view's score).
    The rules stand in ``view_lag_sums_host`` and ``view_offsets_host``; ``align_views_host`` is the same call
    on the host, and the two agree bit for bit.  ``max_lag`` and ``min_terms`` default to ``ALIGN_DEFAULTS``: conveniences for 50 Hz
    and metres, not tuned values.  Whole frames against the reference view only; no accuracy is claimed.  Needs no model."""
    import torch
    params = AlignViews(max_lag, min_terms)
    cams, counts, flat, flat_valid, _ = _match_inputs(views, cameras, valid, "align", False)
    _same_index_counts(counts, same_index)
    if device is None:
        on = [t.device for t in flat if isinstance(t, torch.Tensor) and t.is_cuda]
        device = on[0] if on else torch.device("cuda", torch.cuda.current_device())
    tr, _ = _undistorted_tracks(flat, cams, counts, torch.device(device))
    return _align_device(tr, cams, counts, flat_valid, params, same_index)


def _view_lengths(views):
    """The one length T_v of every view's tracks, None for an empty view; a view whose tracks differ in length is a ValueError."""
    if not isinstance(views, (list, tuple)) or not 1 <= len(views) <= MAX_VIEWS or not all(isinstance(v, (list, tuple)) for v in views):
        raise ValueError(f"views must be a list of 1 to {MAX_VIEWS} lists of tracks, one list per camera, got "
                         f"{len(views) if isinstance(views, (list, tuple)) else type(views).__name__}")
    lengths = []
    for v, tracks in enumerate(views):
        here = [int(_shape(t)[0]) if len(_shape(t)) else -1 for t in tracks]
        if len(set(here)) > 1 or (here and here[0] < 1):
            raise ValueError(f"align: every track of a view needs the same number of frames T_v >= 1 (they share the camera's clock): view {v} has {here}")
        lengths.append(here[0] if here else None)
    return lengths


def crop_views(views, offsets, valid=None):
    """The common time window of V views with known clock offsets, on the host and without a copy (slices): ``views[v]``: a list of
    tracks (T_v, K, 2), all of view v's of one length, on the host or the device; ``offsets``: V ints, view v's frame f was taken at
    common time f + offsets[v]; ``valid``: None, "finite" or a list of V lists of per-track entries, arrays of T_v rows (anything else in
    an entry passes through) -> (the cropped views, the cropped ``valid``, first: V ints).  Over the non-empty views lo = max o_v and
    hi = min (T_v + o_v); view v keeps its frames lo - o_v .. hi - o_v - 1, and first[v] = lo - o_v (0 for an empty view).  A window of
    less than one frame (hi - lo < 1) is a ValueError."""
    lengths = _view_lengths(views)
    V = len(views)
    if not isinstance(offsets, (list, tuple, np.ndarray)) or len(offsets) != V or not all(_is_int(o) for o in offsets):
        raise ValueError(f"offsets must hold one int per view ({V}), got {offsets!r}")
    live = [v for v in range(V) if lengths[v] is not None]
    if not live:
        raise ValueError("align: at least one view must hold a track")
    lo, hi = max(int(offsets[v]) for v in live), min(lengths[v] + int(offsets[v]) for v in live)
    if hi - lo < 1:
        raise ValueError(f"align: the views share no frame: offsets {[int(o) for o in offsets]} and lengths {lengths} leave a window of {hi - lo} frames")
    first = [lo - int(offsets[v]) if lengths[v] is not None else 0 for v in range(V)]
    cropped = [[t[first[v]:first[v] + hi - lo] for t in views[v]] for v in range(V)]
    if valid is None or isinstance(valid, str):
        return cropped, valid, first
    if not isinstance(valid, (list, tuple)) or len(valid) != V or not all(isinstance(f, (list, tuple)) and len(f) == len(t) for f, t in zip(valid, views)):
        raise ValueError(f"valid must be None, \"finite\" or a list of {V} lists, one per view, of {[len(t) for t in views]} entries")
    kept = []
    for v in range(V):
        row = []
        for f in valid[v]:
            if f is None or isinstance(f, str):
                row.append(f)
                continue
            if not len(_shape(f)) or int(_shape(f)[0]) != lengths[v]:
                raise ValueError(f"an entry of valid must have one row per frame of its track ({lengths[v]}), got {tuple(_shape(f))}")
            row.append(f[first[v]:first[v] + hi - lo])
        kept.append(row)
    return cropped, kept, first


def _predict_aligned_views(align, match, model, views, cameras, valid, fps, keyframes_only, out_fps, call):
    """``predict_views(align=...)``: the steps of its docstring, "One clock"; ``call(views, valid)`` is the call without ``align``."""
    import torch
    if keyframes_only:
        raise ValueError("predict_views does not take keyframes_only: the fusion needs one returned frame per given frame of every view")
    if out_fps is not None:
        raise ValueError("predict_views does not take out_fps: the fusion needs one returned frame per given frame of every view")
    lengths = _view_lengths(views)
    V = len(views)
    check_view_cameras(cameras, V)
    if isinstance(fps, (list, tuple, np.ndarray)):
        raise ValueError("predict_views(align=...) takes one fps for all tracks, not a list: the offsets are frames of one common rate")
    counts = [len(v) for v in views]
    if match is None and (counts[0] < 1 or any(n != counts[0] for n in counts)):
        raise ValueError(f"every view must hold the same persons, at least one: got {counts} tracks per view")
    if isinstance(align, AlignViews):
        cams, counts, flat, flat_valid, _ = _match_inputs(views, cameras, valid, "align", False)
        shortest = min(n for n in lengths if n is not None)
        if align.max_lag >= 2 * shortest:
            raise ValueError(f"align: max_lag must stay below twice the shortest view's frames ({shortest}), got {align.max_lag}")
        tr, _ = _undistorted_tracks(flat, cams, counts, torch.device(model.device))
        offset, state, _, _, _ = _align_device(tr, cams, counts, flat_valid, align, match is None)
        back = torch.stack([offset, state]).cpu().numpy()                # the ONE copy: the window's length shapes every buffer behind it
        lost = [v for v in range(V) if back[1, v] == 0]
        if lost:
            raise ValueError(f"align: view {lost[0]} shares no lag of at least {align.min_terms} terms with the reference view and cannot be "
                             f"aligned (views without an offset: {lost})")
        offsets = [int(o) for o in back[0]]
    else:
        if len(align) != V:
            raise ValueError(f"align: one offset per view ({V}) is needed, got {len(align)}")
        offsets = list(align)
    cropped, kept, first = crop_views(views, offsets, valid)
    return tuple(call(cropped, kept)) + (offsets, first)


def _check_views(views, cameras, valid, keyframes_only, out_fps):
    """The refusals of ``predict_views`` that need no device -> (the cameras, V, N, frames per person)."""
    if keyframes_only:
        raise ValueError("predict_views does not take keyframes_only: the fusion needs one returned frame per given frame of every view")
    if out_fps is not None:
        raise ValueError("predict_views does not take out_fps: the fusion needs one returned frame per given frame of every view")
    if not isinstance(views, (list, tuple)) or not 1 <= len(views) <= MAX_VIEWS or not all(isinstance(v, (list, tuple)) for v in views):
        raise ValueError(f"views must be a list of 1 to {MAX_VIEWS} lists of tracks, one list per camera, got "
                         f"{len(views) if isinstance(views, (list, tuple)) else type(views).__name__}")
    V, N = len(views), len(views[0])
    cams = check_view_cameras(cameras, V)
    if N < 1 or any(len(v) != N for v in views):
        raise ValueError(f"every view must hold the same persons, at least one: got {[len(v) for v in views]} tracks per view")
    frames = [int(_shape(t)[0]) if len(_shape(t)) else -1 for t in views[0]]
    for v, tracks in enumerate(views):
        here = [int(_shape(t)[0]) if len(_shape(t)) else -1 for t in tracks]
        if here != frames:
            raise ValueError(f"person i must have the same number of frames T_i in every view (the views are time-synchronised): view 0 has "
                             f"{frames}, view {v} has {here}")
    if valid is not None and not isinstance(valid, str):
        if not isinstance(valid, (list, tuple)) or len(valid) != V or not all(isinstance(f, (list, tuple)) and len(f) == N for f in valid):
            raise ValueError(f"valid must be None, \"finite\" or a list of {V} lists, one per view, of {N} entries each")
    return cams, V, N, frames


def _fused_scene(pt, person, world, kp2d, flags, cams, lens, rates, model_fps, return_views, triangulate=None, root=0):
    """Stages 3 to 6 of the module's docstring, behind uu3d_camera_to_world: ``world`` (V, R, J, 3), ``kp2d`` (V, R, J, 2) and ``flags`` None
    or (V, R, J), view-major, the same person at the same rows of every view; ``person``: the ``StageOptions`` of the persons; ``lens``:
    frames per person; ``triangulate``: None or a ``Triangulate``, ``root`` the root joint -> what ``predict_views`` returns."""
    import torch
    # 4. the fusion
    fused, view_count, sees = fuse_views(world, kp2d, flags, person.min_root_joints)
    # 4a. + 4b. where rays meet: the joints two or more seeing cameras agree on, placed by geometry
    joint_views = None
    if triangulate is not None:
        points, agreed = triangulate_joints(kp2d, cams, sees, flags, triangulate.max_residual, triangulate.min_views)
        fused, joint_views = place_joints(fused, points, agreed, root)
    # 5. bones on the fused poses of the N persons
    if person.rigid is not None:
        skeleton, known = person.rigid
        bone_table = pt.bone_lengths(fused, lens, skeleton) if known is None else _upload(known, np.float64, fused.device)
        fused = pt.fix_bones(fused, lens, bone_table, skeleton)
    # 6. + 7. one world root per frame from all views, joined to each person's trajectory
    solved_roots, solved = solve_view_roots(fused, kp2d, cams, flags, person.min_root_joints)
    roots, root_state = pt.root_trajectory(solved_roots, solved, lens, None)
    # 8. filters and rotations on the fused world scene, in the order of predict_tracks
    shown = fused
    if person.pose_filter is not None or person.root_filter is not None:
        out_rate = model_fps if rates is None else rates
    if person.pose_filter is not None:
        shown = pt.one_euro(shown, lens, out_rate, person.pose_filter)
    if person.root_filter is not None:
        roots = pt.one_euro(roots, lens, out_rate, person.root_filter, state=root_state)
    sizes = [int(n) for n in lens]
    result = tuple(list(torch.split(a, sizes, 0)) for a in (shown, roots, root_state, view_count) + (() if joint_views is None else (joint_views,)))
    if person.rotations is not None:
        turned = pt.joint_rotations(shown, person.rotations)
        result += (list(torch.split(turned[0], sizes, 0)),) + ((list(torch.split(turned[2], sizes, 0)),) if person.rotations.return_global else ())
    if return_views:
        result += ([list(torch.split(block, sizes, 0)) for block in world],)
    return result


def predict_views(model, config, views, cameras, resolutions=None, mask_stride=None, flip=None, reuse_frames=True, batch_size=None, depth=None,
                  graph=True, valid=None, fps=None, model_fps=50, repair_joints=None, keypoints=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS,
                  smooth=None, bones=None, rotations=None, interpolation="linear", return_views=False, keyframes_only=False, out_fps=None, match=None,
                  align=None, triangulate=None, calibrate=None):
    """One world scene from V calibrated views of the same N persons -> (poses, roots, root_state, view_count): per person ``poses``
    (T_i, J, 3) float32 in world axes and root-relative, ``roots`` (T_i, 3) float32 in world coordinates, ``root_state`` (T_i,) uint8 (1
    solved here, 2 interpolated or held, 0 no solved frame) and ``view_count`` (T_i,) uint8, the views that saw the frame; on the model's
    device, views of one buffer each.  ``rotations`` appends the quaternion lists as ``predict_tracks`` does; ``return_views=True`` then
    appends the per-view world poses the fusion read, a list of V lists.

    ``views``: a list of V lists, 1 <= V <= 8; ``views[v][i]`` is person i's 2D track in camera v, (T_i, J, 2), or (T_i, K_in, 2) with
    ``keypoints``.  The same index is the same person, frames are time-synchronised and person i has the same T_i in every view (anything
    else: ValueError, unless ``match`` finds who is who across cameras and ``align`` the cameras' clock offsets, below).  A view that does not see the person at a
    frame passes NaN coordinates there (with ``valid="finite"``) or cleared flags.  ``cameras``: V ``Camera`` objects, all with
    extrinsics, each with or without distortion, one per view and shared by its persons.  ``resolutions``: None, one (w, h) or one per
    view.  ``valid``: as in ``predict_tracks``, per view -- None, "finite" or a list of V lists.  ``fps``: one rate, or one per person.
    ``bones``: "track", one (J,) array, a ``Bones`` or a list with one entry per PERSON.  ``mask_stride``, ``flip``, ``repair_joints``,
    ``keypoints``, ``smooth``, ``rotations``, ``interpolation``, ``min_root_joints``, ``batch_size``, ``depth``, ``graph`` and
    ``reuse_frames`` mean what they mean in ``predict_tracks``.  ``keyframes_only`` and ``out_fps`` are refused: the fusion needs one
    returned frame per given frame.

    The stages and the two rules stand in the module's docstring.  The views with distortion are undistorted by one
    uu3d_undistort_points over their tracks in front of everything else (a list that mixes cameras with and without distortion is taken
    here, which the front of ``predict_tracks`` refuses).  The result equals, bit for bit, the host composition on
    ``predict_tracks(flattened tracks, camera=the cameras minus extrinsics, one per track)``: ``camera_to_world_host``,
    ``fuse_views_host``, ``fix_bones_host``, ``solve_view_roots_host``, ``root_trajectory_host``, ``one_euro_host``,
    ``joint_rotations_host``.  No accuracy is claimed.

    Who is who -- ``match``: None = the call above, the same launches, buffers, refusals and bits.  True (``MATCH_DEFAULTS``) or a
    ``MatchViews(max_dist=, min_terms=)``: ``views[v]`` is the list of camera v's N_v tracks in ANY order -- other counts per view, an
    empty view as long as one is not --, M = sum N_v <= 64 tracks, all with the same T (anything else: ValueError) and one ``fps``.
    ``bones`` as a per-person list is refused (the persons are not known beforehand); "track", one array and a ``Bones`` stay.  The
    tracks are undistorted and matched on the detector's joints, in front of any ``keypoints`` map (``match_views``); then ``person``,
    ``n_persons`` and ``table`` are copied to the host -- the ONE copy of the call, M + 1 + V M int32, which waits for the two launches:
    the number of persons P shapes every buffer behind it.  All M tracks run through the front as given, go to world axes (block sizes
    N_v T), uu3d_gather_view_tracks lays them out per person, and the fusion, ``bones``, the root solve, the trajectory, ``smooth`` and
    ``rotations`` run unchanged on P persons.  -> today's tuple with P persons, followed by ``person``: per view a list of N_v ints, the
    person of each given track.  A person seen by one camera comes out with ``view_count`` <= 1 and the monocular root.  The result
    equals, bit for bit, the host composition with ``match_views_host`` and ``gather_view_tracks_host`` in front of the fusion.

    One clock -- ``align``: None = the call above, the same launches, buffers, refusals and bits.  With ``align`` every track of view v
    has one length T_v and starts at frame 0 of camera v's clock; the views may differ in length (this replaces "the same T in every
    view" for this call only), and view v's frame f was taken at common time f + o_v.  A list of V ints gives the offsets o_v as known:
    no device work and no copy, only the crop.  True (``ALIGN_DEFAULTS``) or an ``AlignViews(max_lag=, min_terms=)`` estimates them: the
    tracks are undistorted, uu3d_view_lag_sums and uu3d_view_offsets run on the detector's joints (``align_views``; with ``match`` None
    the same index is the same person, ``same_index=True``; with ``match`` every reference track takes its best partner per lag), and
    ``offset`` and ``state``, 2 V int32, are copied to the host -- ONE small copy, which waits for the launches: the window's length
    shapes every buffer behind it.  A view that cannot be aligned (state 0) is a ValueError that names it.  ``crop_views`` then cuts the
    views, and the entries of ``valid`` given as arrays, to the common window by slicing, and the call proceeds as above on the cropped
    tracks, through the ``match`` path or the plain one (the cropped tracks of a camera with distortion are undistorted there once more:
    per point, the same bits) -> that call's tuple followed by ``offsets`` and ``first``, two lists of V ints: the clock offsets, and
    the given frame of every view that became frame 0.  Refused with ``align``: ``fps`` as a per-person list, a view whose tracks differ
    in length, ``max_lag`` of twice the shortest view's frames or more; ``keyframes_only`` and ``out_fps`` stay refused in their words.
    The result minus its last two items equals, bit for bit, ``predict_views(*crop_views(views, offsets, valid)[:2], align=None)``.
    Whole frames against the first non-empty view only: no sub-frame refinement, no per-camera frame rates, no chaining through a third
    camera; periodic or standing motion is ambiguous.  No alignment accuracy is claimed.

    Where rays meet -- ``triangulate``: None = the call above, the same launches, buffers, refusals and bits.  True
    (``TRIANGULATE_DEFAULTS``) or a ``Triangulate(max_residual=, min_views=)``; anything else is a ValueError.  Directly behind the fusion
    and in front of ``bones`` -- on the plain, the ``match`` and the ``align`` route alike -- uu3d_triangulate_joints solves every joint
    that at least ``min_views`` seeing cameras observed from their rays alone, and uu3d_place_joints writes the hybrid pose: a joint the
    cameras agree on within ``max_residual`` pixels (of the tracks as given, undistorted) is X_j - X_root, with ``config.ROOT_KEYTPOINT``
    the root; every other joint, and every joint of a frame whose root joint is not triangulated, keeps the fused lift.  Two launches,
    nothing copies to the host or waits; everything behind runs unchanged on that pose.  -> ``joint_views`` directly behind
    ``view_count``: per person (T_i, J) uint8, the cameras that placed the joint, 0 where it is the lift; ``rotations``, ``return_views``
    (still the per-view lifts), ``person``, ``offsets`` and ``first`` follow as before.  One view is taken, and nothing is triangulated.
    The result equals, bit for bit, the host composition with ``triangulate_joints_host`` and ``place_joints_host`` behind
    ``fuse_views_host``.  The limits stand in the module's docstring; the defaults are not tuned, and no accuracy is claimed.

    Where the cameras stand -- ``calibrate``: None = the call above, the same launches, buffers, refusals and bits.  True
    (``VIEW_CALIBRATE_DEFAULTS``) or a ``CalibrateViews(min_terms=)``; anything else is a ValueError.  ``cameras`` are V ``Camera`` objects
    with intrinsics, each with or without distortion; cameras 1 .. V - 1 come WITHOUT extrinsics (one that has them is a ValueError that
    names it), camera 0 may keep its own, which then define the world -- without, the world is camera 0's own space.  The same index is
    the same person on one clock: ``match=True``, a ``MatchViews`` and an ``align`` that estimates (True, an ``AlignViews``) are refused,
    since they need the rays in one world (a ``MatchLifts`` does not, see below); ``align=[o_0, ...]`` with known offsets is taken, it only crops.  Behind the assembly, which runs on pinhole cameras
    anyway, and in front of uu3d_camera_to_world the four launches of ``calibrate_views`` run on the lifts in camera axes and the
    keypoints in the model's layout; then the poses are copied to the host -- the ONE copy of the stage, V x 9 float64 (quaternion,
    position, state, terms), which waits for the launches -- and ``calibrated_cameras`` builds every view's ``Camera``.  A view that
    cannot be calibrated (state 0: fewer than ``min_terms`` rows shared with view 0, lifts that fix no rotation, a position the rows do
    not fix) is a ValueError that names it.  The call proceeds unchanged -> its tuple followed by ``cameras``, the V ``Camera`` objects
    with extrinsics, ready for a later call without ``calibrate``, and ``calibration``, per view (state, terms); with ``align=[...]``
    the two stand behind ``offsets`` and ``first``.  One view calibrates nothing and returns camera 0 as the world.  The result minus
    its last two items equals, bit for bit, ``predict_views(views, the returned cameras, ...)``.  The rig's scale is the model's; the
    limits stand in the module's docstring, and no accuracy is claimed.

    Who is who without a world -- ``match=MatchLifts(max_dist=, min_terms=)`` (``LIFT_MATCH_DEFAULTS``: 0.1 m, 50 frames), with or without
    ``calibrate``: the tracks are matched by their LIFTS, which needs no extrinsics -- two tracks of different views are one person iff
    their lifts agree up to one rotation over the whole track (``match_lifts``; ``max_dist`` is the root-mean-square joint distance after
    that rotation, ``min_terms`` the frames both tracks must see).  ``views``, ``fps`` and ``bones`` are taken and refused as ``match=True``
    takes and refuses them; with ``calibrate`` view 0 must hold a track, since it defines the world.  The M tracks are undistorted and run
    through the front as given; uu3d_lift_pair_sums and uu3d_group_views run on the lifts in camera axes and the keypoints in the model's
    layout; ``person``, ``n_persons`` and ``table`` are copied to the host, the ONE copy of the matched route; uu3d_gather_view_tracks lays
    the lifts out per person BEFORE they go to world axes; with ``calibrate`` the four launches of ``calibrate_views`` run on the gathered
    (V, P T, ...) buffers, followed by its V x 9 copy and its ValueError that names a view without a pose; uu3d_camera_to_world takes one
    row per view block, and everything behind runs unchanged on P persons.  -> today's tuple, then ``person``, then, with ``calibrate``,
    ``cameras`` and ``calibration``, which stay last (``align=[o_0, ...]`` puts ``offsets`` and ``first`` in front of them).  ``align=True``
    or an ``AlignViews`` is refused with a ``MatchLifts``.  The result equals, bit for bit, the host composition ``match_lifts_host``,
    ``gather_view_tracks_host``, ``calibrate_views_host``, ``camera_to_world_host``, ``fuse_views_host``, ``solve_view_roots_host``,
    ``root_trajectory_host`` on ``predict_tracks`` of the flattened tracks.  Two persons with one body who move alike cannot be told
    apart; no matching accuracy is claimed."""
    import torch
    from . import predict as pt
    match = check_match(match)
    align = check_align(align)
    triangulate = check_triangulate(triangulate)
    calibrate = check_calibrate(calibrate)
    as_given = cameras
    lifts = isinstance(match, MatchLifts)
    if lifts and isinstance(align, AlignViews):
        raise ValueError("predict_views(match=MatchLifts(...)) does not take align=True or an AlignViews: the lifts are matched frame by frame on "
                         "one clock, and estimating offsets needs tracks that are matched already; pass known offsets as a list, which only crops")
    if calibrate is not None:
        if match is not None and not lifts:
            raise ValueError("predict_views(calibrate=...) does not take match: matching needs the rays in one world, which is what the call is "
                             "there to find; the same index must be the same person")
        if isinstance(align, AlignViews):
            raise ValueError("predict_views(calibrate=...) does not take align=True or an AlignViews: estimating offsets needs the rays in one "
                             "world; pass known offsets as a list, which only crops")
        # the cameras of every check and launch in front of the stage: where one has no extrinsics, the identity stands in
        cameras = [c if c.has_extrinsics else _with_identity(c)
                   for c in check_calibrate_cameras(cameras, len(views) if isinstance(views, (list, tuple)) else None)]
    if align is not None:
        def call(cropped, kept):
            return predict_views(model, config, cropped, as_given, resolutions, mask_stride, flip, reuse_frames, batch_size, depth, graph, kept, fps,
                                 model_fps, repair_joints, keypoints, min_root_joints, smooth, bones, rotations, interpolation, return_views,
                                 keyframes_only, out_fps, match, None, triangulate, calibrate)
        got = _predict_aligned_views(align, match, model, views, cameras, valid, fps, keyframes_only, out_fps, call)
        return got if calibrate is None else got[:-4] + got[-2:] + got[-4:-2]      # cameras and calibration stay the last two items
    if lifts:
        return _predict_lift_matched_views(pt, match, model, config, views, cameras, resolutions, mask_stride, flip, reuse_frames, batch_size, depth,
                                           graph, valid, fps, model_fps, repair_joints, keypoints, min_root_joints, smooth, bones, rotations,
                                           interpolation, return_views, keyframes_only, out_fps, triangulate, calibrate, as_given)
    if match is not None:
        return _predict_matched_views(pt, match, model, config, views, cameras, resolutions, mask_stride, flip, reuse_frames, batch_size, depth, graph,
                                      valid, fps, model_fps, repair_joints, keypoints, min_root_joints, smooth, bones, rotations, interpolation,
                                      return_views, keyframes_only, out_fps, triangulate)
    cams, V, N, frames = _check_views(views, cameras, valid, keyframes_only, out_fps)
    # the options of the N persons: what runs behind the fusion (the flattened front takes none of them)
    person = pt.stage_options(config, N, "track", True, keypoints, cams[0].without(distortion=True, extrinsics=True), min_root_joints, smooth,
                              bones, repair_joints, fps, None, interpolation=interpolation, rotations=rotations)
    flat = [t for tracks in views for t in tracks]
    flat_valid = valid if valid is None or isinstance(valid, str) else [f for flags in valid for f in flags]
    res = None if resolutions is None else pt.check_resolutions(resolutions, V, per="view")[np.repeat(np.arange(V), N)]
    rates = None if fps is None else pt.frame_rates(fps, N)
    # lens distortion: the tracks of the views that have it, one launch in front of everything else
    bent = [v for v in range(V) if cams[v].has_distortion]
    if bent:
        tr, _, given = _device_tracks([flat[v * N + i] for v in bent for i in range(N)], torch.device(model.device))
        src = torch.cat(tr, 0).contiguous() if len(tr) > 1 else tr[0].contiguous()
        src = undistort_rows(src, np.stack([cams[v].row() for v in bent for _ in range(N)]), given)
        for k, t in zip([v * N + i for v in bent for i in range(N)], torch.split(src, [int(n) for n in given], 0)):
            flat[k] = t
    pinhole = [cams[v].without(distortion=True, extrinsics=True) for v in range(V) for _ in range(N)]
    # 1. + 2. one run of the front, the windows, the forwards and the assembly over all V N tracks
    front = pt._assembled_tracks(model, config, flat, res, mask_stride, flip, False, reuse_frames, batch_size, True, depth, None, graph, flat_valid,
                                 None if rates is None else rates * V, None, model_fps, repair_joints, keypoints, pinhole, min_root_joints, None, None,
                                 None, interpolation)
    lens = np.asarray(front.lens, np.int64)[:N]
    R = int(lens.sum())
    if [int(n) for n in front.lens] != frames * V or tuple(front.out.shape[:1]) != (V * R,):
        raise ValueError("predict_views: the assembly did not return one frame per given frame")      # (cannot happen without out_fps / keyframes_only)
    J = int(front.out.shape[1])
    kp2d, flags = front.table.source
    kp2d, flags = kp2d.reshape(V, R, J, 2), None if flags is None else flags.reshape(V, R, J)
    # 2a. - 2e. where the cameras stand: every view's pose against view 0 from the lifts in camera axes, then the one copy
    calibration = None
    if calibrate is not None:
        cams, calibration = _calibrated_views(calibrate, as_given, front.out.reshape(V, R, J, 3), kp2d, flags, person.min_root_joints)
    # 3. every view's poses to world axes: the existing launch, poses only, one row of extrinsics per view block
    world, _ = camera_to_world_rows(front.out, None, None, np.stack([c.pose_row() for c in cams]), [R] * V)
    result = _fused_scene(pt, person, world.view(V, R, J, 3), kp2d, flags, cams, lens, rates, model_fps, return_views, triangulate,
                          int(config.ROOT_KEYTPOINT))
    return result if calibration is None else result + (cams, calibration)


def _calibrated_views(calibrate, as_given, lifts, kp2d, flags, min_joints):
    """Steps 1a. to 1e. of the module's docstring, "Where the cameras stand": ``lifts`` (V, R, J, 3) in camera axes, ``kp2d`` (V, R, J, 2) and
    ``flags`` None or (V, R, J) on the device; ``as_given``: the cameras of the call -> (the V cameras with extrinsics, per view (state,
    terms)).  A view without a pose is a ValueError that names it."""
    import torch
    V = int(kp2d.shape[0])
    rows = np.zeros((V, CALIBRATE_POSE + 1), np.float64)
    rows[0, 0] = rows[0, 7] = 1.0
    if V > 1:
        pose_dev, terms_dev = calibrate_views(lifts, kp2d, as_given, flags, min_joints, calibrate.min_terms)
        rows = torch.cat([pose_dev, terms_dev.to(torch.float64)[:, None]], 1).cpu().numpy()
    lost = [v for v in range(V) if rows[v, 7] != 1.0]
    if lost:
        raise ValueError(f"calibrate: view {lost[0]} cannot be calibrated against view 0 ({int(rows[lost[0], 8])} shared rows, {calibrate.min_terms} "
                         f"needed; or its lifts fix no rotation, or the rows fix no position) (views without a pose: {lost})")
    return calibrated_cameras(as_given, rows[:, :CALIBRATE_POSE]), [(int(rows[v, 7]), int(rows[v, 8])) for v in range(V)]


def _predict_lift_matched_views(pt, match, model, config, views, cameras, resolutions, mask_stride, flip, reuse_frames, batch_size, depth, graph,
                                valid, fps, model_fps, repair_joints, keypoints, min_root_joints, smooth, bones, rotations, interpolation,
                                return_views, keyframes_only, out_fps, triangulate, calibrate, as_given):
    """``predict_views(match=MatchLifts(...))``: the steps of its docstring, "Who is who without a world".  ``cameras``: every view's camera
    with extrinsics (under ``calibrate`` the identity stands in where one has none); ``as_given``: the cameras of the call."""
    import torch
    if keyframes_only:
        raise ValueError("predict_views does not take keyframes_only: the fusion needs one returned frame per given frame of every view")
    if out_fps is not None:
        raise ValueError("predict_views does not take out_fps: the fusion needs one returned frame per given frame of every view")
    cams, counts, flat, flat_valid, T = _match_inputs(views, cameras, valid)
    V, M = len(cams), len(flat)
    if calibrate is not None and counts[0] < 1:
        raise ValueError("calibrate: view 0 holds no track, and view 0 defines the world: put a camera that saw somebody first")
    if isinstance(bones, (list, tuple)):
        raise ValueError("predict_views(match=...) does not take bones as a per-person list: the persons are not known beforehand; "
                         "pass \"track\", one array of lengths or a Bones")
    rate = None
    if fps is not None:
        if isinstance(fps, (list, np.ndarray)):
            raise ValueError("predict_views(match=...) takes one fps for all tracks, not a list: they are on one clock")
        rate = pt.frame_rates(fps, 1)[0]
    # every refusal of the persons' options before any device work (they are checked again for the P persons found)
    pinhole0 = cams[0].without(distortion=True, extrinsics=True)
    first = pt.stage_options(config, 1, "track", True, keypoints, pinhole0, min_root_joints, smooth, bones, repair_joints, fps, None,
                             interpolation=interpolation, rotations=rotations)
    view_of = np.repeat(np.arange(V, dtype=np.int32), counts)
    res = None if resolutions is None else pt.check_resolutions(resolutions, V, per="view")[view_of]
    # 0. undistort; 1. one run of the front, the windows, the forwards and the assembly over the M tracks as given
    tr, _ = _undistorted_tracks(flat, cams, counts, torch.device(model.device))
    pinhole = [cams[v].without(distortion=True, extrinsics=True) for v in view_of]
    front = pt._assembled_tracks(model, config, tr, res, mask_stride, flip, False, reuse_frames, batch_size, True, depth, None, graph, flat_valid,
                                 None if rate is None else [rate] * M, None, model_fps, repair_joints, keypoints, pinhole, min_root_joints, None, None,
                                 None, interpolation)
    if [int(n) for n in front.lens] != [T] * M or tuple(front.out.shape[:1]) != (M * T,):
        raise ValueError("predict_views: the assembly did not return one frame per given frame")      # (cannot happen without out_fps / keyframes_only)
    J = int(front.out.shape[1])
    kp2d, flags = front.table.source
    kp2d, flags = kp2d.contiguous(), None if flags is None else flags.contiguous()
    # 2. who is who from the lifts in camera axes and the keypoints in the model's layout; the one copy of the route
    person_dev, count_dev, table_dev, _, _ = match_lifts(front.out.view(M, T, J, 3), kp2d.view(M, T, J, 2), view_of,
                                                         None if flags is None else flags.view(M, T, J), V, first.min_root_joints, match.max_dist,
                                                         match.min_terms)
    back = torch.cat([person_dev, count_dev, table_dev.reshape(-1)]).cpu().numpy()
    who, P, table = back[:M], int(back[M]), back[M + 1:].reshape(V, M)
    person = pt.stage_options(config, P, "track", True, keypoints, pinhole0, min_root_joints, smooth, bones, repair_joints, fps, None,
                              interpolation=interpolation, rotations=rotations)
    # 3. the persons' tracks, view-major and padded, still in camera axes: this route gathers before it turns the lifts to world axes
    src = _upload(table[:, :P], np.int32, front.out.device)
    lifts, kp2d, flags = gather_view_tracks(src, front.out, kp2d, flags, T)
    # 4. where the cameras stand, on the gathered buffers: a (view, person) pair without a track is rows the view does not SEE
    calibration = None
    if calibrate is not None:
        cams, calibration = _calibrated_views(calibrate, as_given, lifts, kp2d, flags, person.min_root_joints)
    # 5. every view's poses to world axes: one row of extrinsics per view block of P T rows
    world, _ = camera_to_world_rows(lifts.view(V * P * T, J, 3), None, None, np.stack([c.pose_row() for c in cams]), [P * T] * V)
    lens = np.full(P, T, np.int64)
    result = _fused_scene(pt, person, world.view(V, P * T, J, 3), kp2d, flags, cams, lens, None if rate is None else [rate] * P, model_fps,
                          return_views, triangulate, int(config.ROOT_KEYTPOINT))
    starts = np.concatenate([[0], np.cumsum(counts)])
    result += ([[int(k) for k in who[starts[v]:starts[v + 1]]] for v in range(V)],)
    return result if calibration is None else result + (cams, calibration)


def _predict_matched_views(pt, match, model, config, views, cameras, resolutions, mask_stride, flip, reuse_frames, batch_size, depth, graph, valid,
                           fps, model_fps, repair_joints, keypoints, min_root_joints, smooth, bones, rotations, interpolation, return_views,
                           keyframes_only, out_fps, triangulate=None):
    """``predict_views(match=...)``: the steps of its docstring, "Who is who"."""
    import torch
    if keyframes_only:
        raise ValueError("predict_views does not take keyframes_only: the fusion needs one returned frame per given frame of every view")
    if out_fps is not None:
        raise ValueError("predict_views does not take out_fps: the fusion needs one returned frame per given frame of every view")
    cams, counts, flat, flat_valid, T = _match_inputs(views, cameras, valid)
    V, M = len(cams), len(flat)
    if isinstance(bones, (list, tuple)):
        raise ValueError("predict_views(match=...) does not take bones as a per-person list: the persons are not known beforehand; "
                         "pass \"track\", one array of lengths or a Bones")
    rate = None
    if fps is not None:
        if isinstance(fps, (list, np.ndarray)):
            raise ValueError("predict_views(match=...) takes one fps for all tracks, not a list: they are on one clock")
        rate = pt.frame_rates(fps, 1)[0]
    # every refusal of the persons' options before any device work (they are checked again for the P persons found)
    pinhole0 = cams[0].without(distortion=True, extrinsics=True)
    pt.stage_options(config, 1, "track", True, keypoints, pinhole0, min_root_joints, smooth, bones, repair_joints, fps, None,
                     interpolation=interpolation, rotations=rotations)
    view_of = np.repeat(np.arange(V), counts)
    res = None if resolutions is None else pt.check_resolutions(resolutions, V, per="view")[view_of]
    # 0a. + 0b. undistort, then who is who on the detector's joints; the one copy of the call
    tr, _ = _undistorted_tracks(flat, cams, counts, torch.device(model.device))
    person_dev, count_dev, table_dev, _, _ = _match_device(tr, cams, counts, flat_valid, match)
    back = torch.cat([person_dev, count_dev, table_dev.reshape(-1)]).cpu().numpy()
    who, P, table = back[:M], int(back[M]), back[M + 1:].reshape(V, M)
    person = pt.stage_options(config, P, "track", True, keypoints, pinhole0, min_root_joints, smooth, bones, repair_joints, fps, None,
                              interpolation=interpolation, rotations=rotations)
    # 1. one run of the front, the windows, the forwards and the assembly over the M tracks as given
    pinhole = [cams[v].without(distortion=True, extrinsics=True) for v in view_of]
    front = pt._assembled_tracks(model, config, tr, res, mask_stride, flip, False, reuse_frames, batch_size, True, depth, None, graph, flat_valid,
                                 None if rate is None else [rate] * M, None, model_fps, repair_joints, keypoints, pinhole, min_root_joints, None, None,
                                 None, interpolation)
    if [int(n) for n in front.lens] != [T] * M or tuple(front.out.shape[:1]) != (M * T,):
        raise ValueError("predict_views: the assembly did not return one frame per given frame")      # (cannot happen without out_fps / keyframes_only)
    J = int(front.out.shape[1])
    kp2d, flags = front.table.source
    # 2. every track's poses to world axes: one row of extrinsics per non-empty view block of N_v T rows
    seen = [v for v in range(V) if counts[v] > 0]
    world, _ = camera_to_world_rows(front.out, None, None, np.stack([cams[v].pose_row() for v in seen]), [counts[v] * T for v in seen])
    # 0c. the persons' tracks, view-major and padded
    src = _upload(table[:, :P], np.int32, world.device)
    world, kp2d, flags = gather_view_tracks(src, world, kp2d.contiguous(), None if flags is None else flags.contiguous(), T)
    lens = np.full(P, T, np.int64)
    result = _fused_scene(pt, person, world, kp2d, flags, cams, lens, None if rate is None else [rate] * P, model_fps, return_views, triangulate,
                          int(config.ROOT_KEYTPOINT))
    starts = np.concatenate([[0], np.cumsum(counts)])
    return result + ([[int(k) for k in who[starts[v]:starts[v + 1]]] for v in range(V)],)
