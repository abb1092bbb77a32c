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
passes NaN coordinates (with ``valid="finite"``) or cleared flags there.  Out of scope: finding which detection of one camera is which
of another, time alignment, per-view confidence weights, estimating extrinsics, a live form.  No accuracy is claimed."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import ptr as _ptr
from .camera import Camera, _rotate_f64, camera_to_world_rows, undistort_rows
from .roots import DEFAULT_MIN_ROOT_JOINTS, MAX_ROOT_JOINTS, check_min_root_joints
from .tracks import _device_tracks, _host_array, _shape, _upload

MAX_VIEWS = 8                                                          # kViewsMax
VIEW_RANK = 2.0 ** -40                                                 # kViewRank


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


def predict_views(model, config, views, cameras, resolutions=None, mask_stride=None, flip=None, reuse_frames=True, batch_size=None, depth=None,
                  graph=True, valid=None, fps=None, model_fps=50, repair_joints=None, keypoints=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS,
                  smooth=None, bones=None, rotations=None, interpolation="linear", return_views=False, keyframes_only=False, out_fps=None):
    """One world scene from V calibrated views of the same N persons -> (poses, roots, root_state, view_count): per person ``poses``
    (T_i, J, 3) float32 in world axes and root-relative, ``roots`` (T_i, 3) float32 in world coordinates, ``root_state`` (T_i,) uint8 (1
    solved here, 2 interpolated or held, 0 no solved frame) and ``view_count`` (T_i,) uint8, the views that saw the frame; on the model's
    device, views of one buffer each.  ``rotations`` appends the quaternion lists as ``predict_tracks`` does; ``return_views=True`` then
    appends the per-view world poses the fusion read, a list of V lists.

    ``views``: a list of V lists, 1 <= V <= 8; ``views[v][i]`` is person i's 2D track in camera v, (T_i, J, 2), or (T_i, K_in, 2) with
    ``keypoints``.  The same index is the same person, frames are time-synchronised and person i has the same T_i in every view (anything
    else: ValueError; finding who is who across cameras and aligning clocks are out of scope).  A view that does not see the person at a
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
    ``joint_rotations_host``.  No accuracy is claimed."""
    import torch
    from . import predict as pt
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
    # 3. every view's poses to world axes: the existing launch, poses only, one row of extrinsics per view block
    world, _ = camera_to_world_rows(front.out, None, None, np.stack([c.pose_row() for c in cams]), [R] * V)
    # 4. the fusion
    kp2d, flags = kp2d.reshape(V, R, J, 2), None if flags is None else flags.reshape(V, R, J)
    fused, view_count, _ = fuse_views(world.view(V, R, J, 3), kp2d, flags, person.min_root_joints)
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
    result = tuple(list(torch.split(a, sizes, 0)) for a in (shown, roots, root_state, view_count))
    if person.rotations is not None:
        turned = pt.joint_rotations(shown, person.rotations)
        result += (list(torch.split(turned[0], sizes, 0)),) + ((list(torch.split(turned[2], sizes, 0)),) if person.rotations.return_global else ())
    if return_views:
        result += ([list(torch.split(block, sizes, 0)) for block in world.view(V, R, J, 3)],)
    return result
