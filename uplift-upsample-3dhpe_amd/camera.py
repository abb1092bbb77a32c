"""The lens stage of the track pipeline: a camera with radial and tangential distortion (include/uu3d.h, LENS DISTORTION).  ``Camera``
is what ``camera=`` takes beside a plain (fx, fy, cx, cy); wraps uu3d_undistort_points (``undistort_points``; the rule in numpy:
``undistort_points_host``); ``distort_points_host`` is the forward model, for building inputs.

Lens distortion -- ``predict_tracks(..., camera=Camera(fx, fy, cx, cy, distortion=(k1, k2, p1, p2, k3)))``: everything else in this package
reads a camera as an ideal pinhole -- the root solve back-projects raw pixels through (u - cx) / fx, the network reads raw pixels scaled by
the resolution.  A real lens puts a keypoint near the image border tens of pixels from where a pinhole would, and for a person off centre
that goes straight into the root's depth and lateral position.  With a ``Camera`` that has distortion the given 2D points are taken back,
on the device and before anything else looks at them, to the pixels a pinhole with the same intrinsics would have seen:
uu3d_undistort_points is the FIRST launch of the call -- on the given frames in the detector's layout, in front of uu3d_map_keypoints (an
affine joint map does not commute with distortion) -- and everything behind reads the undistorted points: the map, ``repair_joints``, the
normalisation or resampling, and the root solve.  The caller's memory is never written.  ``predict_detections`` undistorts all D x K points
of a frame before the association (one camera per video); ``StreamSession`` runs the launch as the first step of its one captured tick
(with ``fps`` in front of uu3d_stream_source_push, with ``detections`` in front of the association), from the staged push into a buffer
of the session: ``push`` still never waits and ``captures`` stays 1.  A point the rule does not accept comes back (NaN, NaN) and is a lost
joint for the finite tests behind: ``valid="finite"`` (and ``repair_joints``) is the companion option offline, ``missed_detections=True``
live; the root solve never uses it.  The result equals, bit for bit, the same call on ``undistort_points_host(tracks, camera)`` with
``camera=(fx, fy, cx, cy)``.  A ``Camera`` without distortion (None, or all coefficients zero) is the plain tuple: the same launches,
buffers and bits.  No accuracy is claimed: the mechanism is the feature.

World space -- ``camera=Camera(fx, fy, cx, cy, orientation=(w, x, y, z), translation=(tx, ty, tz))`` (include/uu3d.h, WORLD SPACE): the
scene a call with ``camera`` returns -- root-relative poses and a root per frame -- stands in the camera's own space, where "up" is a
slanted direction for every camera that is tilted or rolled.  With extrinsics, in the convention of ``h36m.camera_to_world``
(``X_world = qrot(orientation, X_cam) + translation``: the quaternion turns camera axes onto world axes, the translation is the camera's
position), uu3d_camera_to_world takes poses and roots to world axes in one launch BEHIND the root solve, which stays in camera space, and
IN FRONT of the ``smooth`` filters and of ``rotations``: the filters steady the floor's axes, and the quaternions and a BVH written from
them stand upright.  Poses are rotated only and stay root-relative (``poses + roots[:, None]`` is the world scene), a solved or held root
is rotated and translated, a root with state 0 stays zeros.  ``camera_to_world`` is the launch alone; ``camera_to_world_host`` is the rule
in numpy, bit for bit; ``world_to_camera_host`` its inverse in float64, for building inputs; ``extrinsics_from_opencv`` turns OpenCV's
world-to-camera (R, tvec) into the two keywords.  A ``Camera`` without extrinsics launches nothing new: the same buffers and bits."""
import copy
import ctypes as C

import numpy as np

from . import _capi
from ._capi import ptr as _ptr
from .roots import _root_lens, check_cameras
from .tracks import _host_array, _upload


class Camera(object):
    """A camera's intrinsics with lens distortion: ``Camera(fx, fy, cx, cy, distortion=(k1, k2, p1, p2, k3), tol=1e-3)``, in the units of
    the 2D points as given (pixels).  The coefficients follow OpenCV's Brown-Conrady order and model, which is what a calibration tool
    hands over (``cv2.calibrateCamera``'s ``distCoeffs``): with r2 = x x + y y on normalised coordinates,
        xd = x (1 + k1 r2 + k2 r2^2 + k3 r2^3) + 2 p1 x y + p2 (r2 + 2 x x)      yd = y (...) + p1 (r2 + 2 y y) + 2 p2 x y.
    Human3.6M's ``project_to_2d`` (and ``utils/h36m_cameras.json`` with it) uses a DIFFERENT tangential form -- with t = p1 x + p2 y it
    is ``xd = x (radial + t) + p1 r2`` -- so its coefficients cannot be passed here as they are; converting them is out of scope.
    ``distortion``: None or five finite numbers (anything else: ValueError); None and all zeros are "without distortion" -- the plain
    tuple.  ``tol`` (finite, > 0): the largest re-distortion residual, in pixels, at which an undistorted point is accepted.
    THE RULE (``undistort_points_host``; float64, every operation rounded once, one final rounding to float32) runs exactly ``ITERATIONS``
    = 20 steps of OpenCV's fixed-point iteration with no early exit.  20 is a constant of the rule, not a measurement: on a 41 x 41 grid
    over a 1920 x 1080 image at fx = 1145 the worst residual after 20 steps is 2.4e-9 normalised units (3e-6 px) for moderate
    coefficient sets (k1 down to -0.35 at a normalised radius of 1.17) and still 9e-6 units after 10; the default ``tol`` of 1e-3 px sits
    far above that noise and far below a detector's precision.
    EXTRINSICS (keyword only; module docstring, "World space"): ``orientation`` = the quaternion (w, x, y, z) that turns camera axes onto
    world axes, ``translation`` = the camera's position in the world in the poses' units (metres for the shipped configs) --
    ``X_world = qrot(orientation, X_cam) + translation``, the convention of ``h36m.camera_to_world`` and of ``utils/h36m_cameras.json``
    (whose translations are millimetres).  ``orientation``: four finite numbers, not all zero, normalised ONCE here in float64
    (``q / np.sqrt(w*w + x*x + y*y + z*z)``); ``translation``: three finite numbers, None = zeros, and a ValueError without
    ``orientation``.  ``extrinsics_from_opencv`` makes the pair from OpenCV's (R, tvec).  Without the two keywords nothing changes."""
    ITERATIONS = 20

    def __init__(self, fx, fy, cx, cy, distortion=None, tol=1e-3, *, orientation=None, translation=None):
        self.intrinsics = tuple(float(v) for v in check_cameras((fx, fy, cx, cy), 1, per="track")[0])
        if distortion is None:
            d = np.zeros(5, np.float64)
        else:
            try:
                d = np.asarray(distortion, np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"distortion must be five numbers (k1, k2, p1, p2, k3), got {distortion!r}") from None
            if d.shape != (5,):
                raise ValueError(f"distortion must be five numbers (k1, k2, p1, p2, k3), got shape {d.shape}")
            if not np.isfinite(d).all():
                raise ValueError("distortion must be finite (k1, k2, p1, p2, k3)")
        try:
            t = float(tol)
        except (TypeError, ValueError):
            raise ValueError(f"tol must be a finite number of pixels > 0, got {tol!r}") from None
        if isinstance(tol, bool) or not np.isfinite(t) or not t > 0:
            raise ValueError(f"tol must be a finite number of pixels > 0, got {tol!r}")
        self.distortion, self.tol = d, t
        self.orientation, self.translation = _check_extrinsics(orientation, translation)      # the unit quaternion and t, or (None, None)

    @property
    def has_distortion(self):
        return bool((self.distortion != 0).any())

    @property
    def has_extrinsics(self):
        return self.orientation is not None

    def row(self):
        """The ten doubles of the device call: fx, fy, cx, cy, k1, k2, p1, p2, k3, tol."""
        return np.concatenate([self.intrinsics, self.distortion, [self.tol]]).astype(np.float64)

    def pose_row(self):
        """The seven doubles of uu3d_camera_to_world: the normalised quaternion (w, x, y, z), then t.  Without extrinsics: ValueError."""
        if not self.has_extrinsics:
            raise ValueError("pose_row needs a Camera with extrinsics (orientation=, translation=)")
        return np.concatenate([self.orientation, self.translation]).astype(np.float64)

    def without(self, distortion=False, extrinsics=False):
        """A copy of this camera minus its distortion and / or its extrinsics; what stays keeps its bits (nothing is normalised twice)."""
        c = copy.copy(self)
        if distortion:
            c.distortion = np.zeros(5, np.float64)
        if extrinsics:
            c.orientation = c.translation = None
        return c

    def __repr__(self):
        fx, fy, cx, cy = self.intrinsics
        more = ""
        if self.has_extrinsics:
            more = f", orientation={tuple(self.orientation.tolist())!r}, translation={tuple(self.translation.tolist())!r}"
        return f"Camera({fx!r}, {fy!r}, {cx!r}, {cy!r}, distortion={tuple(self.distortion.tolist())!r}, tol={self.tol!r}{more})"


def _check_extrinsics(orientation, translation):
    """``Camera(orientation=, translation=)`` -> (the unit quaternion (4,) float64, t (3,) float64), or (None, None) without extrinsics."""
    if orientation is None:
        if translation is not None:
            raise ValueError("translation needs orientation: extrinsics are the pair (the identity is orientation=(1, 0, 0, 0))")
        return None, None
    try:
        q = np.asarray(orientation, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"orientation must be four numbers (w, x, y, z), got {orientation!r}") from None
    if q.shape != (4,):
        raise ValueError(f"orientation must be four numbers (w, x, y, z), got shape {q.shape}")
    if not np.isfinite(q).all() or not (q != 0).any():
        raise ValueError("orientation must be finite (w, x, y, z), not all zero")
    w, x, y, z = q
    q = q / np.sqrt(w * w + x * x + y * y + z * z)
    if not np.isfinite(q).all() or not (q != 0).any():               # (components whose squares leave float64's range)
        raise ValueError("orientation must be finite (w, x, y, z), not all zero")
    if translation is None:
        return q, np.zeros(3, np.float64)
    try:
        t = np.asarray(translation, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"translation must be three numbers (tx, ty, tz), got {translation!r}") from None
    if t.shape != (3,):
        raise ValueError(f"translation must be three numbers (tx, ty, tz), got shape {t.shape}")
    if not np.isfinite(t).all():
        raise ValueError("translation must be finite (tx, ty, tz)")
    return q, t


def _is_camera_list(camera):
    return isinstance(camera, (list, tuple)) and any(isinstance(c, Camera) for c in camera)


def split_cameras(camera, count, per="track"):
    """What ``camera=`` was given -> (the plain camera ``check_cameras`` takes, lens): ``lens`` is None -- nothing to undistort: None, plain
    tuples, ``Camera``s without distortion -- or the (count, 10) float64 rows of uu3d_undistort_points.  A list that mixes tuples and
    ``Camera``s, or ``Camera``s with and without distortion, is a ValueError; counts and intrinsics stay ``check_cameras``' to refuse."""
    if isinstance(camera, Camera):
        return camera.intrinsics, (np.tile(camera.row(), (int(count), 1)) if camera.has_distortion else None)
    if not _is_camera_list(camera):
        return camera, None
    if not all(isinstance(c, Camera) for c in camera):
        raise ValueError(f"camera must be plain (fx, fy, cx, cy) tuples or Camera objects, one or one per {per}, not a mix of the two")
    if len({c.has_distortion for c in camera}) > 1:
        raise ValueError(f"camera: the Camera objects of a list, one per {per}, must all have distortion or all have none")
    if len({c.has_extrinsics for c in camera}) > 1:
        raise ValueError(f"camera: the Camera objects of a list, one per {per}, must all have extrinsics or all have none")
    plain = [c.intrinsics for c in camera]
    if not camera[0].has_distortion:
        return plain, None
    check_cameras(plain, count, per=per)                                 # (a wrong count is refused in check_cameras' words)
    return plain, np.ascontiguousarray(np.stack([c.row() for c in camera]))


def world_rows(camera, count):
    """What ``camera=`` was given, after ``split_cameras`` and ``check_cameras`` have passed it -> None -- nothing to take to world axes:
    None, plain tuples, ``Camera``s without extrinsics -- or the (count, 7) float64 rows of uu3d_camera_to_world."""
    if isinstance(camera, Camera):
        return np.tile(camera.pose_row(), (int(count), 1)) if camera.has_extrinsics else None
    if not _is_camera_list(camera) or not camera[0].has_extrinsics:
        return None
    return np.ascontiguousarray(np.stack([c.pose_row() for c in camera]))


def plain_camera(camera):
    """``camera=`` as the checks that only look at its shape take it: a ``Camera`` as its (fx, fy, cx, cy), a list of them as a list."""
    if isinstance(camera, Camera):
        return camera.intrinsics
    if _is_camera_list(camera):
        return [c.intrinsics if isinstance(c, Camera) else c for c in camera]
    return camera


def _lens_rows(camera, lens, rows):
    """One ``Camera`` or one per track of ``lens`` rows -> ((tracks, 10) float64, rows per track)."""
    lens = _root_lens(lens, rows)
    cams = [camera] * len(lens) if isinstance(camera, Camera) else list(camera) if isinstance(camera, (list, tuple)) else None
    if cams is None or len(cams) != len(lens) or not all(isinstance(c, Camera) for c in cams):
        raise ValueError(f"camera must be one Camera or one per track ({len(lens)})")
    return np.ascontiguousarray(np.stack([c.row() for c in cams])), lens


def _radial_tangential(x, y, k1, k2, p1, p2, k3):
    """r2, the radial polynomial's inner sum and the two tangential terms at (x, y): the parenthesisation of the rule, written out."""
    r2 = x * x + y * y
    poly = ((k3 * r2 + k2) * r2 + k1) * r2
    dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return poly, dx, dy


def undistort_rows_host(kp, rows):
    """``undistort_points_host`` with the camera of every row of ``kp`` given as a (R, 10) float64 row of the device call."""
    uv = np.asarray(_host_array(kp), np.float32)
    cam = np.asarray(rows, np.float64).reshape((uv.shape[0], 10) + (1,) * (uv.ndim - 2))
    fx, fy, cx, cy, k1, k2, p1, p2, k3, tol = (cam[:, i] for i in range(10))
    with np.errstate(all="ignore"):
        u, v = uv[..., 0].astype(np.float64), uv[..., 1].astype(np.float64)
        x0 = (u - cx) / fx
        y0 = (v - cy) / fy
        x, y = x0, y0
        for _ in range(Camera.ITERATIONS):                               # exactly, no early exit
            poly, dx, dy = _radial_tangential(x, y, k1, k2, p1, p2, k3)
            ic = 1.0 / (1.0 + poly)
            x = (x0 - dx) * ic
            y = (y0 - dy) * ic
        # the acceptance check: the forward model on (x, y) must land on the observation
        poly, dx, dy = _radial_tangential(x, y, k1, k2, p1, p2, k3)
        rad = 1.0 + poly
        xd = x * rad + dx
        yd = y * rad + dy
        ex = np.abs(xd - x0) * fx
        ey = np.abs(yd - y0) * fy
        ok = np.isfinite(uv).all(axis=-1) & np.isfinite(x) & np.isfinite(y) & (ex <= tol) & (ey <= tol)
        out = np.stack([(fx * x + cx).astype(np.float32), (fy * y + cy).astype(np.float32)], axis=-1)
        ok &= np.isfinite(out).all(axis=-1)
    out[~ok] = np.float32(np.nan)
    return out


def undistort_points_host(kp, camera, lens=None):
    """The rule of LENS DISTORTION (include/uu3d.h) in numpy, written to be read: what uu3d_undistort_points computes, bit for bit.
    ``kp`` (R, ..., 2): raw points as a detector saw them (read as float32), or a list of such arrays, one per track (-> a list);
    ``camera``: one ``Camera`` or -- with ``lens``, rows per track; for a list its arrays -- one per track -> float32 of the same shape: the pixel an ideal pinhole with the same intrinsics would have seen, or (NaN, NaN).
    Per point, in float64, every operation rounded once (no fused multiply-add):
        x0 = (u - cx) / fx, y0 = (v - cy) / fy, x = x0, y = y0; then exactly ``Camera.ITERATIONS`` times
            r2 = x*x + y*y;  ic = 1.0 / (1.0 + ((k3*r2 + k2)*r2 + k1)*r2)
            dx = 2.0*p1*x*y + p2*(r2 + 2.0*x*x);  dy = p1*(r2 + 2.0*y*y) + 2.0*p2*x*y
            x = (x0 - dx)*ic;  y = (y0 - dy)*ic
    and the forward model once on the result: rad = 1.0 + ((k3*r2 + k2)*r2 + k1)*r2, xd = x*rad + dx, yd = y*rad + dy.  ACCEPTED iff
    everything is finite, |xd - x0|*fx <= tol and |yd - y0|*fy <= tol: (fx*x + cx, fy*y + cy), rounded once to float32.  Anything else
    -- a non-finite input, an observation outside the region where the model can be inverted -- is (NaN, NaN)."""
    if isinstance(kp, (list, tuple)) and len(kp) and all(hasattr(t, "shape") for t in kp):      # a list of tracks: one camera or one each
        parts = [np.asarray(_host_array(t), np.float32) for t in kp]
        sizes = [len(t) for t in parts]
        return np.split(undistort_points_host(np.concatenate(parts), camera, sizes if lens is None else lens), np.cumsum(sizes)[:-1])
    uv = np.asarray(_host_array(kp), np.float32)
    if uv.ndim < 2 or uv.shape[-1] != 2:
        raise ValueError(f"kp must be (R, ..., 2), got {uv.shape}")
    if lens is None and isinstance(camera, (list, tuple)) and len(camera) == 1:
        camera = camera[0]
    rows, lens = _lens_rows(camera, lens, uv.shape[0])
    return undistort_rows_host(uv, np.repeat(rows, lens, axis=0))


def distort_points_host(kp, camera):
    """The forward model in numpy, float64 in and out: ``kp`` (..., 2) ideal pinhole pixels -> the pixels the lens of ``camera`` (one
    ``Camera``) puts them at.  For building test inputs and for users; ``undistort_points_host`` inverts it where it can be inverted."""
    if not isinstance(camera, Camera):
        raise ValueError("camera must be a Camera")
    p = np.asarray(_host_array(kp), np.float64)
    if p.ndim < 1 or p.shape[-1] != 2:
        raise ValueError(f"kp must be (..., 2), got {p.shape}")
    fx, fy, cx, cy = camera.intrinsics
    x = (p[..., 0] - cx) / fx
    y = (p[..., 1] - cy) / fy
    poly, dx, dy = _radial_tangential(x, y, *camera.distortion.tolist())
    rad = 1.0 + poly
    return np.stack([fx * (x * rad + dx) + cx, fy * (y * rad + dy) + cy], axis=-1)


def undistort_rows(kp, rows, lens=None):
    """uu3d_undistort_points on the current stream with the cameras given as (tracks, 10) float64 rows (host); ``lens``: rows of ``kp``
    per track, None: one track.  ``kp`` (R, P, 2) float32 on the device, contiguous, only read -> a fresh (R, P, 2) buffer."""
    import torch
    lib = _capi.load_library()
    if not isinstance(kp, torch.Tensor) or not kp.is_cuda or kp.dim() != 3 or kp.shape[2] != 2 or kp.dtype != torch.float32 or not kp.is_contiguous():
        raise ValueError(f"kp must be a contiguous (R, P, 2) float32 device tensor, got {tuple(getattr(kp, 'shape', ()))}")
    dev = kp.device
    R, P = int(kp.shape[0]), int(kp.shape[1])
    lens = _root_lens(lens, R)
    rows = np.ascontiguousarray(np.asarray(rows, np.float64).reshape(len(lens), 10))
    cams = _upload(rows, np.float64, dev)
    row_track = None if len(lens) == 1 else _upload(np.repeat(np.arange(len(lens), dtype=np.int32), lens), np.int32, dev)
    out = torch.empty_like(kp)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_undistort_points(_ptr(kp), _ptr(out), R, P, _ptr(row_track), len(lens), _ptr(cams), C.c_void_p(stream)), None)
    return out


def undistort_points(kp, camera, lens=None):
    """uu3d_undistort_points on the current stream: ``undistort_points_host`` on a device tensor, one launch, nothing copies to the host
    or waits.  ``kp`` (R, P, 2) float32 on the device, contiguous (only read); ``camera``: one ``Camera`` or one per track with ``lens``
    (rows per track) -> a fresh (R, P, 2) float32 device buffer.  Needs no model."""
    rows, lens = _lens_rows(camera, lens, int(kp.shape[0]) if hasattr(kp, "shape") and len(kp.shape) else 0)
    return undistort_rows(kp, rows, lens)


# ---- world space (include/uu3d.h, WORLD SPACE) --------------------------------------------------------------------------------------
def extrinsics_from_opencv(R, tvec):
    """OpenCV's world-to-camera pair (``cv2.solvePnP`` / ``cv2.calibrateCamera`` with ``cv2.Rodrigues``), ``X_cam = R X_world + tvec``
    -> (orientation (w, x, y, z), translation (tx, ty, tz)), two float64 arrays for ``Camera(..., orientation=, translation=)``:
    ``orientation = quat(R^T)`` with w >= 0 and ``translation = -R^T tvec``, in float64.  ``R`` must be (3, 3) and a rotation:
    ``|R R^T - I|_inf > 1e-6`` or ``det R < 0`` (a reflection) is a ValueError.  The matrix-to-quaternion conversion branches on the
    largest of the trace and the three diagonal terms, so no small number is ever divided by."""
    try:
        R, t = np.asarray(R, np.float64), np.asarray(tvec, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("R must be a (3, 3) rotation matrix and tvec three numbers") from None
    if R.shape != (3, 3) or t.shape != (3,) or not np.isfinite(R).all() or not np.isfinite(t).all():
        raise ValueError(f"R must be a finite (3, 3) rotation matrix and tvec three finite numbers, got shapes {R.shape} and {t.shape}")
    if np.abs(R @ R.T - np.eye(3)).max() > 1e-6:
        raise ValueError("R is not orthonormal: |R R^T - I| > 1e-6")
    if np.linalg.det(R) < 0:
        raise ValueError("R is a reflection (det R < 0), not a rotation")
    m = R.T                                                              # camera axes onto world axes
    trace = m[0, 0] + m[1, 1] + m[2, 2]
    if trace > 0.0:
        s = 2.0 * np.sqrt(1.0 + trace)                                   # 4 w
        q = [0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
    elif m[0, 0] >= m[1, 1] and m[0, 0] >= m[2, 2]:
        s = 2.0 * np.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2])             # 4 x
        q = [(m[2, 1] - m[1, 2]) / s, 0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s]
    elif m[1, 1] >= m[2, 2]:
        s = 2.0 * np.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2])             # 4 y
        q = [(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s]
    else:
        s = 2.0 * np.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1])             # 4 z
        q = [(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s]
    q = np.array(q, np.float64)
    if q[0] < 0.0:
        q = -q
    return q, -(m @ t)


def _rotate_f64(q, a, b, c):
    """The rotation of WORLD SPACE on float64 arrays, the statements written out one by one (no ``np.cross``: every product and sum is
    one numpy operation, rounded once).  q = (w, x, y, z), broadcast against the point (a, b, c) -> (r0, r1, r2)."""
    w, x, y, z = q
    uv0 = y * c - z * b
    uv1 = z * a - x * c
    uv2 = x * b - y * a
    uuv0 = y * uv2 - z * uv1
    uuv1 = z * uv0 - x * uv2
    uuv2 = x * uv1 - y * uv0
    r0 = a + 2.0 * (w * uv0 + uuv0)
    r1 = b + 2.0 * (w * uv1 + uuv1)
    r2 = c + 2.0 * (w * uv2 + uuv2)
    return r0, r1, r2


def _camera_to_world_f64(points, rows, place):
    """The rule BEFORE its final rounding: ``points`` (R, ..., 3), read as float32 and widened; ``rows`` (R, 7) float64, the camera of
    every row (``Camera.pose_row``); ``place``: add t (roots), else rotate only (poses) -> (R, ..., 3) float64."""
    v = np.asarray(_host_array(points), np.float32).astype(np.float64)
    ext = np.asarray(rows, np.float64).reshape((v.shape[0], 7) + (1,) * (v.ndim - 2))
    with np.errstate(all="ignore"):
        r0, r1, r2 = _rotate_f64([ext[:, i] for i in range(4)], v[..., 0], v[..., 1], v[..., 2])
        if place:
            r0 = r0 + ext[:, 4]
            r1 = r1 + ext[:, 5]
            r2 = r2 + ext[:, 6]
    return np.stack([r0, r1, r2], axis=-1)


def _world_rows(camera, lens, rows):
    """One ``Camera`` with extrinsics or one per track of ``lens`` rows -> ((tracks, 7) float64, rows per track)."""
    lens = _root_lens(lens, rows)
    cams = [camera] * len(lens) if isinstance(camera, Camera) else list(camera) if isinstance(camera, (list, tuple)) else None
    if cams is None or len(cams) != len(lens) or not all(isinstance(c, Camera) and c.has_extrinsics for c in cams):
        raise ValueError(f"camera must be one Camera with extrinsics or one per track ({len(lens)})")
    return np.ascontiguousarray(np.stack([c.pose_row() for c in cams])), lens


def _world_shapes(poses, roots, root_state):
    """The shapes of a WORLD SPACE call -> its rows.  ``poses`` (R, J, 3) or None; ``roots`` (R, 3) and ``root_state`` (R,), or both None."""
    if (roots is None) != (root_state is None) or (poses is None and roots is None):
        raise ValueError("camera_to_world takes poses, roots with their root_state, or both")
    ps, rs, ss = (None if a is None else tuple(a.shape) for a in (poses, roots, root_state))
    if ps is not None and (len(ps) != 3 or ps[2] != 3 or ps[1] < 1):
        raise ValueError(f"poses must be (R, J, 3), got {ps}")
    R = ps[0] if ps is not None else rs[0] if len(rs) else -1
    if rs is not None and (rs != (R, 3) or ss != (R,)):
        raise ValueError(f"roots must be (R, 3) and root_state (R,) with the R = {R} rows of the poses, got {rs} and {ss}")
    return int(R)


def camera_to_world_rows_host(poses, roots, root_state, rows):
    """``camera_to_world_host`` with the camera of every row given as a (R, 7) float64 row of the device call."""
    poses, roots = (None if a is None else np.asarray(_host_array(a), np.float32) for a in (poses, roots))
    state = None if root_state is None else np.asarray(_host_array(root_state))
    _world_shapes(poses, roots, state)
    with np.errstate(all="ignore"):
        out = None if poses is None else _camera_to_world_f64(poses, rows, False).astype(np.float32)
        placed = None
        if roots is not None:
            placed = _camera_to_world_f64(roots, rows, True).astype(np.float32)
            placed[state == 0] = np.float32(0.0)
    return out, placed


def camera_to_world_host(poses, roots, root_state, camera, lens=None):
    """The rule of WORLD SPACE (include/uu3d.h) in numpy, written to be read: what uu3d_camera_to_world computes, bit for bit.
    ``poses`` (R, J, 3) or None, ``roots`` (R, 3) with ``root_state`` (R,) or both None (read as float32 / as they are; host arrays or
    tensors); ``camera``: one ``Camera`` with extrinsics or -- with ``lens``, rows per track -- one per track
    -> (poses, roots) float32, None where None was given.  With q = (w, x, y, z) the camera's unit quaternion, t its position and
    v = (a, b, c) a point, in float64 on the float32 input, every operation rounded once (no fused multiply-add):
        uv  = (y*c - z*b,      z*a - x*c,      x*b - y*a)
        uuv = (y*uv2 - z*uv1,  z*uv0 - x*uv2,  x*uv1 - y*uv0)
        r_i = v_i + 2.0 * (w*uv_i + uuv_i)
    A joint of a pose becomes float32(r_i): rotated only, so the poses stay root-relative and the root joint's exact zeros stay +0.0.  A
    root whose state is not 0 becomes float32(r_i + t_i); a root with state 0 stays zeros.  NaN in, NaN out."""
    given = poses if poses is not None else roots
    rows, lens = _world_rows(camera, lens, int(given.shape[0]) if hasattr(given, "shape") and len(given.shape) else 0)
    return camera_to_world_rows_host(poses, roots, root_state, np.repeat(rows, lens, axis=0))


def world_to_camera_host(points, camera):
    """The inverse of the rule in float64, in and out: ``points`` (..., 3) in world axes -> the same points in the space of ``camera`` (one
    ``Camera`` with extrinsics): ``qrot(conj(q), X_world - t)``.  For building test inputs and for users."""
    if not isinstance(camera, Camera) or not camera.has_extrinsics:
        raise ValueError("camera must be a Camera with extrinsics")
    p = np.asarray(_host_array(points), np.float64)
    if p.ndim < 1 or p.shape[-1] != 3:
        raise ValueError(f"points must be (..., 3), got {p.shape}")
    w, x, y, z = camera.orientation.tolist()
    d = p - camera.translation
    return np.stack(_rotate_f64((w, -x, -y, -z), d[..., 0], d[..., 1], d[..., 2]), axis=-1)


def camera_to_world_rows(poses, roots, root_state, rows, lens=None, in_place=False):
    """uu3d_camera_to_world on the current stream with the cameras given as (tracks, 7) float64 rows (host); ``lens``: rows per track,
    None: one track.  ``poses`` (R, J, 3) float32 or None, ``roots`` (R, 3) float32 with ``root_state`` (R,) uint8 or both None: device
    tensors, contiguous -> (poses, roots): fresh buffers (None where None was given), or with ``in_place`` the given ones, overwritten."""
    import torch
    lib = _capi.load_library()
    for name, a, dtype in (("poses", poses, torch.float32), ("roots", roots, torch.float32), ("root_state", root_state, torch.uint8)):
        if a is not None and (not isinstance(a, torch.Tensor) or not a.is_cuda or a.dtype != dtype or not a.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {str(dtype).split('.')[-1]} device tensor")
    R = _world_shapes(poses, roots, root_state)
    given = poses if poses is not None else roots
    dev = given.device
    lens = _root_lens(lens, R)
    rows = np.ascontiguousarray(np.asarray(rows, np.float64).reshape(len(lens), 7))
    ext = _upload(rows, np.float64, dev)
    row_track = None if len(lens) == 1 else _upload(np.repeat(np.arange(len(lens), dtype=np.int32), lens), np.int32, dev)
    out = None if poses is None else poses if in_place else torch.empty_like(poses)
    placed = None if roots is None else roots if in_place else torch.empty_like(roots)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_camera_to_world(_ptr(poses), _ptr(out), _ptr(roots), _ptr(root_state), _ptr(placed), R,
                                                  int(poses.shape[1]) if poses is not None else 1, _ptr(row_track), len(lens), _ptr(ext),
                                                  C.c_void_p(stream)), None)
    return out, placed


def camera_to_world(poses, roots, root_state, camera, lens=None):
    """uu3d_camera_to_world on the current stream: ``camera_to_world_host`` on device tensors, one launch, nothing copies to the host or
    waits.  ``poses`` (R, J, 3) float32 or None, ``roots`` (R, 3) float32 with ``root_state`` (R,) uint8 or both None (only read);
    ``camera``: one ``Camera`` with extrinsics or one per track with ``lens`` (rows per track) -> (poses, roots), fresh device buffers
    (None where None was given).  Needs no model."""
    given = poses if poses is not None else roots
    rows, lens = _world_rows(camera, lens, int(given.shape[0]) if hasattr(given, "shape") and len(given.shape) else 0)
    return camera_to_world_rows(poses, roots, root_state, rows, lens)


class LiveWorld(object):
    """uu3d_camera_to_world as an output-side stage of a ``StreamSession`` (``smooth.LiveOneEuro``'s interface): stateless, all slots at every tick, nothing to reset."""

    def __init__(self, slots, joints, rows, device):
        import torch
        self._lib = _capi.load_library()
        self.slots, self.joints = slots, joints
        self._world = _upload(rows, rows.dtype, device)
        self._track = torch.arange(slots, dtype=torch.int32, device=device)
        self.poses = torch.zeros((slots, joints, 3), dtype=torch.float32, device=device)
        self.roots = torch.zeros((slots, 3), dtype=torch.float32, device=device)
        self.outputs = (("poses", "world_poses", self.poses), ("roots", "world_roots", self.roots))

    def launch(self, active=None, frames=None, drain_state=None):
        read = self.read
        return (self._lib.uu3d_camera_to_world, (_ptr(read.poses), _ptr(self.poses), _ptr(read.roots), _ptr(read.root_state), _ptr(self.roots),
                                                 self.slots, self.joints, _ptr(self._track), self.slots, _ptr(self._world)))
