"""CPU: joint rotations (include/uu3d.h, JOINT ROTATIONS; rotations.joint_rotations_host, Rotations, forward_kinematics; bvh) -- the
properties of the rule in numpy on seeded random poses of h36m17 and two made-up trees, every degenerate input against its stated
fallback and flag, the refusals that need no device, the unchanged surface, and the BVH round trip."""
import ast
import inspect
import os
import types

import numpy as np
import pytest

from tests import util

TREE_A = [-1, 0, 0, 1, 1, 2, 4]                                       # two forks; its rest bones are axis-aligned, no fork collinear
REST_A = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
TREE_B = [1, -1, 1, 1, 3, 3]                                          # the root is joint 1, with three children; joint 3 forks again
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0])


def _cases():
    from uplift_upsample_3dhpe_amd import predict
    rest_b = np.random.default_rng(5).normal(size=(6, 3)) * 3.0      # (any lengths: only directions matter)
    return {"h36m17": predict.Rotations("h36m17"), "tree_a": predict.Rotations(REST_A, predict.Skeleton(TREE_A)),
            "tree_b": predict.Rotations(rest_b, predict.Skeleton(TREE_B), primary={1: 2}, secondary={1: 3})}


def _random_unit(rng, shape):
    q = rng.normal(size=shape + (4,))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _cube_group():
    """The 24 rotations that map the coordinate axes onto each other, as unit quaternions: poses made of them from axis-aligned rest
    bones and dyadic lengths are exactly representable in float32."""
    h, r = 0.5, np.sqrt(0.5)
    qs = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]
    qs += [(h, a * h, b * h, c * h) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
    qs += [(r, s * r, 0, 0) for s in (1, -1)] + [(r, 0, s * r, 0) for s in (1, -1)] + [(r, 0, 0, s * r) for s in (1, -1)]
    qs += [(0, r, s * r, 0) for s in (1, -1)] + [(0, r, 0, s * r) for s in (1, -1)] + [(0, 0, r, s * r) for s in (1, -1)]
    return np.array(qs, np.float64)


def _own_lengths(X, sk):
    par = np.array(sk.parents)
    X = np.asarray(X, np.float64)
    return np.where(par >= 0, np.linalg.norm(X - X[:, np.where(par >= 0, par, 0)], axis=2), 0.0)


def _canonical(q):
    w, x, y, z = (q[..., k] for k in range(4))
    return (w > 0) | ((w == 0) & ((x > 0) | ((x == 0) & ((y > 0) | ((y == 0) & (z > 0))))))


# ---- properties of the rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["h36m17", "tree_a", "tree_b"])
def test_unit_canonical_and_leaves(name):
    from uplift_upsample_3dhpe_amd import rotations
    R = _cases()[name]
    J = R.skeleton.joints
    X = np.random.default_rng(1).normal(size=(40, J, 3)).astype(np.float32)
    local, flags, glob = rotations.joint_rotations_host(X, R, return_global=True)
    assert local.shape == (40, J, 4) and local.dtype == np.float32 and flags.shape == (40, J) and flags.dtype == np.uint8 and glob.dtype == np.float32
    for q in (local, glob):
        assert np.abs(np.linalg.norm(q.astype(np.float64), axis=-1) - 1.0).max() <= 2.0 ** -23
    assert _canonical(local).all() and (flags == 1).all()
    leaves = [j for j in range(J) if R.primary[j] < 0]
    assert leaves and (local[:, leaves] == IDENTITY.astype(np.float32)).all()
    # two outputs or three, the same bits; and the float64 form rounds to the float32 one
    again = rotations.joint_rotations_host(X, R)
    assert len(again) == 2 and np.array_equal(again[0], local)
    assert np.array_equal(rotations.joint_rotations_host(X, R, rounded=False)[0].astype(np.float32), local)


@pytest.mark.parametrize("name", ["h36m17", "tree_a"])
def test_rest_pose_gives_identities(name):
    """The rest pose itself, at any lengths and anywhere: every local quaternion is the identity.  Axis-aligned rest bones, lengths and a
    translation that are multiples of 1/8 keep the float32 pose exact, so the identities are exact as well."""
    from uplift_upsample_3dhpe_amd import rotations
    R = _cases()[name]
    J = R.skeleton.joints
    rng = np.random.default_rng(2)
    for _ in range(4):
        L = rng.integers(1, 17, J) / 8.0
        X = rotations.forward_kinematics(np.tile(IDENTITY, (3, J, 1)), R, L, root=rng.integers(-40, 41, (3, 3)) / 8.0)
        local, flags = rotations.joint_rotations_host(X.astype(np.float32), R)
        assert np.array_equal(X.astype(np.float32).astype(np.float64), X)
        assert (local == IDENTITY.astype(np.float32)).all() and (flags == 1).all()


@pytest.mark.parametrize("name", ["h36m17", "tree_a", "tree_b"])
def test_rotating_the_pose_changes_only_the_root(name):
    """A rotated pose is not a float32 pose, so the rule takes both as float64 arrays (``exact_input``): what is compared is the rule."""
    from uplift_upsample_3dhpe_amd import rotations
    R = _cases()[name]
    J, root = R.skeleton.joints, R.skeleton.root
    rng = np.random.default_rng(3)
    X = rng.normal(size=(30, J, 3)).astype(np.float32).astype(np.float64)
    turn = _random_unit(rng, (30,))
    M = rotations.quat_to_matrix(turn)
    Y = np.einsum("gab,gjb->gja", M, X)
    a = rotations.joint_rotations_host(X, R, rounded=False, exact_input=True)[0]
    b = rotations.joint_rotations_host(Y, R, rounded=False, exact_input=True)[0]
    others = [j for j in range(J) if j != root]
    assert np.abs(a[:, others] - b[:, others]).max() <= 1e-12
    want = rotations._mul(turn, a[:, root])
    assert np.minimum(np.abs(b[:, root] - want).max(-1), np.abs(b[:, root] + want).max(-1)).max() <= 1e-12


@pytest.mark.parametrize("name", ["h36m17", "tree_a", "tree_b"])
def test_forward_kinematics_gives_every_primary_bone_back(name):
    """FK of the quaternions with the pose's own bone lengths: the direction of every primary bone, relative to its length -- 1e-12 for the
    float64 quaternions, 1e-6 for the float32 ones (a component moves by <= 2^-25, an angle by < 2.4e-7 rad)."""
    from uplift_upsample_3dhpe_amd import rotations
    R = _cases()[name]
    sk = R.skeleton
    X = np.random.default_rng(4).normal(size=(60, sk.joints, 3)).astype(np.float32)
    L = _own_lengths(X, sk)
    for rounded, bound in ((False, 1e-12), (True, 1e-6)):
        local = rotations.joint_rotations_host(X, R, rounded=rounded)[0]
        Y = rotations.forward_kinematics(local, R, L, root=X[:, sk.root])
        worst = 0.0
        for p in range(sk.joints):
            c = int(R.primary[p])
            if c >= 0:
                worst = max(worst, (np.linalg.norm((Y[:, c] - Y[:, p]) - (X[:, c].astype(np.float64) - X[:, p]), axis=1) / L[:, c]).max())
        print(f"{name} rounded={rounded}: primary bone direction error {worst:.3e} (bound {bound:g})")
        assert worst <= bound


def _assert_joints_come_back(name, rounded, bound, sk, X, Y, L):
    """Every joint of the FK pose Y against the pose X.  (1) Every joint relative to its parent -- every bone, primary or not -- to
    ``bound``, relative to the bone's length: the measure of the primary-bone test.  (2) Every joint's position: it adds the bones of its
    path up, and the bone to a joint of level l is turned by the product of l quaternions, each off by at most e (2.4e-7 rad rounded to
    float32; 1e-12 is taken for the float64 ones), so the position of joint j is off by at most e * sum over its path of l(a) * L[a]."""
    X = np.asarray(X, np.float64)
    par = np.array(sk.parents)
    bones = [j for j in range(sk.joints) if j != sk.root]
    per_bone = max((np.linalg.norm((Y[:, j] - Y[:, par[j]]) - (X[:, j] - X[:, par[j]]), axis=1) / L[j]).max() for j in bones)
    e = 2.4e-7 if rounded else 1e-12
    budget = np.array([sum((i + 1) * L[a] for i, a in enumerate(sk.paths[j])) for j in range(sk.joints)])
    position = max((np.linalg.norm(Y[:, j] - X[:, j], axis=1) / budget[j]).max() for j in bones)
    print(f"{name} rounded={rounded}: bone error {per_bone:.3e} of its length (bound {bound:g}); position error {position:.3e} of its budget (bound {e:g})")
    assert per_bone <= bound and position <= e


@pytest.mark.parametrize("name", ["h36m17", "tree_a"])
def test_forward_kinematics_gives_a_consistent_rigid_pose_back(name):
    """Poses made by FK from random locals, sent through ``fix_bones_host``: every joint comes back, to the bounds of the test above
    (``_assert_joints_come_back``).  A float32 pose holds its secondary bones consistent with the rest pose only where it is exact, so the
    random locals are the 24 axis-permuting rotations on axis-aligned rest bones with lengths in eighths: every coordinate is a multiple
    of 1/8 (a float64 product of such rotations is off by ~1e-16, far below the bound).  Many of these bones are exactly antiparallel
    to where the parent's frame has them, and many secondary projections exactly opposite: both half-turn branches are run."""
    from uplift_upsample_3dhpe_amd import predict, rotations
    R = _cases()[name]
    sk = R.skeleton
    J = sk.joints
    rng = np.random.default_rng(6)
    group = _cube_group()
    G = 200
    local = group[rng.integers(0, 24, (G, J))]
    L = rng.integers(2, 17, J) / 8.0
    L[sk.root] = 0.0
    X = predict.fix_bones_host(rotations.forward_kinematics(local, R, L, root=rng.integers(-16, 17, (G, 3)) / 8.0).astype(np.float32), None, L, sk)
    for rounded, bound in ((False, 1e-12), (True, 1e-6)):
        got, flags = rotations.joint_rotations_host(X, R, rounded=rounded)
        Y = rotations.forward_kinematics(got, R, L, root=X[:, sk.root])
        _assert_joints_come_back(name, rounded, bound, sk, X, Y, L)
        assert (flags == 1).all()


@pytest.mark.parametrize("name", ["h36m17", "tree_a", "tree_b"])
def test_forward_kinematics_of_any_consistent_pose(name):
    """The same with any random locals and lengths: such a pose is not a float32 pose, so the rule takes it as float64 (``exact_input``)."""
    from uplift_upsample_3dhpe_amd import rotations
    R = _cases()[name]
    sk = R.skeleton
    J = sk.joints
    rng = np.random.default_rng(7)
    L = rng.uniform(0.2, 1.5, J)
    X = rotations.forward_kinematics(_random_unit(rng, (50, J)), R, L, root=rng.normal(size=(50, 3)))
    for rounded, bound in ((False, 1e-12), (True, 1e-6)):
        got = rotations.joint_rotations_host(X, R, rounded=rounded, exact_input=True)[0]
        Y = rotations.forward_kinematics(got, R, L, root=X[:, sk.root])
        _assert_joints_come_back(name, rounded, bound, sk, X, Y, L)


# ---- degenerate inputs -----------------------------------------------------------------------------------------------------------------
def degenerate_rows():
    """(Rotations, poses (G, 5, 3) float32, what each row is) on the tree 0 -> 1 -> {2, 3}, 3 -> 4 with axis-aligned rest bones: row 0 a
    plain pose, 1 a zero-length primary bone, 2 a NaN joint, 3-5 exactly antiparallel bones along x, y, z, 6 a zero secondary projection."""
    from uplift_upsample_3dhpe_amd import predict
    sk = predict.Skeleton([-1, 0, 1, 1, 3])
    R = predict.Rotations(np.array([[0, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 0, 1]], np.float64), sk, return_global=True)
    base = np.array([[0, 0, 0], [0, 1, 0], [1, 1, 0], [0, 1, 1], [0, 1, 2]], np.float32)     # the rest pose
    rows = np.tile(base, (7, 1, 1))
    rows[0] = np.random.default_rng(8).normal(size=(5, 3))
    rows[1, 1:] -= rows[1, 1] - rows[1, 0]                            # joint 0's primary bone has no length: joint 1 and all below it move up
    rows[2, 2] = np.nan                                               # joint 1's primary child is nowhere
    for k, axis in enumerate(np.eye(3, dtype=np.float32)):            # a chain along -axis where the rest pose ...
        rows[3 + k] = 0.0
        rows[3 + k, 1:] = -axis                                       # (joints 2, 3, 4 on joint 1: degenerate bones below it)
    rows[6, 3] = rows[6, 1] + 2.0 * (rows[6, 2] - rows[6, 1])        # joint 1's secondary bone along its primary one
    rows[6, 4] = rows[6, 3] + base[4] - base[3]                       # (joint 3's own bone as in the rest pose)
    return R, rows


def test_degenerate_inputs_fall_back_as_stated():
    from uplift_upsample_3dhpe_amd import rotations
    R, X = degenerate_rows()
    local, flags, glob = rotations.joint_rotations_host(X, R)
    one = IDENTITY.astype(np.float32)
    assert np.isfinite(local).all() and np.isfinite(glob).all() and _canonical(local).all()
    assert (flags[0] == 1).all()
    # 1: the root's primary bone is zero -> the root keeps its parent's frame (the identity), flag 0; below it the rest pose is intact
    assert flags[1].tolist() == [0, 1, 1, 1, 1] and (local[1] == one).all() and (glob[1] == one).all()
    # 2: the NaN joint is joint 1's primary child -> joint 1 falls back, flag 0; joint 2 is a leaf (identity, flag 1); joint 3 is fine
    assert flags[2].tolist() == [1, 0, 1, 1, 1] and (local[2] == one).all()
    # ... and as a SECONDARY child a NaN joint only drops the twist: the flag stays 1 and the primary bone is followed
    swapped = type(R)(R.rest, R.skeleton, primary={1: 3}, secondary={1: 2})
    l2, f2 = rotations.joint_rotations_host(X[2:3], swapped)
    assert f2.tolist() == [[1, 1, 1, 1, 1]] and (l2 == one).all()
    # 3-5: the root's rest bone is +y; antiparallel poses along each axis of a two-joint tree give the stated half turns
    from uplift_upsample_3dhpe_amd import predict
    two = predict.Skeleton([-1, 0])
    want = {0: [0, 0, 0, 1], 1: [0, 0, 0, 1], 2: [0, 0, 1, 0]}     # a x e: e1 for a = e0 -> e2; e0 for a = e1 -> -e2, made positive; e0 for a = e2 -> e1
    for k in range(3):
        a = np.eye(3)[k]
        pose = np.stack([np.zeros(3), -a])[None].astype(np.float32)
        l, f, g = rotations.joint_rotations_host(pose, predict.Rotations(np.stack([np.zeros(3), a]), two), return_global=True)
        assert f.tolist() == [[1, 1]] and l[0, 0].tolist() == want[k] and (l[0, 1] == one).all(), (k, l)
        assert np.allclose(rotations._rotate(g[0, 0].astype(np.float64), a), -a, atol=1e-15)
    assert (flags[3:6, 0] == 1).all() and (flags[3:6, 1] == 0).all()  # (rows 3-5: joint 1's children sit on it)
    # 6: the secondary bone projects to zero across the primary one -> no twist: the quaternions of the rest pose, flags 1
    assert (flags[6] == 1).all() and (local[6] == one).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from uplift_upsample_3dhpe_amd import predict, rotations, stream
    cfg = util.load_config("h36m_81")
    chain3 = predict.Skeleton([-1, 0, 1])
    with pytest.raises(ValueError, match="17 joints, the poses have 16"):
        rotations.check_rotations(True, 16)
    small = cfg.copy()
    small.NUM_KEYPOINTS = 16
    with pytest.raises(ValueError, match="Skeleton"):
        predict.predict_tracks(None, small, [np.zeros((4, 16, 2), np.float32)], rotations=True)
    with pytest.raises(ValueError, match="rotations must be"):
        predict.predict_tracks(None, cfg, [np.zeros((4, 17, 2), np.float32)], rotations="h36m17")
    with pytest.raises(ValueError, match="the poses have 17"):
        rotations.joint_rotations_host(np.zeros((1, 17, 3), np.float32), chain3, np.ones((3, 3)))
    for bad in (np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0.0]]), np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0.0]])):
        with pytest.raises(ValueError, match="zero or not finite"):
            predict.Rotations(bad, chain3)
    predict.Rotations(np.array([[np.nan] * 3, [1, 0, 0], [1, 0, 0.0]]), chain3)     # (the root's row is ignored)
    with pytest.raises(ValueError, match="needs \\(3, 3\\)"):
        predict.Rotations(np.ones((4, 3)), chain3)
    with pytest.raises(ValueError, match="J <= 64"):                  # more than 64 joints: no such Skeleton, so no such Rotations
        predict.Rotations(np.ones((65, 3)), predict.Skeleton([-1] + list(range(64))))
    fork = predict.Skeleton([-1, 0, 0, 1])
    rest = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0]])
    for kw, what in ((dict(primary={0: 3}), "primary: joint 3 is not a child of joint 0"), (dict(secondary={0: 3}), "secondary: joint 3 is not a child"),
                     (dict(primary={1: 3}, secondary={1: 3}), "must be another one"), (dict(primary=[5, -1, -1, -1]), "not a child"),
                     (dict(primary="first"), "primary must be")):
        with pytest.raises(ValueError, match=what):
            predict.Rotations(rest, fork, **kw)
    with pytest.raises(ValueError, match="parallel in the rest"):
        predict.Rotations(np.array([[0, 0, 0], [1, 0, 0], [-2, 0, 0], [0, 0, 1.0]]), fork)
    assert predict.Rotations(rest, fork, primary={0: 2}).secondary[0] == 1 and predict.Rotations(rest, fork, secondary={0: 1}).primary[0] == 2
    stub = types.SimpleNamespace(arch=types.SimpleNamespace(compiled_dims=True), device="cpu", has_strided_input=True)
    with pytest.raises(ValueError, match="rotations together with out_fps is not supported: a push then returns several rows per slot"):
        stream.StreamSession(stub, cfg, slots=2, mask_stride=4, lookahead=40, fps=25, out_fps=50, rotations=True)
    with pytest.raises(ValueError, match="Skeleton"):
        stream.StreamSession(stub, small, slots=2, mask_stride=4, rotations=True)
    with pytest.raises(TypeError, match="unexpected keyword argument 'rotation'"):
        stream.StreamSession(stub, cfg, slots=2, mask_stride=4, rotation=True)


def test_c_abi_declared_and_refusing():
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(util.ROOT + "/include/uu3d.h").read()
    assert "JOINT ROTATIONS" in header
    for s in ("uu3d_joint_rotations", "uu3d_joint_rotations_reset"):
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s) and s + "(" in header, s
    a, b = C.c_void_p(256), C.c_void_p(512)                           # (aligned addresses that are never dereferenced: the calls refuse first)
    OK, BAD, UNS = _capi.UU3D_OK, _capi.UU3D_ERR_INVALID_ARGUMENT, _capi.UU3D_ERR_UNSUPPORTED
    turn = lambda frames, J, depth=4, poses=a, local=b, glob=None: lib.uu3d_joint_rotations(poses, frames, J, a, depth, a, None, local, glob, None, None)
    assert turn(4, 65) == UNS and turn(0, 65) == UNS
    assert turn(0, 17) == OK                                          # nothing to do, nothing launched
    assert turn(-1, 17) == BAD and turn(4, 0) == BAD and turn(4, 17, depth=-1) == BAD and turn(4, 17, depth=64) == BAD
    assert turn(4, 17, poses=None) == BAD and turn(4, 17, local=None) == BAD and turn(4, 17, local=a) == BAD and turn(4, 17, glob=a) == BAD
    assert turn(4, 17, local=C.c_void_p(520)) == BAD and turn(4, 17, glob=C.c_void_p(520)) == BAD and turn((1 << 32) + 1, 17) == BAD
    reset = lambda slots, J, local=b: lib.uu3d_joint_rotations_reset(slots, J, local, None, None, None, None)
    assert reset(1, 65) == UNS and reset(0, 17) == BAD and reset(1, 0) == BAD and reset(1, 17, local=None) == BAD
    assert reset(1, 17, local=C.c_void_p(520)) == BAD


# ---- unchanged surface -----------------------------------------------------------------------------------------------------------------
def test_surface():
    from uplift_upsample_3dhpe_amd import options, predict, rotations, stream
    assert inspect.signature(predict.predict_tracks).parameters["rotations"].default is None
    assert inspect.signature(options.stage_options).parameters["rotations"].default is None
    assert inspect.signature(stream.StreamSession._init_plan).parameters["rotations"].default is None
    assert list(inspect.signature(options.stage_options).parameters)[-1] == "rotations"
    assert stream.LIVE_OPTIONS[-1] == "rotations" and stream.LIVE_OPTIONS[:6] == ("repair_joints", "keypoints", "camera", "min_root_joints", "smooth", "bones")
    for owner in (predict, stream):
        for n in ("Rotations", "check_rotations", "joint_rotations_host"):
            assert getattr(owner, n) is getattr(rotations, n)
    for n in ("REST_POSES", "joint_rotations", "forward_kinematics", "quat_to_matrix"):
        assert getattr(predict, n) is getattr(rotations, n)
    assert rotations.check_rotations(None, 17) is None and rotations.check_rotations(True, 17).skeleton is predict.SKELETONS["h36m17"]
    R = rotations.check_rotations(True, 17)
    assert R.primary[6] == 8 and R.secondary[6] == 3 and R.primary[7] == 9 and R.secondary[7] == 13 and R.depth == 5
    assert list(R.level) == [len(p) for p in R.skeleton.paths]
    # a session's plan without the keyword is the plan with None
    cfg = util.load_config("h36m_81")
    stub = types.SimpleNamespace(arch=types.SimpleNamespace(compiled_dims=True), device="cpu", has_strided_input=True)
    plans = []
    for kw in ({}, {"rotations": None}):
        s = object.__new__(stream.StreamSession)
        s._init_plan(stub, cfg, 3, (1920, 1080), 4, True, 5, True, True, None, 50, None, **kw)
        plans.append({k: v for k, v in vars(s).items() if k not in ("model", "_key")})
    assert plans[0] == plans[1] and plans[0]["rotations"] is None
    # the stage modules look neither at predict nor at stream
    package = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd")
    for name in ("rotations", "bvh"):
        for node in ast.walk(ast.parse(open(os.path.join(package, name + ".py")).read())):
            if isinstance(node, ast.ImportFrom):
                names = set((node.module or "").split(".")) | ({a.name for a in node.names} if node.level and not node.module else set())
            elif isinstance(node, ast.Import):
                names = {part for a in node.names for part in a.name.split(".")}
            else:
                continue
            assert not names & {"predict", "stream"}, (name, names)


# ---- BVH -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ZXY", "XYZ", "YZX", "ZYX"])
def test_bvh_round_trip(tmp_path, order):
    from uplift_upsample_3dhpe_amd import bvh, rotations
    R = _cases()["h36m17"]
    sk = R.skeleton
    rng = np.random.default_rng(9)
    G = 12
    X = rng.normal(size=(G, 17, 3)).astype(np.float32)
    local = rotations.joint_rotations_host(X, R)[0]
    i, j, k = ("XYZ".index(c) for c in order)                         # two frames at gimbal lock: the middle angle at +-90 degrees
    for g, middle in ((0, 90.0), (1, -90.0)):
        M = bvh.euler_to_matrix(np.array([25.0, middle, 0.0]), order)
        w = 0.5 * np.sqrt(1.0 + np.trace(M))
        local[g, 3] = [w, (M[2, 1] - M[1, 2]) / (4 * w), (M[0, 2] - M[2, 0]) / (4 * w), (M[1, 0] - M[0, 1]) / (4 * w)]
    L = rng.uniform(0.1, 0.6, 17)
    roots = rng.normal(size=(G, 3))
    path = bvh.write_bvh(str(tmp_path / "walk.bvh"), sk, R, L, local, roots, fps=25.0, order=order)
    back = bvh.read_bvh(path)
    assert back["text"].startswith("HIERARCHY") and back["order"] == order
    assert back["frames"] == G and abs(back["frame_time"] - 0.04) < 1e-9 and back["parents"] == list(sk.parents)
    assert back["names"] == [f"joint{j}" for j in range(17)]
    want = R.rest * np.where(np.arange(17) == sk.root, 0.0, L)[:, None] * 100.0
    assert np.abs(back["offsets"] - want).max() <= 0.5e-6            # (six decimals)
    assert sorted(back["end_sites"]) == [j for j in range(17) if R.primary[j] < 0]
    assert np.abs(back["translations"] - roots * 100.0).max() <= 0.5e-6
    # angles are printed with six decimals of a degree, ~1e-8 rad each
    assert np.abs(bvh.euler_to_matrix(back["angles"], order) - rotations.quat_to_matrix(local)).max() <= 1e-6
    # without roots the translation is zero
    still = bvh.read_bvh(bvh.write_bvh(str(tmp_path / "still.bvh"), sk, "h36m17", L, local[:2]))
    assert still["frames"] == 2 and not still["translations"].any() and still["order"] == "ZXY" and abs(still["frame_time"] - 0.02) < 1e-9
    with pytest.raises(ValueError, match="order"):
        bvh.write_bvh(str(tmp_path / "bad.bvh"), sk, R, L, local, order="XYX")
