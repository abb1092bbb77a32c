"""CPU: the ``Scene`` record of stream.py and the fold of the output-side stages over it, with stand-in buffers and stages: no device.
  1. ``Scene.as_result()`` gives the five tuples the docstrings of ``push`` name: plain, with camera, with rotations, with rotations and
     ``return_global``, camera with rotations -- the same buffer objects, the fresh flags viewed as bools
  2. ``scenes`` hands the raw scene through stand-in stages in the session's order and names what each leaves; the scene of an absent
     stage is the one before it; with ``rows`` the drained rows stand in the buffers' places"""
import pytest

torch = pytest.importorskip("torch")


class _Buffer(object):
    def __init__(self, name):
        self.name = name

    def view(self, dtype):
        return ("view", self.name, dtype)


class _Stage(object):
    """A stand-in stage: ``outputs`` puts its own stand-in buffers into the given fields of a scene; the fold sets ``read``."""

    def __init__(self, leaves, *fields):
        self.leaves, self.read = leaves, None
        self.outputs = tuple((f, ("rows", leaves, f, id(self)), (leaves, f, id(self))) for f in fields)

    def out(self, field):
        return (self.leaves, field, id(self))


def test_as_result_gives_the_five_tuples():
    from uplift_upsample_3dhpe_amd.stream import Scene
    p, f, r, st, q, g = (_Buffer(n) for n in ("poses", "fresh", "roots", "root_state", "local", "global"))
    fresh = ("view", "fresh", torch.bool)
    assert Scene(p, f, None, None, ()).as_result() == (p, fresh)
    assert Scene(p, f, r, st, ()).as_result() == (p, fresh, r, st)
    assert Scene(p, f, None, None, (q,)).as_result() == (p, fresh, q)
    assert Scene(p, f, None, None, (q, g)).as_result() == (p, fresh, q, g)
    assert Scene(p, f, r, st, (q,)).as_result() == (p, fresh, r, st, q)
    assert all(a is b for a, b in zip(Scene(p, f, r, st, (q, g)).as_result()[2:], (r, st, q, g)))


def test_the_fold_names_the_scenes_the_properties_read():
    from uplift_upsample_3dhpe_amd.stream import Scene, scenes
    raw = Scene(_Buffer("poses"), _Buffer("fresh"), None, None, ())
    order = ("fixed", "camera", "world", "shown", "shown", "shown")        # bones, root, world, pose filter, root filter, rotations
    named = scenes(raw, [(name, None) for name in order])
    assert set(named) == {"raw", "fixed", "camera", "world", "shown"} and all(scene is raw for scene in named.values())
    bones, root, world = _Stage("fixed", "poses"), _Stage("camera", "roots", "root_state"), _Stage("world", "poses", "roots")
    pose_filter, root_filter, rotations = _Stage("shown", "poses"), _Stage("shown", "roots"), _Stage("shown", "extras", "extras")
    # camera only: the raw pose is the camera-space pose and the one a push returns; the world scene is the camera scene
    named = scenes(raw, list(zip(order, (None, root, None, None, None, None))))
    assert named["fixed"] is raw and named["world"] is named["camera"] is named["shown"] and root.read is raw
    assert named["camera"].poses is raw.poses and named["camera"].roots == root.out("roots")
    # all six, in the session's order: every stage reads what the one before it left
    stages = [bones, root, world, pose_filter, root_filter, rotations]
    named = scenes(raw, list(zip(order, stages)))
    assert named["raw"] is raw and named["fixed"].poses == bones.out("poses") and named["fixed"].roots is None
    assert named["camera"].poses is named["fixed"].poses and named["camera"].root_state == root.out("root_state")
    assert named["world"].poses == world.out("poses") and named["world"].roots == world.out("roots")
    assert named["world"].root_state is named["camera"].root_state and named["world"].fresh is raw.fresh
    assert [st.read for st in stages[:4]] == [raw, named["fixed"], named["camera"], named["world"]]
    assert root_filter.read.poses == pose_filter.out("poses") and root_filter.read.roots is named["world"].roots
    assert named["shown"] == Scene(pose_filter.out("poses"), raw.fresh, root_filter.out("roots"), root.out("root_state"), (rotations.out("extras"),) * 2)
    assert rotations.read.poses is named["shown"].poses and rotations.read.extras == ()
    # the drained rows: the same order, the rows by name in the buffers' places, and no stage is told again what it reads
    rows = {row: ("drained",) + buffer for st in stages for _, row, buffer in st.outputs}
    drained = scenes(Scene("rows of poses", "rows of fresh", None, None, ()), list(zip(order, stages)), rows)
    assert [st.read for st in stages[:4]] == [raw, named["fixed"], named["camera"], named["world"]]
    assert drained["fixed"].poses == ("drained",) + bones.out("poses") and drained["world"].roots == ("drained",) + world.out("roots")
    assert drained["shown"] == Scene(("drained",) + pose_filter.out("poses"), "rows of fresh", ("drained",) + root_filter.out("roots"),
                                     ("drained",) + root.out("root_state"), (("drained",) + rotations.out("extras"),) * 2)
