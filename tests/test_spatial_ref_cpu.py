"""CPU: the two float64 statements of the spatial stack in tests/spatial_util.py agree -- the plain-numpy restatement (spatial_ref64)
and the lines oracle/uplift_oracle.py's forward_torch runs for this stage, at torch.float64 (spatial_torch) -- at <= 1e-12 absolute
(max |S| runs to about 4), for h36m_351's dims and every generic configuration tests/test_spatial_ops_gpu.py uses, on that
file's inputs: uniform frames plus the edge frames.  The float32 oracle's own deviation from float64, which scales the GPU bounds, is
printed per case."""
import numpy as np
import pytest

from tests import spatial_util as SU

torch = pytest.importorskip("torch")

CASES = [("h36m_351", 1, 0.1), ("h36m_351", 2, 0.5)] + [(name, 11, 0.1) for name in sorted(SU.GENERIC)] + [("j13_heads3", 12, 0.5)]


@pytest.mark.parametrize("name,seed,perturb", CASES, ids=[f"{n}-s{s}-p{p}" for n, s, p in CASES])
def test_numpy_float64_matches_the_oracles_float64_path(name, seed, perturb):
    _, arch, w = SU.arch_and_weights(name, seed, perturb)
    J = arch.num_keypoints
    frames = np.concatenate([SU.make_frames(9, J, seed), SU.edge_frames(J, seed)])
    a = SU.spatial_ref64(w, frames, arch.num_heads)
    b = SU.spatial_torch(w, frames, arch.num_heads, torch.float64)
    assert a.shape == b.shape == (len(frames), J * arch.d_spatial) and a.dtype == b.dtype == np.float64
    err = float(np.abs(a - b).max())
    dev = SU.f32_deviation(w, frames, arch.num_heads, a)
    print(f"{name} seed {seed} perturb {perturb}: numpy vs torch float64 {err:.2e} (max|S| {np.abs(a).max():.2f}); float32 oracle vs float64 {dev:.2e}")
    assert np.isfinite(a).all() and err <= 1e-12
    assert 0.0 < dev <= 1e-4                                     # float32 does round, and by what a GPU bound can be built on


def test_frames_are_independent_and_the_edges_are_distinct():
    """A frame's S does not depend on its neighbours (the stage has no cross-frame term), and each edge frame is its own case."""
    _, arch, w = SU.arch_and_weights("h36m_351", 1, 0.1)
    frames = np.concatenate([SU.make_frames(4, 17, 3), SU.edge_frames(17)])
    whole = SU.spatial_ref64(w, frames, 8)
    for i in (0, 3, 5, 8):
        assert np.array_equal(whole[i], SU.spatial_ref64(w, frames[i:i + 1], 8)[0])
    assert len({whole[i].tobytes() for i in range(len(frames))}) == len(frames)
