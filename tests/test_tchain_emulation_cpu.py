"""CPU evidence that the bounds of tests/test_tchain_ops_gpu.py discriminate.  tests/tchain_util.emulate restates the arithmetic of
tchain16_kernel (csrc/uu3d_tchain16.h) in numpy float32 -- operands split into f16 hi / lo planes, hi.hi + (hi.lo + lo.hi) / 2048 with float32
accumulators, LayerNorm's affine part and q's scale folded into weights and biases as uu3d_commit_weights folds them -- on the GPU test's own
weights and its 191 input rows.  Against the float64 restatement from the named weights, block by block as the GPU test holds the kernel:

  * the emulation stays within HALF of every bound;
  * the same emulation with ONE cross term left out of ONE stage exceeds the bound of the quantity that stage ends in.

Figures (max-abs error against float64 over the 191 rows; bound; then with token-hi x weight-lo / token-lo x weight-hi left out of the stage):
  x + projection          (2e-5)   4.75e-06    projection without a term   9.64e-04 / 9.13e-04
  x_out of an MLP form    (6e-5)   9.93e-06    projection                  1.08e-03 / 1.08e-03
                                               fc1                         6.73e-04 / 6.32e-04
                                               fc2                         6.14e-04 / 7.20e-04
  q | k | v               (2e-5)   3.24e-06    QKV                         9.55e-04 / 8.83e-04
  H planes                (2e-5)   3.20e-06    fc1                         9.63e-04 / 8.94e-04
(the x30 row carries the residual sums' error: a float32 near 100 has an ulp of 7.6e-6)"""
import functools

import numpy as np
import pytest

from tests import tchain_util as T


@functools.lru_cache(maxsize=None)
def _errors(planes_form, drop, term):
    w = T.weights(True)
    x, o_hi, o_lo = T.pool()
    p, p_next = (T.block(True, 0), None) if planes_form else (T.block(False, 0), T.block(False, 1))
    e = T.emulate(w, p, p_next, x, o_hi, o_lo, planes_form=planes_form, drop=drop, term=term)
    o_val = T.planes_value(o_hi, o_lo)
    err = {"x1": np.abs(e["x1"] - T.ref_proj(w, p, x, o_val)).max()}
    if planes_form:
        err["h"] = np.abs(e["h"] - T.ref_fc1(w, p, e["x1"])).max()                     # (from the x + projection the launch stored)
    else:
        err["x2"] = np.abs(e["x2"] - T.ref_mlp(w, p, T.ref_proj(w, p, x, o_val))).max()
        err["qkv"] = np.abs(e["qkv"] - T.ref_qkv(w, p_next, e["qkv_in"])).max()       # (from the residual tile the launch stored)
    return err


BOUND = {"x1": T.TOL, "h": T.TOL, "x2": T.TOL_X, "qkv": T.TOL}


@pytest.mark.parametrize("planes_form", [False, True])
def test_emulation_stays_within_half_of_every_bound(planes_form):
    err = _errors(planes_form, None, "hl")
    print({k: f"{v:.2e}" for k, v in err.items()})
    for k, v in err.items():
        assert v <= 0.5 * BOUND[k], (k, v)


@pytest.mark.parametrize("term", ["hl", "lh"])
@pytest.mark.parametrize("planes_form,stage,quantity", [(True, "proj", "x1"), (True, "fc1", "h"), (False, "proj", "x2"), (False, "fc1", "x2"),
                                                        (False, "fc2", "x2"), (False, "qkv", "qkv")])
def test_one_dropped_cross_term_exceeds_the_bound(planes_form, stage, quantity, term):
    err = _errors(planes_form, stage, term)
    print(stage, term, {k: f"{v:.2e}" for k, v in err.items()})
    assert err[quantity] > BOUND[quantity], (stage, term, err)
    clean = _errors(planes_form, None, "hl")
    for k in err:                                             # each block is held on its own: a stage behind a stored intermediate is not charged
        if k != quantity and not (stage == "proj" and k == "x1"):
            assert err[k] <= 0.5 * BOUND[k] or err[k] == clean[k], (stage, k, err[k])
