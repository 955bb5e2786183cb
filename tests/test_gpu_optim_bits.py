"""The optimiser steps give the bits stored in tests/golden/optim_bits.npz (made by tests/golden/make_golden_optim_bits.py
from the library as it stood while AdamW had its own kernels and its own half of TrainStep, before it became the fourth
kind of optim.hip's one path).  torch.equal, digest equality and == on the float64 norms: no tolerance.  The cases and the
calls are those of tests/optim_bits_cases.py.  Needs an MI355X: run with `-m gpu`."""
import numpy as np
import pytest

from conftest import load_npz
import optim_bits_cases as OB

pytestmark = pytest.mark.gpu

_D = {}


def golden():
    if not _D:
        _D.update(load_npz("optim_bits.npz"))
    return _D


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):                    # sized for the report; any difference fails
        pytest.fail("%s: %d of %d elements differ" % (what, int((got != want).sum()), got.size))


@pytest.mark.parametrize("kind", OB.KINDS)
def test_c_abi_steps_keep_their_bits(kind):
    """Three steps through bfm_<kind>_step_multi on sizes 1 .. 2 chunks + 1 and the misaligned view: parameters and every
    state buffer after step 3, and the fp64 sums of the measuring launch of step 1 (bfm_grad_sumsq_multi, or
    bfm_lars_sums_multi for LARS)."""
    d = golden()
    got = OB.run_abi(kind)
    assert set(got) == {k for k in d if k.startswith("abi/%s/" % kind)} | {"abi/lars_sums" if kind == "lars" else "abi/sumsq"}
    for k, v in got.items():
        same(v, d[k], k)


@pytest.mark.parametrize("kind", OB.KINDS)
def test_train_step_apply_keeps_its_bits(kind):
    """TrainStep.apply twice on seeded gradients under a loss scale of 1024, some below and some above clip_max_norm: the
    returned norms as float64 and the digest of every parameter and state buffer."""
    d = golden()
    got, names = OB.run_apply(kind)
    assert names == d["apply/names"].tolist()
    for k, v in got.items():
        same(v, d[k], k)
