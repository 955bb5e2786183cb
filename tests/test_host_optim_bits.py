"""CPU checks of tests/golden/optim_bits.npz (the stored bits of the four optimiser steps, tests/test_gpu_optim_bits.py):
its size, and that every key tests/optim_bits_cases.py expects for each kind is there with its type and shape."""
import os

import numpy as np

from conftest import GOLDEN, load_npz
import optim_bits_cases as OB


def test_file_stays_small_and_holds_every_key_of_all_four_kinds():
    assert os.path.getsize(os.path.join(GOLDEN, "optim_bits.npz")) < 1 << 20
    d = load_npz("optim_bits.npz")
    want = OB.expected_keys()
    assert OB.KINDS == ("adamw", "adam", "sgd", "lars")
    assert set(d) == set(want) | {"apply/names"}
    n = len(d["apply/names"])
    assert n > 0
    for k, (dt, shape) in want.items():
        assert d[k].dtype == dt, k
        assert d[k].shape == tuple(n if s is None else s for s in shape), (k, d[k].shape)
    for kind in OB.KINDS:
        norms = d["apply/%s/norms" % kind]
        assert np.isfinite(norms).all() and (norms > 0).all() and not np.array_equal(norms[0], norms[1]), kind
        # a digest per tensor, none repeated: every parameter and buffer moved away from its start and from each other
        sha = np.concatenate([d["apply/%s/p_sha" % kind], d["apply/%s/s_sha" % kind].reshape(-1, 32)])
        assert len({bytes(r) for r in sha}) == len(sha), kind
    assert (d["abi/sumsq"] > 0).all() and np.isfinite(d["abi/lars_sums"]).all()
