"""The bits of the optimiser steps (AdamW, Adam, SGD, LARS) as the built library gives them, through the C ABI and through
TrainStep.apply, so that a refactor of the optimiser path can be held to torch.equal.  The other optimiser tests compare
with float64 at 2e-6 and would not see a changed last bit.

Run on an MI355X with the library built: python tests/golden/make_golden_optim_bits.py -> optim_bits.npz.
Regenerate it only from a commit whose kernels are known good; the cases and the layout are in tests/optim_bits_cases.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import optim_bits_cases as OB  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "optim_bits.npz")
    d = {}
    for kind in OB.KINDS:
        for k, v in OB.run_abi(kind).items():
            if k in d:                                   # abi/sumsq: one record, whichever kind measured
                assert np.array_equal(d[k], v), (kind, k)
            d[k] = v
        res, names = OB.run_apply(kind)
        d.update(res)
        assert d.setdefault("apply/names", np.array(names)).tolist() == names
    np.savez_compressed(out_path, **d)
    print("%s: %d keys, %d bytes" % (out_path, len(d), os.path.getsize(out_path)))
    for kind in OB.KINDS:
        n = d["apply/%s/norms" % kind]
        print("  %-6s apply norms %s  min %.3e  max %.3e" % (kind, n.shape, n.min(), n.max()))
    print("  abi/sumsq %s  abi/lars_sums %s" % (d["abi/sumsq"].shape, d["abi/lars_sums"].shape))


if __name__ == "__main__":
    main()
