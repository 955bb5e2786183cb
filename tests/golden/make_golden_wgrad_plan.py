"""bfm_conv3x3x3_wgrad_workspace over the grid of tests/wgrad_cases.py (every Cin the grid's channel pairs add up to, every
Cout, every extent), so that the bound can be rewritten in the route plan's terms and held to the values it had when it was
derived by hand.  tests/test_host_wgrad_plan.py compares and checks every plan's exact total against it.

Needs the built library and no GPU (the function is host arithmetic): python tests/golden/make_golden_wgrad_plan.py [out]
[library] -> wgrad_plan.json, {"cin", "cout", "dims", "bytes": [cin][cout][dims]}.  The file in the tree was made from the
library as it stood before the route plan existed."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import wgrad_cases as WC  # noqa: E402


def grid_cins():
    return sorted({ca + cb for ca, cb in WC.GRID_CHANNELS})


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "wgrad_plan.json")
    lib = C.CDLL(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "brainfm_amd", "libbrainfm_hip.so"))
    fn = lib.bfm_conv3x3x3_wgrad_workspace
    fn.restype, fn.argtypes = C.c_size_t, [C.c_int] * 5
    d = {"cin": grid_cins(), "cout": list(WC.GRID_COUT), "dims": [list(v) for v in WC.GRID_DIMS]}
    d["bytes"] = [[[fn(cin, cout, *dims) for dims in WC.GRID_DIMS] for cout in WC.GRID_COUT] for cin in d["cin"]]
    with open(out_path, "w") as f:
        json.dump(d, f)
        f.write("\n")
    print("%s: %d values, %d bytes" % (out_path, len(d["cin"]) * len(d["cout"]) * len(d["dims"]), os.path.getsize(out_path)))


if __name__ == "__main__":
    main()
