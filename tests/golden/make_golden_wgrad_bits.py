"""The bits of bfm_conv3x3x3_wgrad_ex's dW on the cases of tests/wgrad_cases.py, on every route a process can be put on
(default, BFM_WGRAD_WS=0, BFM_WGRAD_UPFOLD=0), so that a change of the host code that picks and launches the kernels can be
held to equality.  The float64 tests of tests/test_gpu_backward.py allow 2e-5 and would not see a changed last bit.

Run on an MI355X with the library built: python tests/golden/make_golden_wgrad_bits.py [out] -> wgrad_bits.json, {run: {case:
{"sha", "head"}}}.  The children are those of tests/test_gpu_wgrad_bits.py (tests/wgrad_bits_worker.py).  The file in the tree
was made from the library as it stood before the route plan (bfm_conv3x3x3_wgrad_plan) existed, so it holds no routes.
Regenerate it only from a commit whose kernels are known good."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import wgrad_bits_worker as WW  # noqa: E402
import wgrad_cases as WC  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "wgrad_bits.json")
    d = {}
    for run in WC.BITS_RUNS:
        d[run] = {k: {"sha": v["sha"], "head": v["head"]} for k, v in WW.spawn(run).items()}
        print("%s: %d cases" % (run, len(d[run])), flush=True)
    with open(out_path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d bytes" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main()
