"""A 64 -> 64 hidden task-head layer (task_f_maps [64, 64]; Conv3d(3, p=1) + bias + LeakyReLU(0.2), head.py:152-167) at
N^3 against the last decoder's second SingleConv of the same net -- the same shape with GroupNorm, on the path it has
always taken (GroupNorm statistics + the tuned conv variant) -- alternated in one process.  The hidden layer is two
launches: the convolution with the identity affine and slope 1, then bfm_head_bias_lrelu in place (bias, activation and the
next layer's bound); that pass is also timed alone.  Cold: the inputs rotate over SETS buffer sets (1 GB each at 160^3,
beyond the 256 MiB Infinity Cache).  Reports min / median / max over the repeats.

usage: python scripts/bench_head_layers.py [--size 160] [--reps 9] [--out profiles/head_layers.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from brainfm_amd import _lib as L
from brainfm_amd import test_utils as TU
from brainfm_amd.engine import HEAD_SLOPE

SETS = 3
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps, warm=2):
    for i in range(warm):
        fn(i)
    ts = []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(warm + i)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return min(ts), statistics.median(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=160)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_layers.py needs a HIP device")
    dev = torch.device("cuda:0")
    N = a.size
    dims = (N, N, N)
    ga, ta = TU.default_inference_args(f_maps=64, num_levels=2)
    ta.task_f_maps = [64, 64]
    torch.manual_seed(1)
    s = TU.InferenceSession(ga, ta, dev)
    eng = s.engine
    (hl,) = eng.head_layers([64, 64])
    ly = eng.dec[-1][1]                                    # 64 -> 64 at full resolution, with GroupNorm
    g = torch.Generator().manual_seed(N)
    xs = []
    for _ in range(SETS):
        x = torch.randn(dims + (64,), generator=g).to(dev)
        xs.append(x / x.norm(dim=-1, keepdim=True))       # unit vectors, as the first hidden layer reads them
    bound = eng.unit_bound()
    y = eng.head_conv(hl, xs[0], dims, bound)[0]
    nb = torch.empty(1, device=dev)

    def hidden(i):
        eng.head_conv(hl, xs[i % SETS], dims, bound)

    def parent(i):
        eng.single_conv(ly, xs[i % SETS], dims)

    def bias_pass(i):
        L.check(eng.lib.bfm_head_bias_lrelu(L.ptr(y), L.ptr(hl.bias), 64, N * N * N, HEAD_SLOPE, None, L.ptr(nb),
                                            L.stream_ptr()), "head_bias_lrelu")

    parent(0)                                              # tunes / looks up the variant, packs
    torch.cuda.synchronize()
    res = {}
    for _ in range(2):                                     # alternate, keep the better pass of each
        for name, fn in (("hidden layer", hidden), ("decoder SingleConv2", parent), ("bias + lrelu pass", bias_pass)):
            r = timed(fn, a.reps)
            if name not in res or r[1] < res[name][1]:
                res[name] = r
    gflop = 2.0 * 27 * 64 * 64 * N ** 3 / 1e9
    say("64 -> 64 at %d^3 (%.0f GFLOP; ms: min / median / max over %d, %d buffer sets)" % (N, gflop, a.reps, SETS))
    say("  hidden layer variant %d (4: F(4,3) conv_wino4d, 0: conv_mfma); decoder SingleConv2 variant %s"
        % (eng._head_cfg(hl, dims)[6], eng.conv_choices().get((64, 64, dims, False, False), "planner's")))
    for name, r in res.items():
        say("  %-22s %8.3f / %8.3f / %8.3f" % ((name,) + r))
    spread = max(res[k][2] - res[k][0] for k in ("hidden layer", "decoder SingleConv2"))
    diff = res["hidden layer"][1] - res["decoder SingleConv2"][1]
    say("  hidden - decoder = %+.3f ms (%.1f %% of the decoder layer), spread (max - min) %.3f ms; the separate pass costs "
        "%.3f ms = %.2f TB/s over %.2f GB read and written"
        % (diff, 100.0 * diff / res["decoder SingleConv2"][1], spread, res["bias + lrelu pass"][1],
           2.0 * 4 * 64 * N ** 3 / (res["bias + lrelu pass"][1] * 1e-3) / 1e12, 2.0 * 4 * 64 * N ** 3 / 1e9))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
