"""Kernel-only times of the first layer of a conditioned network, 2 -> 32 at 160^3, cold: every launch of the replayed
hipGraph works on another of SETS buffer sets (> 1.2 GB in all, several times the 256 MB Infinity Cache), between two HIP
events.  Three kernels on the same tensors:

  stem_mc   bfm_conv3x3x3_stem_mc_ex, the matrix-core stem for 2..4 input channels
  direct    bfm_conv3x3x3_direct, what the layer ran before (and runs under BFM_STEM_MC=0)
  stem      bfm_conv3x3x3_stem_ex on one channel of the input: the Cin = 1 yardstick, floor = its 128 B/voxel output

usage: python scripts/bench_stem.py [--n 160] [--cout 32] [--cin 2]      (prints a table and one JSON line)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from brainfm_amd import _lib as L

HBM_PEAK = 8.0e12          # bytes/s, MI355X
SETS = 3


def timed(fns, rounds=2, replays=5):
    """us per launch of the launches in `fns` (one per buffer set), `rounds` times each inside one graph."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for _ in range(rounds):
            for fn in fns:
                fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / (rounds * len(fns) * replays) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=160)
    ap.add_argument("--cin", type=int, default=2)
    ap.add_argument("--cout", type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stem.py needs a HIP device")
    dev = torch.device("cuda:0")
    lib = L.load()
    N, cin, cout = a.n, a.cin, a.cout
    nv = N ** 3
    g = torch.Generator().manual_seed(0)
    xs = [torch.rand((N, N, N, cin), generator=g).to(dev) for _ in range(SETS)]
    x1 = [x[..., 0].contiguous() for x in xs]
    outs = [torch.empty((N, N, N, cout), dtype=torch.float32, device=dev) for _ in range(SETS)]
    assert SETS * nv * 4 * (cin + cout) > 1.2e9 or N < 160
    w = ((torch.rand((cout, cin, 3, 3, 3), generator=g) - 0.5) / (27.0 * cin) ** 0.5).to(dev)
    wp = torch.empty(27 * cin * cout, dtype=torch.float32, device=dev)
    wp1 = torch.empty(27 * cout, dtype=torch.float32, device=dev)
    st = L.stream_ptr()
    L.check(lib.bfm_pack_conv_weights_direct(L.ptr(w), cin, cout, L.ptr(wp), st), "pack")
    L.check(lib.bfm_pack_conv_weights_direct(L.ptr(w[:, :1].contiguous()), 1, cout, L.ptr(wp1), st), "pack")
    scale = torch.tensor([2.0, 1.7, 2.3, 1.9][:cin], device=dev)
    shift = torch.tensor([-1.0, -0.8, -1.1, -0.9][:cin], device=dev)
    bound = torch.tensor([1.3], device=dev)
    rows = torch.empty(lib.bfm_moment_rows_bytes(lib.bfm_conv3x3x3_stem_rows(N, N, N), cout), dtype=torch.uint8, device=dev)

    def stem_mc(i):
        return lambda: L.check(lib.bfm_conv3x3x3_stem_mc_ex(L.ptr(xs[i]), cin, N, N, N, L.ptr(scale), L.ptr(shift),
                                                            L.ptr(bound), L.ptr(wp), cout, 0.01, L.ptr(outs[i]),
                                                            L.ptr(rows), L.stream_ptr()), "stem_mc")

    def direct(i):
        return lambda: L.check(lib.bfm_conv3x3x3_direct(L.ptr(xs[i]), cin, None, 0, N, N, N, None, L.ptr(scale),
                                                        L.ptr(shift), L.ptr(wp), cout, 0.01, L.ptr(outs[i]),
                                                        L.stream_ptr()), "direct")

    def stem(i):
        return lambda: L.check(lib.bfm_conv3x3x3_stem_ex(L.ptr(x1[i]), N, N, N, L.ptr(scale), L.ptr(shift), L.ptr(bound),
                                                         L.ptr(wp1), cout, 0.01, L.ptr(outs[i]), L.ptr(rows),
                                                         L.stream_ptr()), "stem")

    # same results first: the new kernel against the exact-fp32 one on set 0
    direct(0)()
    ref = outs[0].clone()
    stem_mc(0)()
    torch.cuda.synchronize()
    err = float((outs[0] - ref).abs().max()) / float(ref.abs().max())
    res = {"shape": [N, N, N], "cin": cin, "cout": cout, "relerr_stem_mc_vs_direct": err}
    # alternate the kernels, two passes, keep the smaller time of each
    t = {}
    for _ in range(2):
        for name, mk in (("stem_mc", stem_mc), ("direct", direct), ("stem", stem)):
            us = timed([mk(i) for i in range(SETS)])
            t[name] = min(t.get(name, us), us)
    for name, c in (("stem_mc", cin), ("direct", cin), ("stem", 1)):
        nbytes = nv * 4.0 * (c + cout)
        res[name + "_us"] = round(t[name], 2)
        res[name + "_hbm_fraction"] = round(nbytes / (t[name] * 1e-6) / HBM_PEAK, 4)
        print("%-8s %d -> %d @ %d^3  %9.2f us   %6.3f TB/s   %.3f of 8 TB/s" %
              (name, c, cout, N, t[name], nbytes / t[name] / 1e6, nbytes / t[name] / 1e6 / 8))
    print("stem_mc against direct: max|a-b| / max|b| = %.2e" % err)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
