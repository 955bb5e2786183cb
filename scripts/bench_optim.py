"""One optimiser step of each kind over the parameter list of the shipped 64-wide 6-level net (264 M parameters, 1.06 GB;
heads as views into head_w / head_b as TrainStep holds them), one launch per phase, candidates alternated in one process:

  update    bfm_adamw_step_multi (the baseline), bfm_adam_step_multi, bfm_sgd_step_multi, bfm_lars_step_multi
  measure   bfm_grad_sumsq_multi (AdamW, Adam, SGD), bfm_lars_sums_multi (LARS)

all of optim.hip, on one descriptor table (bfm_optim_tensor_t).

Algorithmic bytes per parameter byte: Adam / AdamW update 7 (p, g, m, v read; p, m, v written), SGD / LARS update 5,
grad sumsq 1, the LARS measure 2.  Cold by size: every stream of a launch is 1.06 GB, four times the 256 MiB Infinity Cache,
and the launches rotate over SETS buffer sets besides.  Reports min / median / max of device-event times over the repeats
(each event pair spans the whole call, its fold launch included), bytes over the median as a share of the 8.0 TB/s HBM
peak, and whether the SGD and LARS updates, which move 5/7 of AdamW's bytes, are no slower than it beyond the spread.

usage: python scripts/bench_optim.py [--reps 9] [--sets 2] [--out profiles/optimizers.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from brainfm_amd import _lib as L
from brainfm_amd import train as TR
from oracle import unet_ref as O

HBM_PEAK = 8.0e12
CH = 65536
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def parameter_shapes(f_maps=64, levels=6):
    """(name, shape, reference ndim) in TrainStep.parameters() order; head rows as (task, rows)."""
    out = []
    for ly in O.layer_table(1, f_maps, levels):
        out.append((ly["name"] + ".groupnorm.weight", (ly["cin"],)))
        out.append((ly["name"] + ".groupnorm.bias", (ly["cin"],)))
        out.append((ly["name"] + ".conv.weight", (ly["cout"], ly["cin"], 3, 3, 3)))
    return out, list(O.default_out_channels().items()), f_maps


class BufferSet:
    """p, g, s0, s1 of every parameter: backbone tensors in 16-byte-aligned slots of one flat buffer per stream, the heads
    as row ranges of one (n_out, C) weight and one (n_out,) bias buffer (arbitrary float offsets)."""

    def __init__(self, dev, seed):
        shapes, heads, cf = parameter_shapes()
        sizes = [int(np.prod(s)) for _, s in shapes]
        offs = np.concatenate([[0], np.cumsum([(n + 3) // 4 * 4 for n in sizes])])
        n_out = sum(n for _, n in heads)
        g = torch.Generator(device=dev).manual_seed(seed)
        self.flat = {}
        for what, scale in (("p", 0.05), ("g", 1e-3), ("s0", 0.0), ("s1", 0.0)):
            t = torch.randn(int(offs[-1]) + n_out * cf + n_out + 8, generator=g, device=dev)
            self.flat[what] = t.mul_(scale)
        self.views = []                                        # (name, ref ndim, {stream: view})
        for (name, shape), o, n in zip(shapes, offs[:-1], sizes):
            self.views.append((name, len(shape), {k: v[int(o):int(o) + n] for k, v in self.flat.items()}))
        base, r0 = int(offs[-1]), 0
        for task, n in heads:
            w = {k: v[base + r0 * cf:base + (r0 + n) * cf] for k, v in self.flat.items()}
            b = {k: v[base + n_out * cf + 1 + r0:base + n_out * cf + 1 + r0 + n] for k, v in self.flat.items()}
            self.views.append(("head.final_conv_%s.weight" % task, 5, w))
            self.views.append(("head.final_conv_%s.bias" % task, 1, b))
            r0 += n
        self.n_params = sum(v["p"].numel() for _, _, v in self.views)
        cmap, first, firsts = [], 0, []
        for i, (_, _, v) in enumerate(self.views):
            nch = (v["p"].numel() + CH - 1) // CH
            firsts.append(first)
            cmap += [i] * nch
            first += nch
        self.nchunks = len(cmap)
        self.cmap = torch.tensor(cmap, dtype=torch.int32, device=dev)
        opt = np.zeros(len(self.views), dtype=TR._OPT_DESC)
        b1 = np.float32(1.0) - np.float32(0.9) ** np.float32(10)
        b2 = np.sqrt(np.float32(1.0) - np.float32(0.999) ** np.float32(10))
        for i, (_, nd, v) in enumerate(self.views):
            ptrs = tuple(v[k].data_ptr() for k in ("p", "g", "s0", "s1"))
            opt[i] = ptrs + (v["p"].numel(), 1.0, b1, b2, firsts[i], 1.0 if nd == 1 else 1e-3, 0.0 if nd == 1 else 0.04)
        self.opt = torch.from_numpy(opt.view(np.uint8).reshape(-1)).to(dev)
        self.sums = torch.zeros(3 * len(self.views), dtype=torch.float64, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws = torch.empty(3 * self.nchunks, dtype=torch.float64, device=dev)


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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 7:
        raise SystemExit("at least 7 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py needs a HIP device")
    dev = torch.device("cuda:0")
    lib = L.load()
    sets = [BufferSet(dev, 7 + k) for k in range(max(1, a.sets))]
    nbytes = 4.0 * sets[0].n_params
    lr, wd, mom = 1e-4, 0.04, 0.9

    def call(fn_name, *tail, measure=False):
        fn = getattr(lib, fn_name)

        def run(i):
            s = sets[i % len(sets)]
            args = (L.ptr(s.opt), len(s.views), L.ptr(s.cmap), s.nchunks, CH)
            if measure:
                args += (L.ptr(s.sums), L.ptr(s.flag), L.ptr(s.ws), s.ws.numel() * 8)
            L.check(fn(*args, *tail, L.stream_ptr()), fn_name)
        return run

    cands = [
        ("adamw update (baseline)", 7, call("bfm_adamw_step_multi", lr, 0.9, 0.999, 1e-8, wd)),
        ("adam update", 7, call("bfm_adam_step_multi", lr, 0.9, 0.999, 1e-8, wd)),
        ("sgd update", 5, call("bfm_sgd_step_multi", lr, mom, wd)),
        ("lars update", 5, call("bfm_lars_step_multi", lr, mom)),
        ("grad sumsq (measure)", 1, call("bfm_grad_sumsq_multi", measure=True)),
        ("lars sums (measure)", 2, call("bfm_lars_sums_multi", measure=True)),
    ]
    res = {}
    for _ in range(2):                                     # alternate the kinds, keep the better pass of each
        for name, _, fn in cands:
            r = timed(fn, a.reps)
            if name not in res or r[1] < res[name][1]:
                res[name] = r
    assert all(int(s.flag.item()) == 0 for s in sets)
    say("%d tensors, %d parameters (%.3f GB), %d chunks of %d, %d buffer sets; ms: min / median / max over %d, better of two "
        "alternated passes" % (len(sets[0].views), sets[0].n_params, nbytes / 1e9, sets[0].nchunks, CH, len(sets), a.reps))
    for name, mult, _ in cands:
        mn, med, mx = res[name]
        bw = mult * nbytes / (med * 1e-3)
        say("  %-26s %7.3f / %7.3f / %7.3f   %d x %.2f GB = %5.2f GB algorithmic, %.2f TB/s = %2.0f %% of the 8.0 TB/s HBM peak"
            % (name, mn, med, mx, mult, nbytes / 1e9, mult * nbytes / 1e9, bw / 1e12, 100.0 * bw / HBM_PEAK))
    base = res["adamw update (baseline)"]
    for name in ("adam update", "sgd update", "lars update"):
        r = res[name]
        spread = max(r[2] - r[0], base[2] - base[0])
        diff = r[1] - base[1]
        verdict = "no slower than the AdamW update beyond the spread" if diff <= spread else "SLOWER than the AdamW update"
        say("  %-12s - adamw update = %+.3f ms (%.2f x its time), spread (max - min) %.3f ms: %s"
            % (name, diff, r[1] / base[1], spread, verdict))
    say("  a LARS step = lars sums + lars update = %.3f ms, an AdamW step = grad sumsq + adamw update = %.3f ms (medians)"
        % (res["lars sums (measure)"][1] + res["lars update"][1], res["grad sumsq (measure)"][1] + base[1]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
