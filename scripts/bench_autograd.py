"""One forward + backward through the autograd bridge (brainfm_amd.autograd) against TrainStep.loss_and_grads' phases for
the same loss, on the shipped 64-wide 6-level net with the demo head set, one sample, in one process on one engine:

  bridge     outs = dm(samples); loss = (outs[0]['T1'] - target).abs().mean()  (torch);  loss.backward()
  TrainStep  _sample_forward | _sample_criterion | _sample_backward of TrainStep(loss_names=['T1'])

Both run the same convolution, GroupNorm, pooling and weight-gradient kernels (the training forward with its tape, then
backbone_backward).  What differs: the bridge's head outputs are channels-last and its cotangents come from torch (the
slice and view gradients of the head outputs, the repack to channels-last), its heads' backward is bfm_head_bwd rather than
the rows form, and it forms the gradient of the input (the first layer's GroupNorm backward result is kept).  No optimiser
step in either.

Cold by size: every phase streams several times the 256 MiB Infinity Cache.  Device-event times, min / median / max over
the repeats after two warm passes of each; the two are alternated.  Peak memory is torch.cuda.max_memory_allocated over one
pass of each kind, measured after the warm passes from the same resident state (weights, packed forms, workspaces).

usage: python scripts/bench_autograd.py [size] [--reps 7] [--out profiles/autograd_bridge.txt]"""
import argparse
import gc
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from brainfm_amd import autograd as AG
from brainfm_amd import test_utils as TU
from brainfm_amd import train as TR

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def ev():
    return torch.cuda.Event(enable_timing=True)


def fmt(ts):
    return "%8.2f / %8.2f / %8.2f" % (min(ts), statistics.median(ts), max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("size", nargs="?", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_autograd.py needs a HIP device")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n = a.size
    dims = (n, n, n)
    ga, ta = TU.default_inference_args(f_maps=64, num_levels=6)
    torch.manual_seed(1)                       # default nn init under seed 1, as bench.py
    s = TU.InferenceSession(ga, ta, dev, passes=3)
    model = s.model
    dm = AG.differentiable(model)
    eng = AG.sync_engine(model.backbone, model.head)
    tail = model.head.tail(eng)
    step = TR.TrainStep(eng, tail, ["T1"], {"loss_T1": 1.0}, torch.ones(max(tail.desc.n_seg, 1)), 1)
    g = torch.Generator().manual_seed(0)
    x = torch.rand((1, 1) + dims, generator=g).to(dev)
    t1 = torch.rand((1, 1) + dims, generator=g).to(dev)
    target = {"T1": t1}
    scale = step.scaler.scale

    def bridge(x_in):
        for p in model.parameters():
            p.grad = None
        e = [ev() for _ in range(4)]
        e[0].record()
        outs, _ = dm([{"input": x_in}])
        e[1].record()
        loss = (outs[0]["T1"] - t1).abs().mean()
        e[2].record()
        loss.backward()
        e[3].record()
        torch.cuda.synchronize()
        return e, float(loss.detach())

    def trainstep():
        e = [ev() for _ in range(4)]
        step._touched_heads = set()
        e[0].record()
        ctx = step._sample_forward(x)
        e[1].record()
        step._sample_criterion(ctx, target, {}, scale)
        e[2].record()
        grads, slots, vals = step._sample_backward(ctx, target, scale)
        e[3].record()
        torch.cuda.synchronize()
        total = sum(step._finish_losses([(slots, vals)], n ** 3).values())
        return e, float(total)

    kinds = [("bridge", lambda: bridge(x)), ("bridge + input gradient", lambda: bridge(x.clone().requires_grad_(True))),
             ("TrainStep", trainstep)]
    times = {k: {p: [] for p in ("forward", "loss", "backward", "total")} for k, _ in kinds}
    losses = {}
    for r in range(a.reps + 2):
        for k, fn in kinds:
            e, losses[k] = fn()
            if r < 2:
                continue
            for p, i in (("forward", 0), ("loss", 1), ("backward", 2)):
                times[k][p].append(e[i].elapsed_time(e[i + 1]))
            times[k]["total"].append(e[0].elapsed_time(e[3]))
    peaks = {}
    for k, fn in kinds:
        for p in model.parameters():
            p.grad = None
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        peaks[k] = (torch.cuda.max_memory_allocated(dev) / 2 ** 30, base / 2 ** 30)
    say("64-wide 6-level net, demo head set (%d head channels), one sample at %d^3, loss mean |T1 - target|; ms: min / median / "
        "max over %d passes after two warm ones, the kinds alternated" % (tail.n_out, n, a.reps))
    for k, _ in kinds:
        say("  %-24s loss %.6f, peak memory %.2f GiB (%.2f GiB resident before the pass)" % ((k, losses[k]) + peaks[k]))
        for p in ("forward", "loss", "backward", "total"):
            say("      %-10s %s" % (p, fmt(times[k][p])))
    med = {k: statistics.median(times[k]["total"]) for k, _ in kinds}
    say("  bridge / TrainStep (median totals): %.2f / %.2f ms = %.2f x; with the input gradient %.2f ms = %.2f x"
        % (med["bridge"], med["TrainStep"], med["bridge"] / med["TrainStep"], med["bridge + input gradient"],
           med["bridge + input gradient"] / med["TrainStep"]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
