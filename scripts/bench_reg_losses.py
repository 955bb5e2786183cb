"""The registration regularisers (csrc/reg_regularisers.hip): each loss, value + gradient in one launch pair, on a 3-channel
field at 160^3 and 128^3 in the rows layout of the training step, and one training iteration of the full-width net
(f_maps 64, 6 levels) on a 128^3 crop with losses.registration_smooth / registration_hessian off and on.  HIP events on
torch's stream; one JSON line.
usage: python scripts/bench_reg_losses.py [--reps 20] [--step-reps 3] [--no-step]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from brainfm_amd import _lib as L


def ev():
    return torch.cuda.Event(enable_timing=True)


def time_loss(lib, dev, N, which, reps):
    nvox = N ** 3
    g = torch.Generator().manual_seed(N)
    raw = (torch.randn((3, nvox), generator=g) * 0.1).to(dev)
    dRaw = torch.zeros_like(raw)
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.bfm_loss_reg_workspace(3, N, N, N), dtype=torch.uint8, device=dev)
    fn = lib.bfm_loss_reg_smooth if which == "smooth" else lib.bfm_loss_reg_hessian

    def once():
        L.check(fn(L.ptr(raw), 0, nvox, 1, 3, N, N, N, 1.0, L.ptr(dRaw), L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr()),
                which)
    for _ in range(3):
        once()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = ev(), ev()
        a.record()
        once()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    med = ts[len(ts) // 2]
    # algorithmic traffic: read u (12 B / voxel), read + write dRaw (24 B / voxel)
    return {"ms": med, "min_ms": ts[0], "GBps_algorithmic": 36.0 * nvox / (med * 1e-3) / 1e9}


def time_step(dev, N, on, reps):
    from brainfm_amd import test_utils as TU
    from brainfm_amd import train as TR
    ga, ta = TU.default_inference_args(f_maps=64, num_levels=6)
    torch.manual_seed(1)
    s = TU.InferenceSession(ga, ta, dev, passes=3)
    tail = s.model.head.tail(s.engine)
    names = ["T1", "T1_grad", "T2", "T2_grad", "FLAIR", "FLAIR_grad", "CT", "CT_grad", "seg_ce", "seg_dice", "distance",
             "bias_field_log", "registration", "registration_grad"]
    if on:
        names += ["registration_smooth", "registration_hessian"]
    names += ["SR", "SR_grad"]
    ns = tail.desc.n_seg
    step = TR.TrainStep(s.engine, tail, names, {"loss_" + n: 1.0 for n in names}, torch.full((ns,), 1.0 / ns), 4, lr=1e-4)
    g = torch.Generator().manual_seed(0)
    dims = (N, N, N)
    xs = [torch.rand((1, 1) + dims, generator=g).to(dev)]
    lab = torch.randint(0, ns, (1,) + dims, generator=g)
    target = {"segmentation": torch.nn.functional.one_hot(lab, ns).permute(0, 4, 1, 2, 3).float().contiguous().to(dev)}
    for k in ("T1", "T2", "FLAIR", "CT"):
        target[k] = torch.rand((1, 1) + dims, generator=g).to(dev)
    target["distance"] = torch.randn((1, 4) + dims, generator=g).to(dev)
    target["registration"] = torch.randn((1, 3) + dims, generator=g).to(dev)
    samples = [{"bias_field_log": torch.randn((1, 1) + dims, generator=g).to(dev) * 0.3,
                "high_res_residual": torch.randn((1, 1) + dims, generator=g).to(dev) * 0.2}]
    ts = []
    loss = None
    for r in range(reps + 1):
        a, b = ev(), ev()
        a.record()
        loss, total, stepped = step.step(xs, target, samples)
        b.record()
        torch.cuda.synchronize()
        if r:
            ts.append(a.elapsed_time(b))
    ts.sort()
    del s, step
    torch.cuda.empty_cache()
    return {"ms": ts[len(ts) // 2], "min_ms": ts[0], "losses": {k: float(v) for k, v in loss.items() if "registration" in k}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = L.load()
    res = {}
    for N in (160, 128):
        for which in ("smooth", "hessian"):
            res["%s_%d" % (which, N)] = time_loss(lib, dev, N, which, a.reps)
    if not a.no_step:
        res["step_128_off"] = time_step(dev, 128, False, a.step_reps)
        res["step_128_on"] = time_step(dev, 128, True, a.step_reps)
        res["step_delta_ms"] = res["step_128_on"]["ms"] - res["step_128_off"]["ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
