"""The contrastive pre-training mode (train.ContrastiveStep) measured on one GPU:
  1. bfm_loss_contrastive alone at 128^3 and 160^3, C = 64, n_norm = 2, between HIP events.  Its four maps (2.1 GB at
     128^3, 4.2 GB at 160^3) are far larger than the 256 MiB Infinity Cache, so every launch is a cold one; rate over the
     algorithmic 4 * nvox * C * 4 bytes (two maps read, two gradients written) and its share of the 8 TB/s HBM peak;
  2. beside it the same loss and both gradients by torch on the same device from the reference's formula with autograd
     (criterion.py:96-109: the loop over the channels; F.normalize twice);
  3. one full ContrastiveStep iteration at 128^3 (f_maps 64, 6 levels), per phase, as scripts/bench_train.py.
usage: python scripts/bench_contrastive.py [reps=5] [out.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from brainfm_amd import _lib as L
from brainfm_amd import backward as BW
from brainfm_amd import test_utils as TU
from brainfm_amd import train as TR

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else None
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
lib = L.load()
TEMPS = (0.1, 0.1, 0.1)
C_FEAT = 64
HBM_PEAK = 8.0e12


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed_ms(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = ev(), ev()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def torch_formula(x, y):
    """Loss and both gradients as the reference evaluates them, on (1, C, N) maps."""
    p = x.detach().requires_grad_(True)
    q = y.detach().requires_grad_(True)
    a, b = F.normalize(F.normalize(p, dim=1), dim=1), F.normalize(F.normalize(q, dim=1), dim=1)
    num = torch.exp(a * b / TEMPS[0]).sum(1)
    den = torch.zeros_like(a[:, 0])
    for i in range(a.shape[1]):
        ai = a[:, i]
        den = den + torch.exp(ai ** 2 / TEMPS[1]) + torch.exp(((ai[:, None] * a).sum(1) - ai ** 2) / TEMPS[2])
    loss = (-torch.log(num / den)).mean()
    loss.backward()
    return loss.detach(), p.grad, q.grad


result = {"reps": reps, "temperatures": TEMPS, "kernel": []}
for n in (128, 160):
    nv = n ** 3
    g = torch.Generator(device=dev).manual_seed(n)
    x = torch.randn((nv, C_FEAT), generator=g, device=dev)
    y = x + 0.3 * torch.randn((nv, C_FEAT), generator=g, device=dev)
    dx, dy = torch.empty_like(x), torch.empty_like(y)
    val = torch.zeros(1, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.bfm_loss_contrastive_workspace(), dtype=torch.uint8, device=dev)

    def kern(n_norm=2):
        L.check(lib.bfm_loss_contrastive(L.ptr(x), L.ptr(y), C_FEAT, nv, n_norm, 1e-12, TEMPS[0], TEMPS[1], TEMPS[2], 1.0,
                                         L.ptr(dx), L.ptr(dy), None, None, L.ptr(val), L.ptr(ws), ws.numel(), L.stream_ptr()),
                "contrastive")

    ms = timed_ms(kern, reps)
    # what bounds it: the same traffic as a plain copy of the two maps, and the kernel without the normalisations' arithmetic
    ms_copy = timed_ms(lambda: (dx.copy_(x), dy.copy_(y)), reps)
    ms_n0 = timed_ms(lambda: kern(0), reps)
    kern()                                                       # dx, dy of n_norm = 2 again, for the comparison below
    nbytes = 4 * nv * C_FEAT * 4
    xt, yt = x.t().unsqueeze(0), y.t().unsqueeze(0)              # (1, C, N) views: the reference's layout
    ms_t = timed_ms(lambda: torch_formula(xt, yt), max(1, reps // 2))
    lt, gx, gy = torch_formula(xt, yt)
    err = max(float((dx - gx[0].t()).abs().max() / gx.abs().max()), float((dy - gy[0].t()).abs().max() / gy.abs().max()))
    row = {"size": n, "nvox": nv, "kernel_ms": ms, "bytes": nbytes, "TBps": nbytes / ms / 1e9,
           "fraction_of_hbm_peak": nbytes / (ms * 1e-3) / HBM_PEAK, "copy_two_maps_ms": ms_copy, "kernel_n_norm0_ms": ms_n0,
           "torch_autograd_ms": ms_t, "speedup": ms_t / ms,
           "loss": float(val.item()), "torch_loss": float(lt), "max_rel_grad_diff_vs_torch_fp32": err}
    result["kernel"].append(row)
    print("bfm_loss_contrastive %d^3 C=64 n_norm=2: %.3f ms, %.2f TB/s over %.2f GB = %.3f of the 8 TB/s HBM peak (copy of the two "
          "maps %.3f ms, n_norm=0 %.3f ms) | torch autograd of the reference formula %.1f ms (%.0fx) | loss %.6f vs torch %.6f, "
          "gradients differ by %.1e" % (n, ms, row["TBps"], nbytes / 1e9, row["fraction_of_hbm_peak"], ms_copy, ms_n0, ms_t,
                                        row["speedup"], row["loss"], row["torch_loss"], err))
    del x, y, dx, dy, xt, yt, gx, gy
    torch.cuda.empty_cache()

# ---- one iteration at 128^3
N = 128
dims = (N, N, N)
ga, ta = TU.default_inference_args(f_maps=64, num_levels=6, tasks=dict(contrastive=True))
torch.manual_seed(1)
s = TU.InferenceSession(ga, ta, dev, passes=3)
step = TR.ContrastiveStep(s.engine, {"loss_contrastive": 1.0}, TEMPS, lr=1e-4)
g = torch.Generator().manual_seed(0)
x0 = torch.rand((1, 1) + dims, generator=g)
xs = [x0.to(dev), (x0 + 0.05 * torch.rand((1, 1) + dims, generator=g)).clamp(0, 1).to(dev)]


def forward_only():
    for x in xs:
        BW.backbone_forward_train(s.engine, s.engine.to_cl(x), dims)


forward_only()                                   # tunes the conv variants, packs the weights
torch.cuda.synchronize()
phases = {}
for lanes in (1, 2):
    step.sample_lanes = lanes
    tf = tb = to = 0.0
    for r in range(reps + 1):
        e = [ev() for _ in range(4)]
        e[0].record()
        forward_only()
        e[1].record()
        loss_dict, total, grads = step.loss_and_grads(xs)
        e[2].record()
        ok, _ = step.apply(grads)
        e[3].record()
        torch.cuda.synchronize()
        if r == 0:
            continue                              # first pass allocates the optimiser state and the dgrad packs
        tf += e[0].elapsed_time(e[1])
        tb += e[1].elapsed_time(e[2])
        to += e[2].elapsed_time(e[3])
    tf, tb, to = tf / reps, tb / reps, to / reps
    phases[lanes] = {"two_forwards_ms": tf, "forwards_loss_backwards_ms": tb, "clip_adamw_repack_ms": to,
                     "iteration_ms": tb + to, "loss": loss_dict["loss_contrastive"], "stepped": bool(ok)}
    print("ContrastiveStep %d^3, %d lane(s): two forwards %.1f ms | two forwards + loss + two backwards %.1f ms (loss + "
          "backwards ~%.1f) | clip + AdamW + repack %.1f ms | iteration %.1f ms; loss %.4f stepped=%s; peak memory %.1f GB"
          % (N, lanes, tf, tb, tb - tf, to, tb + to, loss_dict["loss_contrastive"], ok, torch.cuda.max_memory_allocated() / 2 ** 30))
result["iteration_128"] = phases
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
