"""The pooled scalar (brain-age) head alone at the shipped shape: 160^3, C = 64 (models.AgeHead; head.py:39-48,61-66).
Event-timed forward and forward + backward (loss_age included), cold (first call) and warm (mean of `reps`), with a
per-phase breakdown of each launch group.  usage: python scripts/bench_age_head.py [reps] [out]
Writes the table to `out` (default profiles/age_head.txt) and prints it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from brainfm_amd import _lib as L
from brainfm_amd import models as M

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "age_head.txt")
dev = torch.device("cuda:0")
PEAK_GBS = 8000.0
D = H = W = 160
CF = 64
N = M.age_flat_features((D, H, W))
g = torch.Generator().manual_seed(0)
shapes = {"pool_layers.1.main.weight": (16, CF, 3, 3, 3), "pool_layers.1.main.bias": (16,),
          "pool_layers.3.main.weight": (4, 16, 3, 3, 3), "pool_layers.3.main.bias": (4,),
          "final_linear1_age.weight": (160, N), "final_linear1_age.bias": (160,),
          "final_linear2_age.weight": (10, 160), "final_linear2_age.bias": (10,),
          "final_linear3_age.weight": (1, 10), "final_linear3_age.bias": (1,)}
prm = {k: (torch.randn(s, generator=g) * 0.05).to(dev) for k, s in shapes.items()}
head = M.AgeHead(prm, CF, N, dev)
feat = torch.nn.functional.normalize(torch.randn((D, H, W, CF), generator=g), dim=-1).to(dev)
grads = {k: torch.empty_like(v) for k, v in prm.items()}
dfeat = torch.zeros_like(feat)
loss = torch.zeros(1, dtype=torch.float64, device=dev)
lib = L.load()


def ev():
    return torch.cuda.Event(enable_timing=True)


def fwd():
    return head.forward(feat, (D, H, W))


def fwd_bwd():
    _, tape = head.forward(feat, (D, H, W))
    head.backward(tape, 57.0, 0.5, L.ptr(loss), grads, dfeat)


def timed(fn, n):
    e0, e1 = ev(), ev()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def maxpool_only():
    P = (D // 4, H // 4, W // 4)
    o = torch.empty(P + (CF,), device=dev)
    a = torch.empty(P + (CF,), dtype=torch.uint8, device=dev)
    return lambda: L.check(lib.bfm_maxpool4(L.ptr(feat), CF, D, H, W, L.ptr(o), L.ptr(a), L.stream_ptr()), "maxpool4")


def phases():
    """Forward and backward, an event around each launch group (one extra synchronisation-free pass)."""
    marks = []
    orig = L.check

    def check(rc, what):
        orig(rc, what)
        e = ev()
        e.record()
        marks.append((what, e))
    L.check = check
    try:
        e0 = ev()
        e0.record()
        marks.append(("start", e0))
        fwd_bwd()
    finally:
        L.check = orig
    marks[-1][1].synchronize()
    return [(w, marks[i - 1][1].elapsed_time(e)) for i, (w, e) in enumerate(marks) if i > 0]


torch.cuda.synchronize()
cold_f = timed(fwd, 1)
cold_fb = timed(fwd_bwd, 1)
mp = maxpool_only()
cold_mp = timed(mp, 1)
warm_mp = timed(mp, reps)
warm_f = timed(fwd, reps)
warm_fb = timed(fwd_bwd, reps)
ph = phases()
mp_bytes = D * H * W * CF * 4 + (D // 4) * (H // 4) * (W // 4) * CF * 5
lines = ["age head (pooled scalar head, models.AgeHead) at %d^3, C = %d, N = %d -- measured on one MI355X, HIP events" % (D, CF, N),
         "",
         "%-34s %10s %10s %10s" % ("", "cold ms", "warm ms", "target ms"),
         "%-34s %10.3f %10.3f %10s" % ("maxpool4 (feature, 1.05 GB read)", cold_mp, warm_mp, "<= 0.35"),
         "%-34s %10.3f %10.3f %10s" % ("forward (6 launches)", cold_f, warm_f, "<= 0.5"),
         "%-34s %10.3f %10.3f %10s" % ("forward + backward (14 launches)", cold_fb, warm_fb, "<= 1.5"),
         "",
         "maxpool4 warm: %.0f GB/s = %.1f %% of %.0f GB/s HBM peak (compulsory bytes: feature read, pooled + argmax written)"
         % (mp_bytes / warm_mp / 1e6, 100 * mp_bytes / warm_mp / 1e6 / PEAK_GBS, PEAK_GBS),
         "",
         "phases of one forward + backward (ms between consecutive launch groups, host-enqueue gaps included):"]
lines += ["  %-28s %8.3f" % (w, t) for w, t in ph]
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
