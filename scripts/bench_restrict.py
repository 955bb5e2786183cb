"""Cold times of interpol.restrict at 160^3 with one channel (anchor 'e', orders 0, 1 and 3) to 80^3 and to 100^3 (a
non-integer factor), beside grid_push on the materialised restrict grid -- the route a caller had before restrict
existed -- and of the backward of the separable cubic resize 80^3 -> 160^3 beside grid_pull's backward on the same grid.
Cold: before every timed call a 1 GiB buffer is overwritten, so neither the L2 nor the 256 MB memory-side cache holds the
operands; one call between two HIP events, median of 9.

restrict is timed whole (three table builds, three passes, the division by fullscale, their allocations), then each
axis pass alone with its compulsory bytes (input read once, output written once) and their share of the 8 TB/s HBM peak,
and the build of the three transposed tables.

usage: python scripts/bench_restrict.py [output file]   (profiles/restrict.txt holds a run)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from brainfm_amd import interpol as IP

dev = torch.device("cuda:0")
N = 160
PEAK = 8e12
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)


def cold(fn, reps=9):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        flush.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(t):
    return "%10.1f %22s" % (t[0], "(%.1f .. %.1f)" % (t[1], t[2]))


g = torch.Generator(device="cpu").manual_seed(0)
vol = torch.randn((1, 1, N, N, N), generator=g).to(dev)
say("interpol.restrict, %d^3, one channel, anchor 'e', bound nearest, extrapolate; cold, median (min .. max) of 9, "
    "microseconds" % N)
for M in (80, 100):
    shape, lin, fullscale = IP._restrict_geometry(vol.shape, None, [M] * 3, "e")
    coords = [v.to(dev) for v in lin]
    grid = torch.stack(torch.meshgrid(*coords, indexing="ij"), dim=-1)[None].contiguous()
    bnd = IP._opts(1, "nearest", True)[0]
    say()
    say("%d^3 -> %d^3 (factor %.2f)" % (N, M, N / M))
    say("%-44s %10s %22s %10s %8s" % ("", "median us", "(min .. max)", "MB", "of peak"))
    for order in (0, 1, 3):
        o = IP._order_list(order)
        t_r = cold(lambda: IP.restrict(vol, shape=[M] * 3, anchor="e", interpolation=order))
        t_p = cold(lambda: IP._push_raw(vol, grid, shape, bnd, o, 1))          # includes zeroing the output
        say("order %d  %-35s %s" % (order, "restrict (tables + passes + divide)", fmt(t_r)))
        say("order %d  %-35s %s   restrict is %.2fx" % (order, "grid_push on the materialised grid", fmt(t_p),
                                                        t_p[0] / t_r[0]))
        iso0 = o == (0, 0, 0)
        t_t = cold(lambda: [IP._axis_table(coords[a], M, order, 1, 1, True, iso0) for a in range(3)])
        say("order %d  %-35s %s" % (order, "three transposed tables", fmt(t_t)))
        cur = vol.reshape(1, N, N, N)
        for axis in range(3):
            tab = IP._axis_table(coords[axis], M, order, 1, 1, True, iso0)
            t_a = cold(lambda: IP._axis_pass(cur, axis, tab))
            nxt = IP._axis_pass(cur, axis, tab)
            nbytes = 4 * (cur.numel() + nxt.numel())
            say("order %d  %-35s %s %10.1f %7.1f%%" % (order, "pass along %s %s -> %s" % ("xyz"[axis], tuple(cur.shape[1:]),
                                                                                  tuple(nxt.shape[1:])),
                                                       fmt(t_a), nbytes / 1e6, 100 * nbytes / (t_a[0] * 1e-6) / PEAK))
            cur = nxt

say()
say("backward of resize 80^3 -> %d^3, cubic, bound dct2, prefilter=True, one channel (the gradient arrives; forward "
    "not timed)" % N)
small = torch.randn((1, 1, 80, 80, 80), generator=g).to(dev)
w = torch.randn((1, 1, N, N, N), generator=g).to(dev)
lin = [torch.linspace(0, 79, N, dtype=torch.float32) for _ in range(3)]
grid = torch.stack(torch.meshgrid(*lin, indexing="ij"), dim=-1)[None].contiguous().to(dev)
x1 = small.clone().requires_grad_(True)
y1 = IP.resize(x1, shape=[N] * 3, interpolation=3, bound="dct2", prefilter=True)
x2 = small.clone().requires_grad_(True)
y2 = IP.grid_pull(x2, grid, 3, "dct2", True, prefilter=True)


def back(y, x):
    x.grad = None
    y.backward(w, retain_graph=True)


t_s = cold(lambda: back(y1, x1))
t_g = cold(lambda: back(y2, x2))
say("%-44s %s" % ("resize (separable: three transposed passes)", fmt(t_s)))
say("%-44s %s   separable is %.2fx" % ("grid_pull(prefilter=True) on the same grid", fmt(t_g), t_g[0] / t_s[0]))
say("max|difference of the two gradients| %.2e (max|gradient| %.2e)" %
    (float((x1.grad - x2.grad).abs().max()), float(x2.grad.abs().max())))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
