"""Cold kernel times of interpol grid_pull / grid_push on a 2-D grid (the D = 2 instantiations of spline_grid.hip)
beside the same call embedded in 3-D -- image (X, Y, 1), a third coordinate 0, orders (ox, oy, 0) -- on the D = 3
instantiations of the same kernels, at 2048 x 2048 with one channel, bound dct2, extrapolate on.  The protocol of bench_spline_grid.py: before every timed launch a 1 GiB
buffer is overwritten, one launch between two HIP events, median (min .. max) of 9.  Two grids: the identity plus a
smooth displacement (1.5 pixels times a sine of period 40 pixels) and the identity plus a uniform jitter of +-1.5 pixels.

pull and push are one launch each into an output allocated beforehand (push: zeroed before the flush); "fwd+bwd" is
grid_pull(...).sum().backward() with gradients to the image and to the grid (pull, push, the 2-D or 3-D gradient kernel and
the torch kernels of the product, the sums and the allocations), so it is a sequence, not one launch.  The embedded call
needs the grid as 12 bytes per pixel: that repack (cat with a zero plane, contiguous) is timed on its own and added in the
last column.

The last column of each row says whether the native kernel is slower than the embedded one by more than the run-to-run
spread (max - min of the 9, the larger of the two).

usage: python scripts/bench_grid2d.py [output file]   (profiles/grid2d.txt holds a run)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from brainfm_amd import interpol as IP

dev = torch.device("cuda:0")
N = 2048
npix = N * N
PEAK = 8e12                                              # bytes per second
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)


def cold(fn, before=None, reps=9):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        if before is not None:
            before()
        flush.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def embed_grid(grid):
    return torch.cat([grid, torch.zeros_like(grid[..., :1])], -1)[..., None, :].contiguous()


g = torch.Generator(device="cpu").manual_seed(0)
img = torch.randn((1, 1, N, N), generator=g).to(dev)
img3 = img[..., None].contiguous()
ident = torch.stack(torch.meshgrid(*[torch.arange(N, dtype=torch.float32)] * 2, indexing="ij"), dim=-1)
phase = (ident.sum(-1, keepdim=True) * (6.283185307 / 40.0)) + torch.tensor([0.0, 2.1])
grids = {"smooth": (ident + 1.5 * torch.sin(phase))[None].contiguous().to(dev),
         "jitter": (ident + (torch.rand((N, N, 2), generator=g) * 3.0 - 1.5))[None].contiguous().to(dev)}
bnd, ext = IP._opts(1, "dct2", True)[0], 1
ORDERS = (0, 1, 2, 3, [3, 1])
out2, out3 = torch.empty((1, 1, N, N), device=dev), torch.empty((1, 1, N, N, 1), device=dev)

say("interpol 2-D grid kernels, %d x %d, one channel, bound dct2, extrapolate; cold, median (min .. max) of 9, microseconds"
    % (N, N))
say("compulsory HBM bytes per pixel: 8 (grid) + 4 (image) + 4 (out) = 16 -> %.1f MB, %.1f us at the 8 TB/s peak; the embedded "
    "call reads a 12-byte grid" % (npix * 16 / 1e6, npix * 16 / PEAK * 1e6))
say("loads (push: taps tested) per pixel, native: order 0: 1, order 1: 4, order 2: 9, order 3 and [3,1]: 16; embedded: order 0 "
    "runs the 1-tap instantiation, every other order the one padded to 4 x 4 x 4 = 64")
say()
slower = []
for gname, grid in grids.items():
    grid3 = embed_grid(grid)
    rp, rlo, rhi = cold(lambda: embed_grid(grid))
    say("grid: identity + %s displacement; repack of the grid to 12 bytes per pixel: %.1f (%.1f .. %.1f)" % (gname, rp, rlo, rhi))
    say("%-22s %9s %20s %8s | %9s %20s %10s | %6s %s" % ("call", "native us", "(min .. max)", "% peak", "embedded",
                                                        "(min .. max)", "+ repack", "ratio", "verdict"))
    for what in ("pull", "push", "fwd+bwd"):
        for order in ORDERS:
            o2 = IP._order_list(order)
            o3 = (o2[0], o2[1], 0)
            if what == "pull":
                nat = cold(lambda: IP._export("grid_pull2d_spline", img, grid, (N, N), bnd, o2, ext, (), out2))
                emb = cold(lambda: IP._export("grid_pull3d_spline", img3, grid3, (N, N, 1), bnd, o3, ext, (), out3))
            elif what == "push":
                nat = cold(lambda: IP._export("grid_push2d_spline", img, grid, (N, N), bnd, o2, ext, (), out2),
                           before=lambda: out2.zero_())
                emb = cold(lambda: IP._export("grid_push3d_spline", img3, grid3, (N, N, 1), bnd, o3, ext, (), out3),
                           before=lambda: out3.zero_())
            else:
                def fb(x, gr, o):
                    x.grad = gr.grad = None
                    IP.grid_pull(x, gr, list(o), "dct2", True).sum().backward()

                x2, g2 = img.clone().requires_grad_(True), grid.clone().requires_grad_(True)
                x3, g3 = img3.clone().requires_grad_(True), grid3.clone().requires_grad_(True)
                nat = cold(lambda: fb(x2, g2, o2[:2]))
                emb = cold(lambda: fb(x3, g3, o3))
            spread = max(nat[2] - nat[1], emb[2] - emb[1])
            bad = nat[0] > emb[0] + spread
            if bad:
                slower.append("%s %s order %s" % (gname, what, order))
            say("%-22s %9.1f %20s %8s | %9.1f %20s %10.1f | %6.2f %s"
                % ("%s order %s" % (what, order), nat[0], "(%.1f .. %.1f)" % nat[1:],
                   "%.1f" % (npix * 16 / PEAK * 1e6 / nat[0] * 100) if what != "fwd+bwd" else "-", emb[0],
                   "(%.1f .. %.1f)" % emb[1:], emb[0] + rp, emb[0] / nat[0],
                   "SLOWER than embedded + spread %.1f" % spread if bad else "ok"))
    say()
say("native slower than the embedded call by more than the spread: %s" % (", ".join(slower) if slower else "none"))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
