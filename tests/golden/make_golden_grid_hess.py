"""Golden vectors for interpol.grid_hess, grid_pushgrad and the backward of grid_grad at spline orders 0 to 3 and mixed
orders (3-D, all 7 boundary conditions), from the reference's vendored torch-interpol on the CPU (utils/interpol:
pushpull.py:176-233 and :303-325 over nd.py, iso1.py and iso0.py).  The reference runs in float64 and the results are
stored rounded to float32; next to every array `k` the scalar `k + ".err"` holds max|ref32 - ref64| of the reference's
own float32 run.

Run: python tests/golden/make_golden_grid_hess.py -> one interpol_grid_hess_<order tag>.npz per order, each below the
1 MiB a committed file may have.  vol, grid and src of the shapes A and T come from interpol_spline_grid.npz.

Keys: cot/<shape> the cotangent (B,C,*out,3) drawn here, the input of pushgrad; inner/grid the second grid (below);
<shape>/b<bound>_e<extrapolate>/<what> with <what> one of
  hess, pushgrad            the seven bounds at extrapolate 1; pushgrad also at extrapolate 0
  grad_dinput, grad_dgrid   bounds 0 and 3 at extrapolate 1: the backward of sum(grid_grad * sin(arange)); grad_dinput
                            also at extrapolate 0
  grad_pf_dinput            the same with prefilter=True (orders 2 and 3)
and for order 1, where the reference's hess works with a mask, all of them at extrapolate 0 and 2 as well.

The reference's nd.hess raises, or returns a wrongly shaped result, whenever a mask exists (extrapolate 0 or 2) unless
B = C = 1 (nd.py:456 unsqueezes the mask once too often).  inner/b<bound>_e<0|2>/hess is its result on vol[:1, :1] of
shape A at the grid `inner`, drawn in [-0.6, n - 0.4] per axis so that between 40 % and 90 % of its voxels are inside the
mask (the A grid leaves 89 % outside at extrapolate 0); this is stored for order 1 too."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import  # noqa: E402

R = ref_import.setup()
import torch  # noqa: E402
import spline_grid_refs as SR  # noqa: E402
from make_golden_spline_grid import backward_pair, put  # noqa: E402

ORDERS = {"o0": 0, "o1": 1, "o2": 2, "o3": 3, "o312": [3, 1, 2], "o023": [0, 2, 3]}
MARGIN = 1e-3


def three(v):
    v = list(v) if isinstance(v, (list, tuple)) else [v]
    return (v + [v[-1]] * 3)[:3]


def case(out, tag, otag, vol, grid, cot, interpol, PP):
    order = ORDERS[otag]
    o3 = three(order)
    ins = list(vol.shape[2:])
    exts = (1, 0, 2) if otag == "o1" else (1,)
    for bound in range(7):
        for ext in exts:
            k = "%s/b%d_e%d/" % (tag, bound, ext)
            put(out, k + "hess", lambda dt: PP.grid_hess(vol.to(dt), grid.to(dt), [bound] * 3, o3, ext))
            put(out, k + "pushgrad", lambda dt: PP.grid_pushgrad(cot.to(dt), grid.to(dt), ins, [bound] * 3, o3, ext))
            if bound in (0, 3):
                (a, ea), (b_, eb) = backward_pair(lambda x, g: interpol.grid_grad(x, g, order, bound, ext), vol, grid, torch.sin)
                out[k + "grad_dinput"], out[k + "grad_dinput.err"], out[k + "grad_dgrid"], out[k + "grad_dgrid.err"] = a, ea, b_, eb
                if order in (2, 3):
                    (a, ea), _ = backward_pair(lambda x, g: interpol.grid_grad(x, g, order, bound, ext, True), vol, grid,
                                               torch.sin)
                    out[k + "grad_pf_dinput"], out[k + "grad_pf_dinput.err"] = a, ea
        if otag != "o1":                                     # extrapolate 0: what does not go through nd.hess
            k = "%s/b%d_e0/" % (tag, bound)
            put(out, k + "pushgrad", lambda dt: PP.grid_pushgrad(cot.to(dt), grid.to(dt), ins, [bound] * 3, o3, 0))
            if bound in (0, 3):
                # d/dinput only: the grid is a constant here, so nd.hess is not reached
                res = {}
                for dt in (torch.float64, torch.float32):
                    x = vol.to(dt).clone().requires_grad_(True)
                    y = interpol.grid_grad(x, grid.to(dt), order, bound, 0)
                    w = torch.sin(torch.arange(y.numel(), dtype=torch.float32)).reshape(y.shape).to(dt)
                    (y * w).sum().backward()
                    res[dt] = x.grad.detach()
                out[k + "grad_dinput"] = res[torch.float64].to(torch.float32).numpy()
                out[k + "grad_dinput.err"] = np.float64((res[torch.float32].double() - res[torch.float64]).abs().max().item())


def main():
    from utils import interpol
    from utils.interpol import pushpull as PP
    base = dict(np.load(os.path.join(HERE, "interpol_spline_grid.npz")))
    g = torch.Generator().manual_seed(36)
    rng = np.random.default_rng(36)
    shapes = {}
    cots = {}
    for tag in ("A", "T"):
        vol, grid = torch.from_numpy(base[tag + "/vol"]), torch.from_numpy(base[tag + "/grid"])
        cots[tag] = torch.randn(tuple(vol.shape[:2]) + tuple(grid.shape[1:]), generator=g)
        shapes[tag] = (vol, grid)
    ins = tuple(shapes["A"][0].shape[2:])
    inner = torch.rand((1, 5, 9, 6, 3), generator=g) * torch.tensor(ins, dtype=torch.float32) + (-0.6)
    # redraw_near_jumps draws again over the A grid's wider range, so a few coordinates leave [-0.6, n - 0.4]
    inner = torch.from_numpy(SR.redraw_near_jumps(inner.numpy().copy(), ins, rng, MARGIN))
    assert not SR.near_jumps(inner.numpy(), ins, MARGIN).any()
    inside = float(SR._mask(inner.numpy().astype(np.float64).reshape(1, -1, 3), ins, 0).mean())
    print("inner grid: %.1f %% of the voxels inside the mask at extrapolate 0" % (100 * inside))
    assert 0.4 <= inside <= 0.9
    sizes = {}
    for otag, order in ORDERS.items():
        out = {"cot/A": cots["A"].numpy(), "cot/T": cots["T"].numpy(), "inner/grid": inner.numpy()}
        for tag in ("A", "T"):
            case(out, tag, otag, shapes[tag][0], shapes[tag][1], cots[tag], interpol, PP)
        v11 = shapes["A"][0][:1, :1]
        for bound in range(7):
            for ext in (0, 2):
                put(out, "inner/b%d_e%d/hess" % (bound, ext),
                    lambda dt: PP.grid_hess(v11.to(dt), inner.to(dt), [bound] * 3, three(order), ext))
                assert out["inner/b%d_e%d/hess" % (bound, ext)].shape == (1, 1, 5, 9, 6, 3, 3)
        name = "interpol_grid_hess_%s.npz" % otag
        np.savez_compressed(os.path.join(HERE, name), **out)
        sizes[name] = os.path.getsize(os.path.join(HERE, name))
        errs = [float(v) for k, v in out.items() if k.endswith(".err")]
        print(name, len(out), "arrays, max|ref32 - ref64| between %.2e and %.2e" % (min(errs), max(errs)))
    for k, v in sizes.items():
        print("%-36s %8d bytes" % (k, v))
        assert v < 1 << 20, k
    print("total %d bytes" % sum(sizes.values()))


if __name__ == "__main__":
    main()
