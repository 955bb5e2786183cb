"""Golden vectors for interpol.grid_pull / grid_push / grid_count / grid_grad at spline orders 0, 2, 3 and mixed orders
(3-D, all 7 boundary conditions), their first-order backward, the spline prefilter and two resize cases, from the
reference's vendored torch-interpol on the CPU (utils/interpol: nd.py, iso0.py, coeff.py, resize.py).  The reference runs
in float64 and the results are stored rounded to float32; next to every array `k` the scalar `k + ".err"` holds
max|ref32 - ref64| of the reference's own float32 run, the yardstick for what a float32 implementation can be held to.

Run: python tests/golden/make_golden_spline_grid.py -> interpol_spline_grid.npz (inputs, prefilter, resize) and one
interpol_spline_grid_<order tag>.npz per order, each below the 1 MiB a committed file may have.

Keys: <shape>/b<bound>_e<extrapolate>/<what>, shape A = volume (2,3,7,6,8) against a (5,9,6) grid, T = the thin volume
(1,2,1,2,5) against a (3,4,5) grid (the n == 1 special cases of the bounds, a cubic support wider than the axis).

Nearest-neighbour values, the derivative on a linear axis and the inbounds mask jump, so no coordinate may sit closer
than 1e-3 to a multiple of 0.5 or to a mask threshold: such coordinates are drawn again and the script asserts that none
is left.  The float32 and float64 runs then pick the same nodes."""
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

ORDERS = {"o0": 0, "o2": 2, "o3": 3, "o312": [3, 1, 2], "o023": [0, 2, 3]}
MARGIN = 1e-3


def both(fn):
    """fn(dtype) -> tensor; returns (float64 result rounded to float32, max|ref32 - ref64|)"""
    r64 = fn(torch.float64).detach()
    r32 = fn(torch.float32).detach()
    assert r32.dtype == torch.float32 and r64.dtype == torch.float64
    return r64.to(torch.float32).numpy(), np.float64((r32.double() - r64).abs().max().item())


def put(out, key, fn):
    out[key], out[key + ".err"] = both(fn)


def backward_pair(fwd, a, b, wfun):
    """d(sum(fwd(a, b) * w))/da and /db for the float64 and float32 runs"""
    res = {}
    for dt in (torch.float64, torch.float32):
        x = a.to(dt).clone().requires_grad_(True)
        g = b.to(dt).clone().requires_grad_(True)
        y = fwd(x, g)
        w = wfun(torch.arange(y.numel(), dtype=torch.float32)).reshape(y.shape).to(dt)
        (y * w).sum().backward()
        res[dt] = (x.grad.detach(), g.grad.detach())
    outs = []
    for i in range(2):
        r64, r32 = res[torch.float64][i], res[torch.float32][i]
        outs.append((r64.to(torch.float32).numpy(), np.float64((r32.double() - r64).abs().max().item())))
    return outs


def case(out, tag, order, vol, grid, src, interpol):
    ins = list(vol.shape[2:])
    combos = [(b, e) for b in range(7) for e in (0, 1)] + [(3, 2)]          # extrapolate=2 ('hist') once per order
    for bound, ext in combos:
        k = "%s/b%d_e%d/" % (tag, bound, ext)
        put(out, k + "pull", lambda dt: interpol.grid_pull(vol.to(dt), grid.to(dt), order, bound, ext))
        put(out, k + "push", lambda dt: interpol.grid_push(src.to(dt), grid.to(dt), ins, order, bound, ext))
        put(out, k + "grad", lambda dt: interpol.grid_grad(vol.to(dt), grid.to(dt), order, bound, ext))
        if bound in (0, 3) and ext < 2:
            put(out, k + "count", lambda dt: interpol.grid_count(grid.to(dt), ins, order, bound, ext))
            (a, ea), (b_, eb) = backward_pair(lambda x, g: interpol.grid_pull(x, g, order, bound, ext), vol, grid, torch.sin)
            out[k + "pull_dinput"], out[k + "pull_dinput.err"], out[k + "pull_dgrid"], out[k + "pull_dgrid.err"] = a, ea, b_, eb
            (a, ea), (b_, eb) = backward_pair(lambda x, g: interpol.grid_push(x, g, ins, order, bound, ext), src, grid,
                                              torch.cos)
            out[k + "push_dinput"], out[k + "push_dinput.err"], out[k + "push_dgrid"], out[k + "push_dgrid.err"] = a, ea, b_, eb
            if order in (2, 3):
                put(out, k + "pull_pf", lambda dt: interpol.grid_pull(vol.to(dt), grid.to(dt), order, bound, ext, True))
                (a, ea), _ = backward_pair(lambda x, g: interpol.grid_pull(x, g, order, bound, ext, True), vol, grid,
                                           torch.sin)
                out[k + "pull_pf_dinput"], out[k + "pull_pf_dinput.err"] = a, ea


def draw_grid(g, batch, outs, ins, rng):
    grid = torch.rand((batch,) + outs + (3,), generator=g) * (torch.tensor(ins, dtype=torch.float32) + 5.0) - 2.5
    grid = SR.redraw_near_jumps(grid.numpy().copy(), ins, rng, MARGIN)     # spills 2.5 voxels over every face
    assert not SR.near_jumps(grid, ins, MARGIN).any()
    return torch.from_numpy(grid)


def main():
    from utils import interpol
    g = torch.Generator().manual_seed(35)
    rng = np.random.default_rng(35)
    base = {}
    ins, outs = (7, 6, 8), (5, 9, 6)
    vol = torch.randn((2, 3) + ins, generator=g)
    grid = draw_grid(g, 2, outs, ins, rng)
    src = torch.randn((2, 3) + outs, generator=g)
    tins, touts = (1, 2, 5), (3, 4, 5)
    tvol = torch.randn((1, 2) + tins, generator=g)
    tgrid = draw_grid(g, 1, touts, tins, rng)
    tsrc = torch.randn((1, 2) + touts, generator=g)
    base.update({"A/vol": vol.numpy(), "A/grid": grid.numpy(), "A/src": src.numpy(),
                 "T/vol": tvol.numpy(), "T/grid": tgrid.numpy(), "T/src": tsrc.numpy()})
    # the prefilter alone: orders 2 and 3 under the five bounds it has conditions for
    for tag, v in (("A", vol), ("T", tvol)):
        for order in (2, 3):
            for bound in (0, 1, 2, 3, 6):
                put(base, "%s/coeff/o%d_b%d" % (tag, order, bound),
                    lambda dt: interpol.spline_coeff_nd(v.to(dt), order, bound, 3))
    # resize: order 2 with the edge anchor; order 3 with bound 'zero' and no extrapolation
    put(base, "resize/o2_edge", lambda dt: interpol.resize(vol.to(dt), shape=[10, 9, 11], anchor="e", interpolation=2,
                                                           prefilter=True))
    put(base, "resize/o3_zero_noext", lambda dt: interpol.resize(vol.to(dt), shape=[9, 8, 11], anchor="c", interpolation=3,
                                                                 prefilter=True, bound="zero", extrapolate=False))
    np.savez_compressed(os.path.join(HERE, "interpol_spline_grid.npz"), **base)
    sizes = {"interpol_spline_grid.npz": os.path.getsize(os.path.join(HERE, "interpol_spline_grid.npz"))}
    for otag, order in ORDERS.items():
        out = {}
        case(out, "A", order, vol, grid, src, interpol)
        case(out, "T", order, tvol, tgrid, tsrc, interpol)
        name = "interpol_spline_grid_%s.npz" % otag
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
