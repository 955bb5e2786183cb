"""Golden vectors for interpol.grid_pull / grid_push / grid_count on 2-D grids at spline orders 0 to 3 and mixed orders
(all 7 boundary conditions), their first-order backward, the 2-D spline prefilter and three 2-D resize cases, from the
reference's vendored torch-interpol on the CPU (utils/interpol: iso0.py, iso1.py, nd.py, coeff.py, resize.py).  The
reference runs in float64 and the results are stored rounded to float32; next to every array `k` the scalar `k + ".err"`
holds max|ref32 - ref64| of the reference's own float32 run.

Run: python tests/golden/make_golden_grid2d.py -> interpol_grid2d.npz (inputs, prefilter, resize) and one
interpol_grid2d_<order tag>.npz per order, each below the 1 MiB a committed file may have.

Keys: <shape>/b<bound>_e<extrapolate>/<what>, shape A = image (2,3,7,6) against a (5,9) grid, T = the thin image
(1,2,1,5) against a (3,4) grid (the n == 1 special cases of the bounds, a cubic support wider than the axis).

The reference's all-nearest pull (iso0.pull2d) has no defined result when it masks (extrapolate 0 or 'hist'): it ends in
`out = mask * mask` where iso0.pull3d has `out = out * mask`, so it returns the mask for one channel and raises for more
("shape '[2, 3, 5, 9]' is invalid for input of size 90").  With extrapolation it takes every B and C.  The order-0 pull
arrays under a mask, forward and backward, therefore come from the reference's generic path (nd.pull with two order-0
splines), which the reference's own dispatch is pointed to for these calls; away from ties it picks the nodes of iso0.

No coordinate may sit closer than 1e-3 to a multiple of 0.5 or to a mask threshold: such coordinates are drawn again and
the script asserts that none is left.  The float32 and float64 runs then pick the same nodes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import  # noqa: E402

R = ref_import.setup()
import torch  # noqa: E402
import grid2d_refs as GR  # noqa: E402
from make_golden_spline_grid import backward_pair, put  # noqa: E402

ORDERS = {"o0": 0, "o1": 1, "o2": 2, "o3": 3, "o31": [3, 1], "o02": [0, 2]}
MARGIN = 1e-3


def masked_nearest_through_nd():
    """Points the reference's dispatch of an all-nearest 2-D pull that masks to nd.pull (see the module docstring)"""
    from utils.interpol import iso0, nd, pushpull
    own = iso0.pull2d

    def pull2d(inp, g, bound, extrapolate=1):
        if extrapolate == 1:
            return own(inp, g, bound, extrapolate)
        return nd.pull(inp, g, bound, pushpull.make_spline([0, 0]), extrapolate)

    iso0.pull2d = pull2d


def case(out, tag, order, vol, grid, src, interpol):
    ins = list(vol.shape[2:])
    combos = [(b, e) for b in range(7) for e in (0, 1)] + [(3, 2)]          # extrapolate=2 ('hist') once per order
    for bound, ext in combos:
        k = "%s/b%d_e%d/" % (tag, bound, ext)

        def pull(x, g, pf=False):
            return interpol.grid_pull(x, g, order, bound, ext, pf)

        def push(x, g):
            return interpol.grid_push(x, g, ins, order, bound, ext)

        put(out, k + "pull", lambda dt: pull(vol.to(dt), grid.to(dt)))
        put(out, k + "push", lambda dt: push(src.to(dt), grid.to(dt)))
        put(out, k + "count", lambda dt: interpol.grid_count(grid.to(dt), ins, order, bound, ext))
        if bound in (0, 3) and ext < 2:
            (a, ea), (b_, eb) = backward_pair(pull, vol, grid, torch.sin)
            out[k + "pull_dinput"], out[k + "pull_dinput.err"], out[k + "pull_dgrid"], out[k + "pull_dgrid.err"] = a, ea, b_, eb
            (a, ea), (b_, eb) = backward_pair(push, src, grid, torch.cos)
            out[k + "push_dinput"], out[k + "push_dinput.err"], out[k + "push_dgrid"], out[k + "push_dgrid.err"] = a, ea, b_, eb
            if order in (2, 3):
                put(out, k + "pull_pf", lambda dt: pull(vol.to(dt), grid.to(dt), True))
                (a, ea), _ = backward_pair(lambda x, g: pull(x, g, True), vol, grid, torch.sin)
                out[k + "pull_pf_dinput"], out[k + "pull_pf_dinput.err"] = a, ea


def draw_grid(g, batch, outs, ins, rng):
    grid = torch.rand((batch,) + outs + (2,), generator=g) * (torch.tensor(ins, dtype=torch.float32) + 5.0) - 2.5
    grid = GR.redraw_near_jumps(grid.numpy().copy(), ins, rng, MARGIN)     # spills 2.5 pixels over every edge
    assert not GR.near_jumps(grid, ins, MARGIN).any()
    return torch.from_numpy(grid)


def main():
    from utils import interpol
    masked_nearest_through_nd()
    g = torch.Generator().manual_seed(52)
    rng = np.random.default_rng(52)
    base = {}
    ins, outs = (7, 6), (5, 9)
    vol = torch.randn((2, 3) + ins, generator=g)
    grid = draw_grid(g, 2, outs, ins, rng)
    src = torch.randn((2, 3) + outs, generator=g)
    tins, touts = (1, 5), (3, 4)
    tvol = torch.randn((1, 2) + tins, generator=g)
    tgrid = draw_grid(g, 1, touts, tins, rng)
    tsrc = torch.randn((1, 2) + touts, generator=g)
    base.update({"A/vol": vol.numpy(), "A/grid": grid.numpy(), "A/src": src.numpy(),
                 "T/vol": tvol.numpy(), "T/grid": tgrid.numpy(), "T/src": tsrc.numpy()})
    # the weights backward_pair multiplies the outputs by (pull: sin, the grid's shape; push: cos, the image's), as this
    # machine's float32 sin / cos gave them: a test that restates the backward arrays reads them instead of recomputing
    for tag, v, s in (("A", vol, src), ("T", tvol, tsrc)):
        base[tag + "/wsin"] = torch.sin(torch.arange(s.numel(), dtype=torch.float32)).reshape(s.shape).numpy()
        base[tag + "/wcos"] = torch.cos(torch.arange(v.numel(), dtype=torch.float32)).reshape(v.shape).numpy()
    # the prefilter alone: orders 2 and 3 under the five bounds it has conditions for (three families)
    for tag, v in (("A", vol), ("T", tvol)):
        for order in (2, 3):
            for bound in (0, 1, 2, 3, 6):
                put(base, "%s/coeff/o%d_b%d" % (tag, order, bound),
                    lambda dt: interpol.spline_coeff_nd(v.to(dt), order, bound, 2))
    put(base, "resize/o3_dct2", lambda dt: interpol.resize(vol.to(dt), shape=[10, 9], interpolation=3, bound="dct2",
                                                           prefilter=True))
    put(base, "resize/o1_edge", lambda dt: interpol.resize(vol.to(dt), factor=[2, 1.5], anchor="e", interpolation=1))
    put(base, "resize/o2_unbatched", lambda dt: interpol.resize(vol[0, 0].to(dt), shape=[9, 8], interpolation=2,
                                                                prefilter=True))
    np.savez_compressed(os.path.join(HERE, "interpol_grid2d.npz"), **base)
    sizes = {"interpol_grid2d.npz": os.path.getsize(os.path.join(HERE, "interpol_grid2d.npz"))}
    for otag, order in ORDERS.items():
        out = {}
        case(out, "A", order, vol, grid, src, interpol)
        case(out, "T", order, tvol, tgrid, tsrc, interpol)
        name = "interpol_grid2d_%s.npz" % otag
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
