"""Golden vectors for interpol.restrict and for the gradient of the separable cubic interpol.resize, from the reference's
vendored torch-interpol on the CPU (utils/interpol/restrict.py, resize.py).  The reference runs in float64 and the
results are stored rounded to float32; next to every array `k` the scalar `k + ".err"` holds max|ref32 - ref64| of the
reference's own float32 run.

Run: python tests/golden/make_golden_restrict.py -> interpol_restrict.npz (inputs, the coordinate lists, fullscale, the
resize gradients), one interpol_restrict_<order tag>.npz per order, each below the 1 MiB a committed file may have, and
api_signatures_restrict.json (inspect.signature of the reference's restrict).

Keys of the per-order files: <geometry>/b<bound>_e<extrapolate>/<what>, what = fwd, sum (reduce_sum=True), pf
(prefilter=True), dimage (d sum(y * sin(arange)) / dimage, with y = restrict(reduce_sum=True) / fullscale: the
reference's own in-place division stops autograd).  Geometries (input (2,3,11,9,14); T: the thin input (1,2,1,2,5)):
see GEOMS.

Nearest-neighbour nodes and the inbounds mask jump, so no coordinate of an axis of order 0 may sit closer than 1e-3 to
a half-integer (the centre of an odd axis lands on an integer under the 'e' anchor, where nothing jumps), and none of a
call without extrapolation closer than that to a mask threshold -- in float32 or in float64; coordinates that both
precisions compute to the same exactly representable value (i / 2, say) are exempt: there the reference's tie rule
decides (iso0.py rounds to even when all three orders are 0, nd.py takes floor(g + 0.5) otherwise).  The
script asserts it for the coordinates the reference itself hands to grid_push."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import  # noqa: E402

R = ref_import.setup()
import torch  # noqa: E402
import restrict_refs as RR  # noqa: E402
from make_golden_spline_grid import put  # noqa: E402

ORDERS = {"o0": 0, "o1": 1, "o2": 2, "o3": 3, "o312": [3, 1, 2]}
GEOMS = {"c": dict(anchor="c", shape=[5, 4, 6]),
         "f": dict(anchor="f", factor=[2, 3, 2]),
         "l": dict(anchor="l", factor=2, shape=[5, 4, 7]),
         "e": dict(anchor="e", shape=[5, 4, 6]),
         "eu": dict(anchor="e", shape=[13, 9, 19]),                       # upsizing: some nodes receive nothing (14 -> 20
                                                                           # would put a coordinate on 14.5)
         "cef": dict(anchor=["c", "e", "f"], shape=[5, 4, 6], factor=[2, 2, 2]),
         "T": dict(anchor="e", shape=[1, 1, 3])}
ALL_BOUNDS = "e"                                                           # the geometry that runs all seven bounds
BOUNDS = (1, 3, 0, 6)                                                      # nearest, dct2, zero, dft
MARGIN = 1e-3


def ref_modules():
    import utils.interpol  # noqa: F401
    return sys.modules["utils.interpol.restrict"], sys.modules["utils.interpol.resize"]


def captured_coords(mod, fn, *args, **kwargs):
    """The per-axis coordinate lists of the grid the reference builds (it hands the grid to grid_push / grid_pull)."""
    seen = {}
    names = [n for n in ("grid_push", "grid_pull") if hasattr(mod, n)]
    saved = {n: getattr(mod, n) for n in names}

    def spy(name):
        def f(image, grid, *a, **k):
            seen["grid"] = grid.detach().clone()
            return saved[name](image, grid, *a, **k)
        return f

    for n in names:
        setattr(mod, n, spy(n))
    try:
        fn(*args, **kwargs)
    finally:
        for n in names:
            setattr(mod, n, saved[n])
    g = seen["grid"]
    return [g[:, 0, 0, 0], g[0, :, 0, 1], g[0, 0, :, 2]]


def check_margins(tag, c32, c64, shape, order, exts):
    orders = RR._three(order)
    for a in range(3):
        exact = c32[a].astype(np.float64) == c64[a]
        for ext in exts:
            for c in (c32[a], c64[a]):
                bad = RR.near_jumps(c, shape[a], orders[a], ext, MARGIN, exact)
                assert not bad.any(), (tag, a, order, ext, np.asarray(c)[bad])


def main():
    rmod, zmod = ref_modules()
    restrict, resize = rmod.restrict, zmod.resize
    g = torch.Generator().manual_seed(36)
    vol = torch.randn((2, 3, 11, 9, 14), generator=g)
    tvol = torch.randn((1, 2, 1, 2, 5), generator=g)
    base = {"vol": vol.numpy(), "T/vol": tvol.numpy()}
    geo = {}
    for tag, kw in GEOMS.items():
        x = tvol if tag == "T" else vol
        c32 = [c.numpy() for c in captured_coords(rmod, restrict, x, **kw)]
        c64 = [c.numpy() for c in captured_coords(rmod, restrict, x.double(), **kw)]
        y = restrict(x.double(), reduce_sum=True, **kw)
        shape = list(y.shape[-3:])
        fs = float((restrict(x.double(), reduce_sum=True, **kw) / restrict(x.double(), **kw)).flatten()[0])
        shape2, cref, fs2 = RR.geometry(x.shape, kw.get("factor"), kw.get("shape"), kw["anchor"])
        assert shape2 == shape and abs(fs2 - fs) <= 1e-12 * abs(fs), (tag, shape, shape2, fs, fs2)
        for a in range(3):
            assert np.abs(cref[a] - c64[a]).max() < 1e-12, (tag, a)
            base["%s/coord%d" % (tag, a)] = c32[a]
        base[tag + "/shape"] = np.asarray(shape, np.int64)
        base[tag + "/fullscale"] = np.float64(fs2)
        geo[tag] = (x, kw, c32, c64, shape)
        print("%-4s %-18s -> %-12s fullscale %.6g" % (tag, tuple(x.shape), shape, fs2))

    # the gradient of the separable cubic resize (and of the same call off the separable route's prefilter)
    for key, kw in (("resize/dct2_pf", dict(bound="dct2", prefilter=True)),
                    ("resize/nearest_nopf", dict(bound="nearest", prefilter=False))):
        res = {}
        for dt in (torch.float64, torch.float32):
            x = vol.to(dt).clone().requires_grad_(True)
            y = resize(x, shape=[10, 9, 11], anchor="e", interpolation=3, **kw)
            w = torch.sin(torch.arange(y.numel(), dtype=torch.float32)).reshape(y.shape).to(dt)
            (y * w).sum().backward()
            res[dt] = x.grad.detach()
        base[key + "/dimage"] = res[torch.float64].float().numpy()
        base[key + "/dimage.err"] = np.float64((res[torch.float32].double() - res[torch.float64]).abs().max().item())
    np.savez_compressed(os.path.join(HERE, "interpol_restrict.npz"), **base)
    sizes = {"interpol_restrict.npz": os.path.getsize(os.path.join(HERE, "interpol_restrict.npz"))}

    for otag, order in ORDERS.items():
        out = {}
        for tag, (x, kw, c32, c64, shape) in geo.items():
            bounds = range(7) if tag == ALL_BOUNDS else BOUNDS
            combos = [(b, 1) for b in bounds]
            if tag == "e":
                combos += [(3, 0), (3, 2)]                                  # extrapolate=False and 'hist' once per order
            check_margins(tag, c32, c64, shape, order, sorted({e for _, e in combos}))
            for bound, ext in combos:
                k = "%s/b%d_e%d/" % (tag, bound, ext)
                opt = dict(kw, interpolation=order, bound=bound, extrapolate=ext)
                put(out, k + "fwd", lambda dt: restrict(x.to(dt), **opt))
            k = "%s/b3_e1/" % tag
            opt = dict(kw, interpolation=order, bound=3, extrapolate=1)
            put(out, k + "sum", lambda dt: restrict(x.to(dt), reduce_sum=True, **opt))
            if tag == "e" and order in (2, 3):
                put(out, k + "pf", lambda dt: restrict(x.to(dt), prefilter=True, **opt))
            if tag in ("c", "e"):
                res = {}
                for dt in (torch.float64, torch.float32):
                    xx = x.to(dt).clone().requires_grad_(True)
                    # the reference divides in place on a view of a custom Function's output, which autograd refuses:
                    # the same function written out of place
                    y = restrict(xx, reduce_sum=True, **opt) / base[tag + "/fullscale"].item()
                    w = torch.sin(torch.arange(y.numel(), dtype=torch.float32)).reshape(y.shape).to(dt)
                    (y * w).sum().backward()
                    res[dt] = xx.grad.detach()
                out[k + "dimage"] = res[torch.float64].float().numpy()
                out[k + "dimage.err"] = np.float64((res[torch.float32].double() - res[torch.float64]).abs().max().item())
        name = "interpol_restrict_%s.npz" % otag
        np.savez_compressed(os.path.join(HERE, name), **out)
        sizes[name] = os.path.getsize(os.path.join(HERE, name))
        errs = [float(v) for kk, v in out.items() if kk.endswith(".err")]
        big = max(float(np.abs(v).max()) for kk, v in out.items() if not kk.endswith(".err"))
        print(name, len(out) // 2, "arrays, max|ref32 - ref64| up to %.2e, max|ref| %.1f" % (max(errs), big))
    for k, v in sizes.items():
        print("%-36s %8d bytes" % (k, v))
        assert v < 1 << 20, k
    # the signature of the reference's restrict, in the format of api_signatures.json
    import json
    from make_golden_signatures import describe
    table = {"utils.interpol.restrict:restrict": {"mirror": "brainfm_amd.interpol:restrict", "params": describe(restrict)}}
    with open(os.path.join(HERE, "api_signatures_restrict.json"), "w") as f:
        json.dump({"signatures": table, "allowed_extra": {}}, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
