"""interpol.restrict and the gradient of the separable cubic interpol.resize on the device (brainfm_amd/csrc/restrict.hip)
against the reference's own results (tests/golden/interpol_restrict*.npz, float64 runs rounded to float32), against
grid_push on the materialised grid (the route a caller had before) and against the float64 restatement
(tests/restrict_refs.py) on a volume that takes several workgroups, a ragged tail and a z length that is no multiple of
the tile.

The bar is the one of test_gpu_spline_grid.py: max|hip - ref| <= 2e-5 * max(1, max|ref|).

Ties at order 0.  When all three orders are 0 the reference leaves nd.py for iso0.py, whose node is round(g): a
coordinate exactly halfway between two nodes goes to the even one.  restrict follows it (the fixture's 'f' / 'l' cases with
factor 2 put every second sample on such a tie); grid_push of this package takes floor(g + 0.5), the upper node, there.
The route-parity volume (1,2,37,41,67) -> [17,20,30] has two exact ties in float32, 9.5 on y (10 under both rules) and
14.5 on z (node 14 under the reference's rule, 15 under grid_push's).  At order 0 the two z planes 14 and 15 are therefore
held to the restatement, which carries the reference's rule (test_host_restrict.py holds it to the fixture), and every
other element to grid_push; the restatement test covers every element at every order as well."""
import numpy as np
import pytest
import torch

from conftest import load_npz
import restrict_refs as RR
from test_host_restrict import GEOMS, N_ARRAYS, ORDERS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CACHE = {}


def base():
    if "base" not in _CACHE:
        _CACHE["base"] = load_npz("interpol_restrict.npz")
    return _CACHE["base"]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sin_w(y):
    return torch.sin(torch.arange(y.numel(), dtype=torch.float32)).reshape(y.shape).to(y.device)


class Log:
    """worst max|hip - ref| per kind of array, with the stored max|ref32 - ref64| of the same array"""

    def __init__(self):
        self.worst = {}

    def close(self, got, ref, what, kind, stored=float("nan")):
        got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        err = float(np.abs(got.astype(np.float64) - ref).max())
        if err >= self.worst.get(kind, (-1.0, 0.0))[0]:
            self.worst[kind] = (err, float(stored))
        assert err <= 2e-5 * max(1.0, float(np.abs(ref).max())), (what, err)

    def show(self, title):
        for kind, (err, stored) in sorted(self.worst.items()):
            ref = "stored max|ref32 - ref64| %.2e" % stored if stored == stored else "no stored distance"
            print("%-14s %-16s max|hip - ref| %.2e   %s" % (title, kind, err, ref))


@pytest.mark.parametrize("otag", list(ORDERS))
def test_every_array_of_the_fixture(otag):
    """Six geometries and the thin volume: four bounds each (all seven, extrapolate=False and 'hist' for 'e'),
    reduce_sum=True, prefilter=True at orders 2 and 3, the backward of 'c' and 'e'."""
    from brainfm_amd import interpol as IP
    d = load_npz("interpol_restrict_%s.npz" % otag)
    order = ORDERS[otag]
    log, n = Log(), 0
    for k in d:
        if k.endswith(".err"):
            continue
        tag, combo, what = k.split("/")
        x = T(base()["T/vol"] if tag == "T" else base()["vol"])
        opt = dict(GEOMS[tag], interpolation=order, bound=int(combo[1]), extrapolate=int(combo[4]))
        if what == "dimage":
            x = x.clone().requires_grad_(True)
            y = IP.restrict(x, **opt)
            (y * sin_w(y)).sum().backward()
            got = x.grad
        else:
            got = IP.restrict(x, reduce_sum=what == "sum", prefilter=what == "pf", **opt)
            assert got.dtype == torch.float32
        log.close(got, d[k], k, what, d[k + ".err"])
        n += 1
    assert n == N_ARRAYS[otag]
    log.show(otag)


def big():
    """(1,2,37,41,67) -> [17,20,30] under the default anchor; restrict's own host coordinates, the materialised grid"""
    if "big" not in _CACHE:
        from brainfm_amd import interpol as IP
        rng = np.random.default_rng(11)
        x = rng.standard_normal((1, 2, 37, 41, 67)).astype(np.float32)
        shape, lin, fs = IP._restrict_geometry(x.shape, None, [17, 20, 30], "c")
        grid = torch.stack(torch.meshgrid(*lin, indexing="ij"), dim=-1)
        _CACHE["big"] = dict(x=x, shape=list(shape), lin=[v.numpy() for v in lin], fs=fs, grid=grid)
    return _CACHE["big"]


def big_restatement(order, bi, ext):
    key = ("bigref", str(order), bi, ext)
    if key not in _CACHE:
        b = big()
        _CACHE[key] = RR.restrict(b["x"], [c.astype(np.float64) for c in b["lin"]], b["shape"], b["fs"], order, bi, ext)
    return _CACHE[key]


ROUTE = [(o, bnd) for o in ("o0", "o3", "o312") for bnd in ("zero", "dct2", "dft")]


@pytest.mark.parametrize("otag,bound", ROUTE)
def test_route_parity_with_grid_push_on_the_materialised_grid(otag, bound):
    from brainfm_amd import interpol as IP
    b = big()
    order, bi = ORDERS[otag], IP._BOUND[bound]
    ext = 0 if bound == "zero" else 1
    x = T(b["x"])
    got = IP.restrict(x, shape=b["shape"], interpolation=order, bound=bound, extrapolate=ext)
    ref = (IP.grid_push(x, b["grid"].to(DEV), b["shape"], order, bound, ext) / b["fs"]).cpu().numpy().astype(np.float64)
    assert tuple(got.shape) == (1, 2, 17, 20, 30)
    log = Log()
    if order == 0:
        # the tie of the module docstring: the float32 coordinate 14.5 on z, and no other on which the two rules differ
        ties = [(a, float(c)) for a in range(3) for c in b["lin"][a]
                if c - np.floor(c) == 0.5 and np.rint(c) != np.floor(c + 0.5)]
        assert ties == [(2, 14.5)]
        g = got.cpu().numpy()
        rest = big_restatement(order, bi, ext)
        log.close(g[..., 14:16], rest[..., 14:16], "tie planes vs restatement", "tie planes")
        assert float(np.abs(g[..., 14:16] - ref[..., 14:16]).max()) > 1e-2        # the two rules do differ there
        keep = [z for z in range(30) if z not in (14, 15)]
        log.close(g[..., keep], ref[..., keep], "restrict vs grid_push", "vs grid_push")
    else:
        log.close(got, ref, "restrict vs grid_push", "vs grid_push")
    log.show("%s %s" % (otag, bound))


@pytest.mark.parametrize("otag,bound", ROUTE)
def test_several_workgroups_against_the_restatement(otag, bound):
    from brainfm_amd import interpol as IP
    b = big()
    order, bi = ORDERS[otag], IP._BOUND[bound]
    ext = 0 if bound == "zero" else 1
    got = IP.restrict(T(b["x"]), shape=b["shape"], interpolation=order, bound=bound, extrapolate=ext)
    log = Log()
    log.close(got, big_restatement(order, bi, ext), "restrict vs restatement", "restatement")
    log.show("%s %s" % (otag, bound))


def test_two_calls_are_bit_equal_and_input_forms():
    from brainfm_amd import interpol as IP
    b = big()
    x = T(b["x"])
    for order in (0, 3, [3, 1, 2]):
        a1 = IP.restrict(x, shape=b["shape"], interpolation=order, bound="dct2")
        a2 = IP.restrict(x, shape=b["shape"], interpolation=order, bound="dct2")
        assert torch.equal(a1, a2)
        v = x.clone().requires_grad_(True)
        IP.restrict(v, shape=b["shape"], interpolation=order, bound="dct2").sum().backward()
        g1 = v.grad.clone()
        v.grad = None
        IP.restrict(v, shape=b["shape"], interpolation=order, bound="dct2").sum().backward()
        assert torch.equal(g1, v.grad)
    # any leading dimensions, none at all, names for the orders, a non-contiguous and a float64 input
    full = IP.restrict(x, shape=b["shape"], interpolation=3)
    assert torch.equal(IP.restrict(x[0, 1], shape=b["shape"], interpolation="cubic"), full[0, 1])
    assert torch.equal(IP.restrict(x[None, None], shape=b["shape"], interpolation=[3, "cubic", "third"]), full[None, None])
    xt = x.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not xt.is_contiguous() and torch.equal(IP.restrict(xt, shape=b["shape"], interpolation=3), full)
    y64 = IP.restrict(x.double(), shape=b["shape"], interpolation=3)
    assert y64.dtype == torch.float32 and torch.equal(y64, full)


def _tables(coords, shape, orders, bounds, ext, transpose, ties_even=False):
    from brainfm_amd import interpol as IP
    return [IP._axis_table(coords[a], shape[a], orders[a], bounds[a], ext, transpose, ties_even) for a in range(3)]


@pytest.mark.parametrize("order", [0, 3])
def test_every_output_element_is_written_over_a_poisoned_buffer(order):
    """The upsizing geometry (nodes that receive nothing) through the raw exports, every output buffer full of NaN on
    entry: the result has none and equals restrict(reduce_sum=True), which allocates with torch.empty."""
    from brainfm_amd import interpol as IP, _lib as L
    lib = L.load()
    x = T(base()["vol"]).reshape(6, 11, 9, 14).contiguous()
    shape, lin, _ = IP._restrict_geometry(x.shape, None, [13, 9, 19], "e")
    coords = [v.to(DEV) for v in lin]
    tabs = _tables(coords, shape, (order,) * 3, (1, 1, 1), 1, True, order == 0)
    if order == 0:
        rp = [t[0].cpu().numpy() for t in tabs]
        assert any((np.diff(r) == 0).any() for r in rp)                          # empty rows
    cur, dims = x, list(x.shape)
    for axis in range(3):
        rowptr, col, val, rows = tabs[axis]
        nd = list(dims)
        nd[axis + 1] = rows
        out = torch.full(nd, float("nan"), device=DEV)
        rc = lib.bfm_spline_axis_pass(L.ptr(cur), dims[0], dims[1], dims[2], dims[3], axis, L.ptr(rowptr), L.ptr(col),
                                      L.ptr(val), rows, L.ptr(out), L.stream_ptr())
        assert rc == 0
        assert not bool(torch.isnan(out).any()), axis
        cur, dims = out, nd
    ref = IP.restrict(x, shape=[13, 9, 19], anchor="e", interpolation=order, reduce_sum=True)
    assert torch.equal(cur, ref)


@pytest.mark.parametrize("order", [0, 1, 3, [3, 1, 2]])
def test_adjoint_identity(order):
    """<restrict(x, reduce_sum=True), y> = <x, backward applied to y>, both sums on the host in float64, 1e-5 relative"""
    from brainfm_amd import interpol as IP
    b = big()
    rng = np.random.default_rng(5)
    x = T(b["x"]).requires_grad_(True)
    y = T(rng.standard_normal((1, 2, 17, 20, 30)).astype(np.float32))
    for bound, ext in (("dct2", 1), ("zero", 0), ("dst2", 1)):
        x.grad = None
        r = IP.restrict(x, shape=b["shape"], interpolation=order, bound=bound, extrapolate=ext, reduce_sum=True)
        r.backward(y)
        lhs = float((r.detach().cpu().double() * y.cpu().double()).sum())
        rhs = float((x.detach().cpu().double() * x.grad.cpu().double()).sum())
        print("order %s %s: <Rx,y> %.9g <x,R'y> %.9g" % (order, bound, lhs, rhs))
        assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (order, bound, lhs, rhs)


def test_resize_forward_keeps_its_bits_and_has_a_gradient():
    from brainfm_amd import interpol as IP
    x = T(base()["vol"])
    for kw in (dict(bound="dct2", prefilter=True), dict(bound="nearest", prefilter=False)):
        y0 = IP.resize(x, shape=[10, 9, 11], anchor="e", interpolation=3, **kw)
        v = x.clone().requires_grad_(True)
        y1 = IP.resize(v, shape=[10, 9, 11], anchor="e", interpolation=3, **kw)
        assert y1.grad_fn is not None and y0.grad_fn is None
        assert torch.equal(y0, y1.detach())
        with torch.no_grad():
            assert torch.equal(IP.resize(v, shape=[10, 9, 11], anchor="e", interpolation=3, **kw), y0)


def test_resize_backward_matches_the_fixture_and_grid_pull():
    from brainfm_amd import interpol as IP
    log = Log()
    for key, kw in (("resize/dct2_pf", dict(bound="dct2", prefilter=True)),
                    ("resize/nearest_nopf", dict(bound="nearest", prefilter=False))):
        v = T(base()["vol"]).requires_grad_(True)
        y = IP.resize(v, shape=[10, 9, 11], anchor="e", interpolation=3, **kw)
        (y * sin_w(y)).sum().backward()
        log.close(v.grad, base()[key + "/dimage"], key, key, base()[key + "/dimage.err"])
    # several workgroups: the same gradient through grid_pull(prefilter=True) on the materialised grid
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 2, 20, 18, 23)).astype(np.float32)
    shape = [37, 41, 30]
    lin = [torch.linspace(0, n - 1, s, dtype=torch.float32) for n, s in zip(x.shape[2:], shape)]
    grid = torch.stack(torch.meshgrid(*lin, indexing="ij"), dim=-1).to(DEV)
    w = T(rng.standard_normal((1, 2) + tuple(shape)).astype(np.float32))
    for bound in ("dct2", "nearest"):
        v = T(x).requires_grad_(True)
        y = IP.resize(v, shape=shape, interpolation=3, bound=bound, prefilter=True)
        y.backward(w)
        u = T(x).requires_grad_(True)
        yp = IP.grid_pull(u, grid, 3, bound, True, prefilter=True)
        log.close(y, yp.detach().cpu().numpy().astype(np.float64), "resize vs grid_pull " + bound, "forward")
        yp.backward(w)
        log.close(v.grad, u.grad.cpu().numpy().astype(np.float64), "resize grad vs grid_pull grad " + bound, "vs grid_pull")
    log.show("resize")


def test_long_lines_leave_the_tile_and_a_block_beyond_2_31_elements():
    """z lines longer than the LDS tile holds take the strided kernel; a block of more than 2^31 elements takes its 64-bit
    instantiation.  Both against torch on the device."""
    from brainfm_amd import interpol as IP
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn((2, 2, 3, 8200), device=DEV, generator=g)
    coord = (torch.arange(40, dtype=torch.float32) * 205.3 + 0.37).to(DEV)
    for transpose in (False, True):
        n = 8200 if not transpose else 50
        src = x if not transpose else x[..., :40].contiguous()
        tab = IP._axis_table(coord, n, 3, 3, 1, transpose)
        got = IP._axis_pass(src, 2, tab)
        dense = torch.zeros((tab[3], src.shape[-1]), dtype=torch.float64, device=DEV)
        rowptr = tab[0].cpu().numpy()
        rows = torch.from_numpy(np.repeat(np.arange(tab[3]), np.diff(rowptr))).to(DEV)
        nnz = int(rowptr[-1])
        dense.index_put_((rows, tab[1][:nnz].long()), tab[2][:nnz].double(), accumulate=True)
        ref = torch.einsum("rc,...c->...r", dense, src.double())
        assert float((got.double() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    ny, nz = (1 << 15) + 1, 1 << 16                           # 2^31 + 2^16 elements
    big_x = torch.randn((1, 1, ny, nz), device=DEV, generator=g)
    coord = torch.tensor([0.25, ny - 1.5], dtype=torch.float32, device=DEV)
    tab = IP._axis_table(coord, ny, 1, 1, 1, False)
    got = IP._axis_pass(big_x, 1, tab)
    ref = torch.stack([0.75 * big_x[0, 0, 0] + 0.25 * big_x[0, 0, 1], 0.5 * big_x[0, 0, ny - 2] + 0.5 * big_x[0, 0, ny - 1]])
    assert tuple(got.shape) == (1, 1, 2, nz)
    assert float((got[0, 0] - ref).abs().max()) <= 2e-6        # two products of values below 6: a few ulp of 4


def test_exports_refuse_bad_arguments_and_write_nothing():
    from brainfm_amd import _lib as L
    lib = L.load()
    E_ARG, E_SHAPE, E_WS = -1, -2, -3
    coord = torch.linspace(0, 4, 9, device=DEV)
    rowptr = torch.full((10,), 7, dtype=torch.int32, device=DEV)
    col = torch.full((36,), 7, dtype=torch.int32, device=DEV)
    val = torch.full((36,), 7.0, device=DEV)
    nb = lib.bfm_spline_axis_table_workspace(9, 5, 3)
    assert nb > 0 and lib.bfm_spline_axis_table_workspace(9, 5, 4) == 0 and lib.bfm_spline_axis_table_workspace(0, 5, 3) == 0
    ws = torch.full((nb,), 7, dtype=torch.uint8, device=DEV)

    def table(c=coord, m=9, n=5, order=3, bound=3, ext=1, ties=0, tr=1, rp=rowptr, cl=col, vl=val, w=ws, wb=nb):
        return lib.bfm_spline_axis_table(L.ptr(c), m, n, order, bound, ext, ties, tr, L.ptr(rp), L.ptr(cl), L.ptr(vl),
                                         L.ptr(w), wb, L.stream_ptr())

    assert table(c=None) == E_ARG and table(rp=None) == E_ARG and table(cl=None) == E_ARG and table(vl=None) == E_ARG
    assert table(m=0) == E_ARG and table(n=0) == E_ARG and table(order=4) == E_ARG and table(order=-1) == E_ARG
    assert table(bound=7) == E_ARG and table(bound=-1) == E_ARG and table(ext=3) == E_ARG and table(ties=2) == E_ARG
    assert table(tr=2) == E_ARG
    assert table(m=(1 << 24) + 1) == E_SHAPE and table(n=(1 << 24) + 1) == E_SHAPE
    assert table(w=None) == E_WS and table(wb=nb - 1) == E_WS
    assert table(tr=0, w=None, wb=0) == 0                      # the pull direction needs no workspace
    torch.cuda.synchronize()
    assert bool((col == 7).sum() == 0) and bool((ws == 7).all())     # only the accepted call wrote, and not the workspace
    col.fill_(7)
    val.fill_(7.0)
    rowptr.fill_(7)
    x = torch.randn(2, 4, 5, 6, device=DEV)
    out = torch.full((2, 9, 5, 6), 7.0, device=DEV)

    def run(i=x, lead=2, d=(4, 5, 6), axis=0, rp=rowptr, cl=col, vl=val, n_out=9, o=out):
        return lib.bfm_spline_axis_pass(L.ptr(i), lead, d[0], d[1], d[2], axis, L.ptr(rp), L.ptr(cl), L.ptr(vl), n_out,
                                        L.ptr(o), L.stream_ptr())

    assert run(i=None) == E_ARG and run(rp=None) == E_ARG and run(cl=None) == E_ARG and run(vl=None) == E_ARG
    assert run(o=None) == E_ARG and run(lead=0) == E_ARG and run(d=(4, 0, 6)) == E_ARG and run(axis=3) == E_ARG
    assert run(axis=-1) == E_ARG and run(n_out=0) == E_ARG
    assert run(lead=1 << 40, d=(1 << 20, 5, 6)) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((rowptr == 7).all()) and bool((col == 7).all())
