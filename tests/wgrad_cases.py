"""The weight-gradient cases (bfm_conv3x3x3_wgrad_ex, brainfm_amd/csrc/backward.hip) that the tests share: shapes, inputs,
the float64 bound, and next to every case the route its launcher has to take, written by hand from the launcher's predicates.
tests/test_gpu_backward.py runs them against float64, tests/test_host_wgrad_plan.py checks the routes and the split without a
GPU, tests/wgrad_bits_worker.py runs them in child processes for tests/test_gpu_wgrad_bits.py and
tests/golden/make_golden_wgrad_bits.py.

A route, as a test names it: "ws" the wave-specialised kernel on a plain layer, "fold+ws" / "fold+f16" a folded join whose
skip channels run on the wave-specialised or on the f16 tiled kernel, "f16" the f16 tiled kernel on all channels, "fp32" the
fp32 tiled kernel, "cols" the fp32 column kernel.  ROUTES[case] holds the route at passes = 3 for allow = 0, 1, 2, 3 (bit 0:
wave-specialised kernel allowed, bit 1: fold allowed); at passes = 0 every case here that is wide enough for tiles is "fp32"."""
import ctypes as C

import torch

WGRAD_TOL = 2e-5                        # the bound of test_weight_gradient_of_a_decoder_join_vs_float64 (split-fp16 class)
NAN = float("nan")

PLAIN = [                               # Cin, Cout, dims, G
    (64, 64, (5, 7, 19), 8),            # H % 4 != 0, odd W past one tile
    (32, 128, (3, 4, 16), 4),           # exact tile
    (96, 192, (2, 5, 9), 8),            # W below a tile
    (256, 256, (4, 4, 4), 8),           # deep-level extents
    (128, 64, (2, 2, 2), 8),
    (64, 64, (1, 2, 3), 8),
    (1024, 1024, (2, 2, 2), 8),         # 512 / cols == 0: clamped to one split
    (48, 64, (3, 4, 5), 8),             # CA % 32 != 0: the fp32 column kernel
    (256, 256, (6, 9, 33), 8),          # uneven split: 54 tiles of 4 x 16 over 8 workgroups of 7, the last with 5
]
JOINS = [                               # CA, CB, Cout, dims, low-res dims, G: joins that cannot fold
    (32, 64, 64, (7, 9, 18), (3, 4, 9), 8),          # non-2x
    (512, 1024, 512, (4, 4, 4), (2, 2, 2), 8),       # low-res smaller than the tile
]
COLS = [                                # the column kernel: stem, narrow net, narrow join
    (1, 0, 32, (5, 6, 7), None, 1),
    (8, 0, 16, (4, 5, 6), None, 2),
    (8, 8, 16, (5, 7, 9), (2, 3, 4), 2),
]
FOLD_JOIN = (32, 64, 64, (8, 16, 32), (4, 8, 16), 8)   # the foldable join of test_weight_gradient_of_a_decoder_join_vs_float64
# 1 < S < tiles on both halves: 96 skip tiles over 8 workgroups of 12, 12 low-res tiles over 6 workgroups of 2 (8 allowed)
FOLD_JOIN_UNEVEN = (256, 256, 256, (6, 16, 64), (3, 8, 32), 8)
FOLD_JOINS = [FOLD_JOIN, FOLD_JOIN_UNEVEN]


def as_join(c):
    """A PLAIN case in the six-field form of the others."""
    return (c[0], 0, c[1], c[2], None, c[3])


def ids(cases):
    return ["-".join(str(v).replace(" ", "") for v in c) for c in cases]


WIDE_PLAIN = [as_join(c) for c in PLAIN if c[0] % 32 == 0]      # the plain layers wide enough for the tiled kernels
EXACT_FP32 = [as_join(c) for c in PLAIN[:3]] + JOINS[:1]          # passes = 0: test_wgrad_exact_fp32_kernel_vs_float64's cases
ALL = [as_join(c) for c in PLAIN] + JOINS + COLS + FOLD_JOINS

_WS_OR_F16 = ("f16", "ws", "f16", "ws")              # a plain layer with Cout % 64 == 0, Cin % 32 == 0
_F16 = ("f16",) * 4                                  # a join on tiles that cannot fold: CB > 0 keeps it off "ws" as well
_COLS = ("cols",) * 4                                # Cout % 64, Cin % 32 or CA % 32 != 0
_FOLD = ("f16", "f16", "fold+f16", "fold+ws")        # exact 2x, CB % 32 == 0, low-res h >= 4 and w >= 16
ROUTES = {
    as_join(PLAIN[0]): _WS_OR_F16,
    as_join(PLAIN[1]): _WS_OR_F16,
    as_join(PLAIN[2]): _WS_OR_F16,
    as_join(PLAIN[3]): _WS_OR_F16,
    as_join(PLAIN[4]): _WS_OR_F16,
    as_join(PLAIN[5]): _WS_OR_F16,
    as_join(PLAIN[6]): _WS_OR_F16,
    as_join(PLAIN[7]): _COLS,                        # 48 input channels
    as_join(PLAIN[8]): _WS_OR_F16,
    JOINS[0]: _F16,                                  # 7 != 2 x 3
    JOINS[1]: _F16,                                  # low-res 2 x 2 x 2 is below the 4 x 16 tile
    COLS[0]: _COLS,
    COLS[1]: _COLS,
    COLS[2]: _COLS,
    FOLD_JOIN: _FOLD,
    FOLD_JOIN_UNEVEN: _FOLD,
}

# the child processes of the bits test: environment, `allow` that environment amounts to on an MI355X, (case, passes) list
BITS_RUNS = {
    "default": ({}, 3, [(c, 3) for c in ALL] + [(c, 0) for c in EXACT_FP32]),
    "ws0": ({"BFM_WGRAD_WS": "0"}, 2, [(c, 3) for c in WIDE_PLAIN + FOLD_JOINS]),
    "upfold0": ({"BFM_WGRAD_UPFOLD": "0"}, 1, [(c, 3) for c in FOLD_JOINS]),
}

# the grid of the split invariants and of the recorded workspace bound (tests/golden/wgrad_plan.json)
GRID_COUT = (16, 32, 64, 128, 256, 512, 1024)
GRID_CHANNELS = ((1, 0), (8, 0), (8, 8), (48, 0), (32, 0), (64, 0), (32, 64), (256, 256), (512, 1024))      # CA, CB
GRID_DIMS = ((1, 2, 3), (2, 2, 2), (4, 4, 4), (3, 4, 16), (2, 5, 9), (5, 7, 19), (6, 9, 33), (8, 16, 32), (6, 16, 64),
             (7, 9, 18), (16, 16, 16), (24, 40, 48), (32, 32, 32), (64, 64, 64), (80, 96, 112), (128, 128, 128), (160, 160, 160))


def grid_lows(dims):
    """Low-res extents of a join at `dims`: half of every axis (exact 2x where all are even) and about a third (2x on no
    axis longer than 2)."""
    return [tuple(max(1, v // 2) for v in dims), tuple((v + 2) // 3 for v in dims)]


PLAN_LEN = 20                          # int64 entries of bfm_conv3x3x3_wgrad_plan's array (include/brainfm_hip.h)
_ROUTE_NAMES = ("ws", "fold", "f16", "fp32", "cols")


def route_name(plan):
    """The route of a plan array in the words of ROUTES."""
    r = _ROUTE_NAMES[plan[0]]
    return r + ("+ws" if plan[1] else "+f16") if r == "fold" else r


def launches(plan):
    """The launches of a plan array as dicts (the second only on a folded join)."""
    keys = ("nbz", "nby", "nbx", "ntiles", "cols", "S", "per", "off", "bytes")
    out = [dict(zip(keys, plan[2 + 9 * i:11 + 9 * i])) for i in range(2)]
    return out if plan[0] == 1 else out[:1]


def plan(lib, case, passes, allow):
    """(plan array as a list, exact workspace bytes) of a six-field case from bfm_conv3x3x3_wgrad_plan."""
    ca, cb, cout, dims, lo, _ = case
    lo = lo or (0, 0, 0)
    arr, total = (C.c_int64 * PLAN_LEN)(), C.c_size_t(0)
    rc = lib.bfm_conv3x3x3_wgrad_plan(ca, cb, cout, dims[0], dims[1], dims[2], lo[0], lo[1], lo[2], passes, allow, arr,
                                      C.byref(total))
    assert rc == 0, (case, passes, allow, rc)
    return list(arr), total.value


class _Wg:
    """Inputs of one weight-gradient case on the device: A, B, scale (in [0.5, 1.5) times a per-group factor from
    {0.1, 1, 10}), shift, the float64 GroupNorm-applied input X and its true per-group max |X|, a unit-variance dP."""

    def __init__(self, ca, cb, cout, dims, lo, G, seed=0):
        import backward_refs as R
        import test_gpu_backward as TB
        dev = TB._dev()
        self.ca, self.cb, self.cout, self.dims, self.lo, self.G = ca, cb, cout, dims, lo, G
        cin = self.cin = ca + cb
        g = torch.Generator().manual_seed(seed + ca + 3 * cb + 7 * cout + sum(dims))
        self.A = torch.randn(dims + (ca,), generator=g).to(dev)
        self.B = torch.randn(lo + (cb,), generator=g).to(dev) if cb else None
        fac = torch.tensor([0.1, 1.0, 10.0])[torch.randint(0, 3, (G,), generator=g)]
        if G >= 3:
            fac[:3] = torch.tensor([10.0, 0.1, 1.0])                           # all three factors occur
        self.scale = ((torch.rand(cin, generator=g) + 0.5) * fac.repeat_interleave(cin // G)).to(dev)
        self.shift = (torch.randn(cin, generator=g) * 0.1).to(dev)
        self.dP = torch.randn(dims + (cout,), generator=g).to(dev)
        self.up = None
        if cb:
            self.up, _ = TB._Tables.get(lo, dims)
        maps = R.up_maps(lo, dims, dev) if cb else None
        self.X = R.join(self.A, self.B, maps).double() * self.scale.double() + self.shift.double()
        self.xb = self.X.abs().reshape(-1, G, cin // G).amax(dim=(0, 2)).float().contiguous()

    def run(self, dP, passes=3, dp_bound=None, ex=True):
        from brainfm_amd import _lib as L
        lib = L.load()
        D, H, W = self.dims
        dev = dP.device
        if dp_bound is None:
            dp_bound = dP.abs().max().reshape(1)
        nws = lib.bfm_conv3x3x3_wgrad_workspace(self.cin, self.cout, D, H, W)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        dW = torch.full((self.cout, self.cin, 27), NAN, dtype=torch.float32, device=dev)
        upp = C.byref(self.up) if self.cb else None
        if ex:
            rc = lib.bfm_conv3x3x3_wgrad_ex(L.ptr(dP), self.cout, L.ptr(self.A), self.ca, L.ptr(self.B), self.cb, D, H, W, upp,
                                            L.ptr(self.scale), L.ptr(self.shift), L.ptr(dp_bound), L.ptr(self.xb), self.G,
                                            passes, L.ptr(dW), L.ptr(ws), nws, L.stream_ptr())
        else:
            rc = lib.bfm_conv3x3x3_wgrad(L.ptr(dP), self.cout, L.ptr(self.A), self.ca, L.ptr(self.B), self.cb, D, H, W, upp,
                                         L.ptr(self.scale), L.ptr(self.shift), L.ptr(dW), L.ptr(ws), nws, L.stream_ptr())
        L.check(rc, "wgrad")
        return dW

    def err(self, dW, dP):
        import backward_refs as R
        assert bool(torch.isfinite(dW).all())
        return R.rel_err(dW, R.wgrad_ref(self.X, dP))
