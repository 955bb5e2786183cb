"""Every kernel of the backward pass (brainfm_amd/csrc/backward.hip, brainfm_amd/backward.py) on its own against the
float64 references of tests/backward_refs.py -- the whole-net gradient tests of test_gpu_infer.py / test_gpu_train.py see
these kernels only through parameter gradients at 5e-4 .. 3e-3 of a tensor's maximum.  Shapes are the smallest that
reach each code path; every output buffer starts as NaN, so an element a kernel does not write fails its test.
Needs an MI355X: run with `-m gpu`."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import backward_refs as R
from wgrad_cases import COLS, FOLD_JOIN, FOLD_JOINS, JOINS, PLAIN, WGRAD_TOL, _Wg

pytestmark = pytest.mark.gpu

E_SHAPE, E_WORKSPACE = -2, -3
NAN = float("nan")


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _lib():
    from brainfm_amd import _lib as L
    return L, L.load()


def _engine_slope():
    from brainfm_amd.engine import UNetEngine
    return float(inspect.signature(UNetEngine.__init__).parameters["slope"].default)


class _Tables:
    """What UNetEngine._upsample_desc and backward._start_tables use of an engine: the upsampling descriptor and the
    start tables of a kernel test are made by the code that makes them for a training step."""
    _per_device = {}

    def __init__(self, dev):
        self.device = dev
        self._up_cache = {}

    @classmethod
    def get(cls, lo, dims):
        from brainfm_amd import backward as BW
        from brainfm_amd.engine import UNetEngine
        dev = _dev()
        me = cls._per_device.setdefault(str(dev), cls(dev))
        return UNetEngine._upsample_desc(me, lo, dims), BW._start_tables(me, lo, dims)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------- 2. LeakyReLU backward
N_SWEEP = 4 * (4096 * 256 + 5)          # more float4 than one sweep of the kernel's 4096 x 256 threads


@pytest.mark.parametrize("slope", [_engine_slope(), 0.25])
@pytest.mark.parametrize("n", [4, 1020, N_SWEEP])
def test_lrelu_bwd_bitwise(n, slope):
    """bfm_lrelu_bwd_ex is exact in fp32: dP bit-equal to where(Y > 0, dY, dY * float32(slope)) with +0.0 and -0.0 in Y
    taking the slope, absmax bit-equal to max |dP| with the maximum in the last float4 and absmax holding 1e30 before the
    call, exactly 0.0 for dY = 0; bfm_lrelu_bwd writes the same dP."""
    L, lib = _lib()
    dev = _dev()
    g = torch.Generator().manual_seed(n % 1000)
    Y = torch.randn(n, generator=g)
    dY = torch.randn(n, generator=g)
    Y[0], Y[1] = 0.0, -0.0
    dY[0], dY[1] = 1.5, -2.5
    Y[n - 2], dY[n - 2] = -1.0, -4096.0 / 3.0                   # the largest |dP| sits in the last float4, on the slope side
    Y, dY = Y.to(dev), dY.to(dev)
    s32 = torch.tensor(slope, dtype=torch.float32, device=dev)
    ref = torch.where(Y > 0, dY, dY * s32)
    assert float(ref.abs().max()) == abs(float(ref[n - 2]))
    st = L.stream_ptr()
    dP = torch.full((n,), NAN, device=dev)
    am = torch.full((1,), 1e30, device=dev)
    L.check(lib.bfm_lrelu_bwd_ex(L.ptr(dY), L.ptr(Y), n, slope, L.ptr(dP), L.ptr(am), st), "lrelu_bwd_ex")
    assert torch.equal(_bits(dP), _bits(ref))
    assert torch.equal(_bits(am), _bits(ref.abs().max().reshape(1)))
    assert float(dP[0]) == float(np.float32(1.5) * np.float32(slope)) and float(dP[1]) == float(np.float32(-2.5) * np.float32(slope))
    dP2 = torch.full((n,), NAN, device=dev)
    L.check(lib.bfm_lrelu_bwd(L.ptr(dY), L.ptr(Y), n, slope, L.ptr(dP2), st), "lrelu_bwd")
    assert torch.equal(_bits(dP2), _bits(ref))
    zero = torch.zeros(n, device=dev)
    am.fill_(1e30)
    dP.fill_(NAN)
    L.check(lib.bfm_lrelu_bwd_ex(L.ptr(zero), L.ptr(Y), n, slope, L.ptr(dP), L.ptr(am), st), "lrelu_bwd_ex(0)")
    assert float(am) == 0.0 and not bool(torch.signbit(am).any())
    assert bool((dP == 0).all())


def test_lrelu_bwd_rejects_a_length_that_is_no_multiple_of_four():
    L, lib = _lib()
    dev = _dev()
    x = torch.ones(8, device=dev)
    dP = torch.full((8,), NAN, device=dev)
    am = torch.full((1,), NAN, device=dev)
    for n in (1, 6, 7):
        assert lib.bfm_lrelu_bwd_ex(L.ptr(x), L.ptr(x), n, 0.01, L.ptr(dP), L.ptr(am), L.stream_ptr()) == E_SHAPE
        assert lib.bfm_lrelu_bwd(L.ptr(x), L.ptr(x), n, 0.01, L.ptr(dP), L.stream_ptr()) == E_SHAPE
    assert bool(torch.isnan(dP).all()) and bool(torch.isnan(am).all())


# ----------------------------------------------------------------------------------------------- 3. MaxPool3d(2) backward
POOL_DIMS = [(2, 2, 2), (3, 3, 3), (2, 3, 5), (5, 2, 4), (4, 5, 2), (6, 4, 7), (7, 7, 6)]      # every parity combination


@pytest.mark.parametrize("dims", POOL_DIMS)
@pytest.mark.parametrize("c", [1, 3, 6, 4, 8, 36])
def test_maxpool2_bwd_bitwise(c, dims):
    """bfm_maxpool2_bwd (element-centric kernel for C = 1, 3, 6; window-centric for C = 4, 8, 36) bit-equal to first-maximum
    routing on inputs full of ties, on a constant input and on distinct values, odd trailing slices zero; and with
    dOut = 1 the ones of dIn mark, one per window, the values bfm_maxpool2 returns."""
    L, lib = _lib()
    dev = _dev()
    D, H, W = dims
    lo = (D // 2, H // 2, W // 2)
    st = L.stream_ptr()
    g = torch.Generator().manual_seed(c * 100 + D * 16 + H * 4 + W)
    for kind in ("ties", "zeros", "distinct"):
        x = R.pool_input(kind, dims, c, g).to(dev)
        dOut = torch.randn(lo + (c,), generator=g).to(dev)
        dIn = torch.full(dims + (c,), NAN, device=dev)
        L.check(lib.bfm_maxpool2_bwd(L.ptr(x), L.ptr(dOut), c, D, H, W, L.ptr(dIn), st), "maxpool2_bwd")
        assert torch.equal(dIn.double(), R.maxpool2_bwd_ref(x, dOut)), (kind, c, dims)
        ones = torch.ones(lo + (c,), device=dev)
        dIn.fill_(NAN)
        L.check(lib.bfm_maxpool2_bwd(L.ptr(x), L.ptr(ones), c, D, H, W, L.ptr(dIn), st), "maxpool2_bwd(1)")
        out = torch.full(lo + (c,), NAN, device=dev)
        L.check(lib.bfm_maxpool2(L.ptr(x), c, D, H, W, L.ptr(out), st), "maxpool2")
        assert bool(((dIn == 0) | (dIn == 1)).all())

        def windows(t):
            return t[:2 * lo[0], :2 * lo[1], :2 * lo[2]].reshape(lo[0], 2, lo[1], 2, lo[2], 2, c)
        assert bool((windows(dIn).sum(dim=(1, 3, 5)) == 1).all()), (kind, c, dims)
        assert float(dIn.sum()) == float(ones.sum())                           # nothing outside the windows
        assert torch.equal(windows(dIn * x).sum(dim=(1, 3, 5)), out), (kind, c, dims)


# ----------------------------------------------------------------------------------------------- 4. GroupNorm backward
GN_CASES = {                                    # CA, CB, G, full-res dims, low-res dims
    1: (32, 0, 8, (5, 6, 7), None),              # quad path
    2: (1, 0, 1, (5, 6, 7), None),               # stem, scalar path
    3: (6, 0, 2, (3, 5, 9), None),               # scalar path, C % 4 != 0
    4: (32, 64, 8, (6, 8, 10), (3, 4, 5)),       # exact 2x; 12 channels per group: a group straddles the A / B boundary
    5: (32, 64, 8, (7, 9, 11), (3, 4, 5)),       # replica boxes of 2 and 3
    6: (3, 6, 3, (5, 7, 9), (2, 3, 4)),          # scalar path with B
    7: (1024, 2048, 8, (4, 4, 4), (2, 2, 2)),    # three 1024-channel chunks, 384 channels per group
    8: (8, 0, 2, (24, 28, 30), None),            # 20 160 voxels: the 1024-block cap, 20 voxels per block
    9: (320, 0, 8, (2, 2, 2), None),             # 80 quads do not divide 256: idle threads in the partial kernel
}
GN_TOL = {"dA": 2e-6, "dbeta": 2e-6, "dB": 5e-6, "dgamma": 1e-5}


def _gn_inputs(case, m):
    ca, cb, G, dims, lo = GN_CASES[case]
    g = torch.Generator().manual_seed(1000 * case + m)
    A = torch.randn(dims + (ca,), generator=g) * 1.5 + m
    B = (torch.randn(lo + (cb,), generator=g) * 1.5 + m) if cb else None
    gamma = torch.rand(ca + cb, generator=g) + 0.5
    dXn = torch.randn(dims + (ca + cb,), generator=g)
    return A, B, gamma, dXn


def _gn_call(lib, L, A, B, gamma, dXn, G, dims, lo, mean, rstd, ws_short=0):
    dev = A.device
    ca, cb = A.shape[-1], (0 if B is None else B.shape[-1])
    D, H, W = dims
    upp, starts = None, [None] * 3
    if cb:
        up, starts = _Tables.get(lo, dims)
        upp = C.byref(up)
    out = dict(dA=torch.full(dims + (ca,), NAN, device=dev), dB=torch.full(lo + (cb,), NAN, device=dev) if cb else None,
               dgamma=torch.full((ca + cb,), NAN, device=dev), dbeta=torch.full((ca + cb,), NAN, device=dev))
    nws = lib.bfm_gn_bwd_workspace(ca + cb, D, H, W) - ws_short
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    rc = lib.bfm_gn_bwd(L.ptr(dXn), L.ptr(A), ca, L.ptr(B), cb, D, H, W, upp, L.ptr(starts[0]), L.ptr(starts[1]),
                        L.ptr(starts[2]), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), G, L.ptr(out["dA"]), L.ptr(out["dB"]),
                        L.ptr(out["dgamma"]), L.ptr(out["dbeta"]), L.ptr(ws), nws, L.stream_ptr())
    return rc, out


@pytest.mark.parametrize("m", [1, 30])
@pytest.mark.parametrize("case", sorted(GN_CASES))
def test_gn_bwd_vs_float64(case, m):
    """bfm_gn_bwd against float64 autograd through cat(A, up(B)) -> group_norm, with the float32 roundings of the float64
    group statistics as mean / rstd, inputs centred at m = 1 and at m = 30 (20 sigma off centre, where (x - mean) * rstd
    loses digits).  Bounds (max |err| / max |ref|): dA, dbeta 2e-6, dB 5e-6, dgamma 1e-5 -- ten times what a float32
    restatement of the kernel's formula reaches against float64 on the CPU at these cases (dA 1.6e-7, dB 8.7e-8,
    dgamma 9.5e-7 at m = 30); dB has room for the fp32 sum over up to 27 replicas.
    The device errors are printed per case and output (run with -s)."""
    L, lib = _lib()
    dev = _dev()
    ca, cb, G, dims, lo = GN_CASES[case]
    A, B, gamma, dXn = _gn_inputs(case, m)
    ref = R.gn_bwd_ref(A, B, R.up_maps(lo, dims) if cb else None, gamma, G, dXn)
    Ad, gd, dd = A.to(dev), gamma.to(dev), dXn.to(dev)
    Bd = B.to(dev) if cb else None
    rc, out = _gn_call(lib, L, Ad, Bd, gd, dd, G, dims, lo, ref["mean"].float().to(dev), ref["rstd"].float().to(dev))
    L.check(rc, "gn_bwd")
    errs = {k: R.rel_err(out[k], ref[k]) for k in GN_TOL if ref[k] is not None}
    print("gn_bwd case %d m=%d: " % (case, m) + "  ".join("%s %.2e" % (k, v) for k, v in errs.items()))
    for k, v in errs.items():
        assert bool(torch.isfinite(out[k]).all()), k
        assert v <= GN_TOL[k], (case, m, k, v)


def test_gn_bwd_error_paths_launch_nothing():
    """G = 33 and C % G != 0 are BFM_E_SHAPE, a workspace one byte short is BFM_E_WORKSPACE; the outputs stay NaN."""
    L, lib = _lib()
    dev = _dev()
    dims = (3, 4, 5)
    for ca, G, short, want in ((66, 33, 0, E_SHAPE), (32, 33, 0, E_SHAPE), (30, 8, 0, E_SHAPE), (32, 8, 1, E_WORKSPACE)):
        A = torch.randn(dims + (ca,), device=dev)
        stat = torch.ones(64, device=dev)
        rc, out = _gn_call(lib, L, A, None, torch.ones(ca, device=dev), torch.randn(dims + (ca,), device=dev), G, dims, None,
                           stat, stat, ws_short=short)
        assert rc == want, (ca, G, short, rc)
        torch.cuda.synchronize()
        for k in ("dA", "dgamma", "dbeta"):
            assert bool(torch.isnan(out[k]).all()), (ca, G, k)


# ----------------------------------------------------------------------------------------------- 5. weight gradient
# the cases, their inputs (_Wg) and the bound are shared with the route and bits tests: tests/wgrad_cases.py
def _ids(cases):
    return ["-".join(str(v).replace(" ", "") for v in c) for c in cases]


@pytest.mark.parametrize("cin,cout,dims,G", PLAIN, ids=_ids(PLAIN))
def test_wgrad_plain_layers_vs_float64(cin, cout, dims, G):
    """bfm_conv3x3x3_wgrad_ex, passes = 3, on plain layers: conv_wgrad_ws_kernel with extents that are no multiple of, equal
    to and below its 4 x 16 tile, the deep-level 4^3 / 2^3 / (1, 2, 3) volumes, 1024 x 1024 channels (more workgroup columns
    than the split budget), 48 input channels on the fp32 column kernel, and 256 x 256 channels at (6, 9, 33), where every
    workgroup takes seven tiles and the last one five; eight groups whose bounds differ 100-fold.  The routes named here and
    below are asserted by tests/test_host_wgrad_plan.py and tests/test_gpu_wgrad_bits.py."""
    w = _Wg(cin, 0, cout, dims, None, G)
    e = w.err(w.run(w.dP), w.dP)
    print("wgrad plain %s: %.2e" % ((cin, cout, dims, G), e))
    assert e <= WGRAD_TOL, e


@pytest.mark.parametrize("ca,cb,cout,dims,lo,G", JOINS + COLS, ids=_ids(JOINS + COLS))
def test_wgrad_unfolded_joins_and_column_kernel_vs_float64(ca, cb, cout, dims, lo, G):
    """Decoder joins that cannot take the folded kernel (non-2x upsampling; a low-res tensor smaller than the tile) on
    conv_wgrad_f16_kernel, and conv_wgrad_cols_kernel on the one-channel stem, an 8 -> 16 layer and an 8 + 8 -> 16 join."""
    w = _Wg(ca, cb, cout, dims, lo, G)
    e = w.err(w.run(w.dP), w.dP)
    print("wgrad %s: %.2e" % ((ca, cb, cout, dims, lo, G), e))
    assert e <= WGRAD_TOL, e


@pytest.mark.parametrize("ca,cb,cout,dims,lo,G", FOLD_JOINS, ids=_ids(FOLD_JOINS))
def test_wgrad_folded_joins_vs_float64(ca, cb, cout, dims, lo, G):
    """Exact-2x decoder joins on the folded route (skip channels on conv_wgrad_ws_kernel, upsampled channels on
    conv_wgrad_up_f16_kernel): one workgroup per tile, and 256 + 256 -> 256 channels where the workgroups of both halves
    take several tiles each (12 and 2) and the upsampled half runs 6 workgroups where the budget allows 8.
    tests/test_host_wgrad_plan.py holds the routes to what is said here."""
    w = _Wg(ca, cb, cout, dims, lo, G)
    e = w.err(w.run(w.dP), w.dP)
    print("wgrad folded %s: %.2e" % ((ca, cb, cout, dims, lo, G), e))
    assert e <= WGRAD_TOL, e


@pytest.mark.parametrize("ca,cb,cout,dims,lo,G", [(c[0], 0, c[1], c[2], None, c[3]) for c in PLAIN[:3]] + JOINS[:1],
                         ids=_ids(PLAIN[:3] + JOINS[:1]))
def test_wgrad_exact_fp32_kernel_vs_float64(ca, cb, cout, dims, lo, G):
    """passes = 0 (conv_wgrad_tiled_kernel, v_mfma_f32_32x32x2_f32) through bfm_conv3x3x3_wgrad and through _ex: bit-equal
    to each other, and within the split-fp16 bound of float64; the measured error is printed."""
    w = _Wg(ca, cb, cout, dims, lo, G)
    a = w.run(w.dP, passes=0, ex=True)
    b = w.run(w.dP, passes=0, ex=False)
    assert torch.equal(_bits(a), _bits(b))
    e = w.err(a, w.dP)
    print("wgrad passes=0 %s: %.2e" % ((ca, cb, cout, dims, lo, G), e))
    assert e <= WGRAD_TOL, e


MAG_LAYERS = [(64, 0, 64, (5, 7, 19), None, 8), FOLD_JOIN]


@pytest.mark.parametrize("mag", [1e-9, 1e-2, 1e4, "lrelu"])
@pytest.mark.parametrize("ca,cb,cout,dims,lo,G", MAG_LAYERS, ids=_ids(MAG_LAYERS))
def test_wgrad_magnitudes_of_dp(ca, cb, cout, dims, lo, G, mag):
    """dP at 1e-9, 1e-2 and 1e+4 (loss scaling): the power-of-two operand scale makes the relative error independent of the
    magnitude, so the same 2e-5 holds at each; and once with dP and its bound as bfm_lrelu_bwd_ex leaves them on the stream."""
    L, lib = _lib()
    w = _Wg(ca, cb, cout, dims, lo, G, seed=5)
    if mag == "lrelu":
        g = torch.Generator().manual_seed(3)
        Y = torch.randn(w.dP.shape, generator=g).to(w.dP.device)
        dP = torch.full_like(w.dP, NAN)
        bnd = torch.full((1,), 1e30, device=w.dP.device)
        L.check(lib.bfm_lrelu_bwd_ex(L.ptr(w.dP), L.ptr(Y), w.dP.numel(), _engine_slope(), L.ptr(dP), L.ptr(bnd),
                                     L.stream_ptr()), "lrelu_bwd_ex")
        dW = w.run(dP, dp_bound=bnd)
        assert float(bnd) == float(dP.abs().max())
    else:
        dP = w.dP * mag
        dW = w.run(dP)
    e = w.err(dW, dP)
    print("wgrad %s dP x %s: %.2e" % ((ca, cb, cout, dims), mag, e))
    assert e <= WGRAD_TOL, (mag, e)


@pytest.mark.parametrize("ca,cb,cout,dims,lo,G", MAG_LAYERS, ids=_ids(MAG_LAYERS))
def test_wgrad_of_zero_dp_is_exactly_zero(ca, cb, cout, dims, lo, G):
    """dP = 0 with dp_bound = 0 (a head that takes no part in a loss): dW is 0.0 everywhere, no NaN from a scale of 1 / 0."""
    w = _Wg(ca, cb, cout, dims, lo, G)
    zero = torch.zeros_like(w.dP)
    dW = w.run(zero, dp_bound=torch.zeros(1, device=zero.device))
    assert bool((dW == 0).all())


# ----------------------------------------------------------------------------------------------- 6. one SingleConv
_SESSION = {}


def _engine():
    """One 3-level, 64-wide session for all SingleConv cases (the layers are used one at a time)."""
    if "s" not in _SESSION:
        from oracle import unet_ref as O
        from test_gpu_infer import _session
        _SESSION["s"] = _session(sd=O.random_state_dict(1, 64, 3, seed=37), f_maps=64, levels=3)
    return _SESSION["s"].engine


SC_CASES = [                            # block, index, conv, dims, low-res dims
    ("enc", 0, 0, (6, 7, 9), None),     # the one-channel stem
    ("enc", 0, 1, (6, 7, 9), None),     # 32 input channels: data gradient padded to 64 and sliced
    ("enc", 1, 0, (5, 6, 7), None),
    ("dec", 0, 0, (6, 8, 16), (3, 4, 8)),
    ("dec", 0, 0, (7, 9, 11), (3, 4, 5)),
    ("dec", 1, 0, (6, 8, 16), (3, 4, 8)),
    ("dec", 1, 0, (7, 9, 11), (3, 4, 5)),
]


@pytest.mark.parametrize("block,idx,conv,dims,lo", SC_CASES, ids=_ids(SC_CASES))
def test_single_conv_forward_and_all_five_gradients_vs_float64(block, idx, conv, dims, lo):
    """backward.train_single_conv + backward.backward_single_conv of one layer: dA, dB, dW, dgamma, dbeta against float64
    autograd of GroupNorm -> conv3d -> LeakyReLU, each within max(8 x e32, 2e-5) of the float64 tensor's maximum, e32 being the
    error of torch's float32 autograd of the same layer on the CPU (the rule of test_gpu_contrastive.check_against_torch;
    2e-5: the split-fp16 class).  LeakyReLU's mask is a constant taken from the sign of the device's output -- valid because
    that output agrees with the float64 forward within TOL_NET and its sign differs in at most max(3, numel // 100000)
    elements.  tape.bound[g] is at least, and at most (1 + 1e-5) times, the largest |GroupNorm-applied input| of group g
    as the conv kernels form it (fmaf(x, scale, shift) in float32), which in turn sits within 1e-5 of float64 GroupNorm.
    Device error, e32 and bound are printed per tensor."""
    from brainfm_amd import backward as BW
    from test_gpu_infer import TOL_NET
    eng = _engine()
    dev = _dev()
    ly = getattr(eng, block)[idx][conv]
    ca = ly.cin if lo is None else {0: 128, 1: 64}[idx]
    cb = ly.cin - ca
    g = torch.Generator().manual_seed(ly.cin + sum(dims))
    A = (torch.rand(dims + (ca,), generator=g) if ca == 1 else torch.randn(dims + (ca,), generator=g) * 1.5 + 0.5)
    B = torch.randn(lo + (cb,), generator=g) if cb else None
    dY = torch.randn(dims + (ly.cout,), generator=g)
    out, t = BW.train_single_conv(eng, ly, A.to(dev), dims, B=B.to(dev) if cb else None, lo_dims=lo)
    dA, dB, grads = BW.backward_single_conv(eng, t, dY.to(dev))
    got = dict(dA=dA, dB=dB, dW=grads[ly.name + ".conv.weight"].reshape(ly.cout, ly.cin, 27),
               dgamma=grads[ly.name + ".groupnorm.weight"], dbeta=grads[ly.name + ".groupnorm.bias"])
    # float64 and float32 on the CPU, LeakyReLU's mask from the device
    mask = (t.out > 0).cpu()
    maps = R.up_maps(lo, dims) if cb else None
    par = [p.detach().cpu() for p in (ly.gamma, ly.beta, ly.w_raw)]
    r64 = R.single_conv_ref(A.double(), B.double() if cb else None, maps, *[p.double() for p in par], ly.groups, eng.slope,
                            mask=mask, dY=dY.double(), eps=eng.eps)
    r32 = R.single_conv_ref(A, B, maps, *par, ly.groups, eng.slope, mask=mask, dY=dY, eps=eng.eps)
    true_out = torch.where(r64["pre"] > 0, r64["pre"], r64["pre"] * eng.slope)
    assert R.rel_err(t.out, true_out) <= TOL_NET
    flips = int(((r64["pre"] > 0) != mask).sum())
    assert flips <= max(3, mask.numel() // 100000), flips
    # the group bounds of the split-fp16 operand scale
    X = R.join(A, B, maps).double()
    xn32 = (X * t.scale.cpu().double() + t.shift.cpu().double()).float()
    cpg = ly.cin // ly.groups
    gmax = xn32.abs().reshape(-1, ly.groups, cpg).amax(dim=(0, 2))
    bound = t.bound.cpu()
    assert bool((bound >= gmax).all()) and bool((bound.double() <= (1 + 1e-5) * gmax.double()).all()), (bound, gmax)
    gmax64 = r64["xn"].abs().reshape(-1, ly.groups, cpg).amax(dim=(0, 2))
    assert bool(((gmax.double() - gmax64).abs() <= 1e-5 * gmax64).all()), (gmax, gmax64)
    bad = {}
    for k, v in got.items():
        if v is None:
            assert cb == 0 and k == "dB"
            continue
        assert tuple(v.shape) == tuple(r64[k].shape), (k, v.shape, r64[k].shape)
        assert bool(torch.isfinite(v).all()), k
        e, e32 = R.rel_err(v, r64[k]), R.rel_err(r32[k], r64[k])
        lim = max(8.0 * e32, 2e-5)
        print("single_conv %s %s %-6s err %.2e  torch-fp32 %.2e  bound %.2e" % (ly.name.split("backbone.")[-1], dims, k, e, e32, lim))
        if e > lim:
            bad[k] = (e, lim)
    assert not bad, bad
