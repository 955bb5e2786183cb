"""Every forward 3x3x3 convolution kernel of the older family on its own, through the C ABI, against the float64
references of tests/conv_forward_refs.py: bfm_conv3x3x3_mfma_ex (plan variants 0 conv_mfma, 1 conv_mfma_ws, 2 conv_mfma16,
with split-K, two sources, accumulate mode, the batch export), bfm_conv3x3x3_wino_ex (F(2,3)), bfm_conv3x3x3_direct and
bfm_conv3x3x3_stem_ex.  The whole-net tests see these kernels at 1e-3 / 1e-4 of max |y|; a lost lo pass sits at 2e-4
(tests/test_host_conv_forward_refs.py), so the bar here is the family's own: max |out - ref| <= 1e-5 max |ref|.

Every launch has a non-trivial scale, a NON-ZERO shift (zero padding after the affine is then not the same as padding
before it), slope 0.01, G = 8 and a per-group bound taken from the affine-applied input.  Outputs of non-accumulating
launches start as NaN and must come back finite; every output has a 4096-float sentinel tail that must stay untouched.
The variant is chosen through cfg[6], never through the environment.  Each case prints one line: kernel, plan, measured
error, error of torch-CPU fp32 conv3d on the same operands.

Measured on MI355X, worst over the cases of this module, of max |ref| (torch-CPU fp32: 4e-7 .. 9e-7); also in HISTORY.md
section 1:
    kernel                      passes=3 vs float64                      passes=1
    conv_mfma     (variant 0)   1.5e-6 (split-K 4.9e-7, batch 8.5e-7)    5.3e-7 of the hi*hi emulation, 1.00x its distance
    conv_mfma_ws  (variant 1)   1.3e-6                                   the bits of variant 0
    conv_mfma16   (variant 2)   1.5e-6 (split-K 5.0e-7, batch 9.4e-7)    the bits of variant 0
    conv_wino     F(2,3)        6.2e-7                                   5.45e-4 vs float64 = 1.97x the emulation's 2.77e-4
    conv_direct                 7.8e-7
    conv_stem_mfma (Cin = 1)    2.9e-7 (meets 1e-5; its sibling's 1e-4 is not needed)
Needs an MI355X: run with `-m gpu`."""
import ctypes as C
import functools

import pytest
import torch

import conv_forward_refs as R

pytestmark = pytest.mark.gpu

SLOPE = 0.01
G = 8
BAR = 1e-5                       # the family's kernel bar: 20x under a lost lo pass, 20x over fp32 accumulation
TAIL = 4096
SENT = -7777.0
NAN = float("nan")
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
PACKER = {0: "mfma", 1: "mfma", 2: "mfma16"}
KERNEL = {0: "conv_mfma", 1: "conv_mfma_ws", 2: "conv_mfma16"}


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _lib():
    from brainfm_amd import _lib as L
    return L, L.load()


class _Up:
    """The upsampling descriptor of a two-source launch, made by the engine's own code (UNetEngine._upsample_desc)."""
    _me = None

    def __init__(self, dev):
        self.device = dev
        self._up_cache = {}

    @classmethod
    def get(cls, lo, dims):
        from brainfm_amd.engine import UNetEngine
        if cls._me is None:
            cls._me = cls(_dev())
        return UNetEngine._upsample_desc(cls._me, tuple(lo), tuple(dims))


class _Case:
    """Operands of one layer on the host and the device, its float64 pre-activation, and its packed weights per packer."""

    def __init__(self, dims, ca, cout, cb, lo, seed, mag, wseed):
        dev = _dev()
        g = torch.Generator().manual_seed(1000 * seed + 7 * ca + cb + dims[2])
        gw = torch.Generator().manual_seed(wseed) if wseed is not None else g
        cin = ca + cb
        self.dims, self.ca, self.cb, self.cin, self.cout, self.lo = tuple(dims), ca, cb, cin, cout, lo
        A = torch.randn(self.dims + (ca,), generator=g) * 1.7 + 0.2
        B = torch.randn(tuple(lo) + (cb,), generator=g) * 0.8 - 0.1 if cb else None
        scale = torch.rand(cin, generator=g) + 0.5
        shift = torch.randn(cin, generator=g) * 0.3
        shift = torch.where(shift.abs() < 0.02, torch.full_like(shift, 0.05), shift)       # every channel's shift matters
        w = torch.randn(cout, cin, 3, 3, 3, generator=gw) * 0.05
        if isinstance(mag, tuple):                     # ("mul", f): the affine-applied input scaled by f
            A, shift = A * mag[1], shift * mag[1]
            B = None if B is None else B * mag[1]
        elif mag == "spread":                          # the groups' magnitudes spread over 1e4
            grp = torch.arange(cin) // max(1, cin // G)
            f = 10.0 ** (-4.0 * grp.float() / (G - 1))
            scale, shift = scale * f, shift * f
        elif mag == "zero":
            A, shift = torch.zeros_like(A), torch.zeros_like(shift)
        self.maps = R.up_maps(lo, dims) if cb else None
        self.A, self.B, self.scale, self.shift, self.w = A, B, scale, shift, w
        X = R.join(A, B, self.maps)
        self.y32 = R.affine_fp32(X, scale, shift)
        self.y32_fused = R.affine_fp32(X, scale, shift, fused=True)
        self.bound = R.group_bound(self.y32, G) if cin % G == 0 else self.y32.abs().max().reshape(1)
        self.pre = R.conv_ref(A, B, self.maps, scale, shift, w, 1.0)       # slope 1: the convolution itself, float64
        self.f32 = R.rel_err(R.lrelu(R._conv_cl(self.y32, w), SLOPE), R.lrelu(self.pre, SLOPE))
        self.dA, self.dscale, self.dshift, self.dbound, self.dw = (t.to(dev).contiguous() for t in
                                                                   (A, scale, shift, self.bound, w))
        self.dB = B.to(dev).contiguous() if cb else None
        self.up = _Up.get(lo, dims) if cb else None
        self._packs = {}

    def ref(self, prior=None, slope=SLOPE):
        return R.lrelu(self.pre if prior is None else self.pre + prior.double().cpu(), slope)

    def pack(self, kind, passes=3):
        key = (kind, passes if kind == "wino" else 0)
        if key not in self._packs:
            L, lib = _lib()
            wmax = float(self.w.abs().max())
            wexp = C.c_int(0)
            if kind == "direct":
                wp = torch.empty(27 * self.cin * self.cout, dtype=torch.float32, device=_dev())
                L.check(lib.bfm_pack_conv_weights_direct(L.ptr(self.dw), self.cin, self.cout, L.ptr(wp), L.stream_ptr()), "pack")
            elif kind == "wino":
                wp = torch.empty(lib.bfm_pack_conv_weights_wino_bytes(self.cin, self.cout, passes), dtype=torch.uint8, device=_dev())
                L.check(lib.bfm_pack_conv_weights_wino(L.ptr(self.dw), self.cin, self.cout, wmax, passes, L.ptr(wp),
                                                       C.byref(wexp), L.stream_ptr()), "pack_wino")
            else:
                nbytes = getattr(lib, "bfm_pack_conv_weights_%s_bytes" % kind)(self.cin, self.cout)
                wp = torch.empty(nbytes, dtype=torch.uint8, device=_dev())
                L.check(getattr(lib, "bfm_pack_conv_weights_%s" % kind)(L.ptr(self.dw), self.cin, self.cout, wmax, L.ptr(wp),
                                                                        C.byref(wexp), L.stream_ptr()), "pack_" + kind)
            self._packs[key] = (wp, wexp.value)
        return self._packs[key]


@functools.lru_cache(maxsize=None)
def _case(dims, ca, cout, cb=0, lo=None, seed=0, mag=None, wseed=None):
    return _Case(dims, ca, cout, cb, lo, seed, mag, wseed)


def _out_buf(dims, cout, prior=None):
    """(flat buffer with the sentinel tail, the (D, H, W, Cout) view of its head): NaN, or the prior of accumulate mode."""
    n = dims[0] * dims[1] * dims[2] * cout
    flat = torch.full((n + TAIL,), SENT, device=_dev())
    flat[:n] = NAN if prior is None else prior.reshape(-1).to(_dev())
    return flat, flat[:n].view(tuple(dims) + (cout,))


def _rows_buf(n, cout):
    _, lib = _lib()
    return torch.zeros(lib.bfm_moment_rows_bytes(n, cout), dtype=torch.uint8, device=_dev())


def _check_out(label, flat, out, ref, f32, bar=BAR):
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), label + ": an element was not written (NaN left) or is not finite"
    assert bool((flat[out.numel():] == SENT).all()), label + ": wrote behind the output"
    e = R.rel_err(out, ref)
    print("%s: err %.2e, torch fp32 %.2e" % (label, e, f32))
    assert e <= bar, (label, e)
    return e


def _check_rows(label, rows, n, out):
    """The moment rows are the moments of what was stored (tolerances of test_producer_moment_rows_equal_activation_moments:
    sums go through fp32 partials of <= 32 values, min / max are exact)."""
    c = out.shape[-1]
    k = n * c
    rs = rows[:k * 8].view(torch.float64).view(n, c).sum(0)
    rq = rows[k * 8:k * 16].view(torch.float64).view(n, c).sum(0)
    rmn = rows[k * 16:k * 20].view(torch.float32).view(n, c).min(0)[0]
    rmx = rows[k * 20:k * 24].view(torch.float32).view(n, c).max(0)[0]
    td = out.double().reshape(-1, c)
    assert float((rs - td.sum(0)).abs().max()) <= 2e-7 * float(td.abs().sum(0).max()), label
    assert float((rq - (td * td).sum(0)).abs().max()) <= 2e-7 * float((td * td).sum(0).max()), label
    assert torch.equal(rmn, out.reshape(-1, c).min(0)[0]) and torch.equal(rmx, out.reshape(-1, c).max(0)[0]), label


def _cdiv(a, b):
    return -(-a // b)


def _eff_splitk(cin, s):
    kcn = cin // 16
    s = max(1, min(s, kcn))
    return _cdiv(kcn, _cdiv(kcn, s))


def _plan(cs, ver, wg=None, box=None, splitk=1, accum=False):
    L, lib = _lib()
    cfg = (C.c_int * 8)()
    L.check(lib.bfm_conv3x3x3_mfma_plan(cs.cin, cs.cout, cs.dims[0], cs.dims[1], cs.dims[2], cfg), "plan")
    if wg is not None:
        cfg[0], cfg[1] = wg
    if box is not None:
        cfg[2], cfg[3], cfg[4] = box
    cfg[5], cfg[6], cfg[7] = splitk, ver, 1 if accum else 0
    # the launcher's own constraints (conv_mfma_launch): a forced plan it would refuse is a mistake of this file
    wm, wn, td, th, tw = cfg[0], cfg[1], cfg[2], cfg[3], cfg[4]
    assert td * th * tw <= 64 * wm and (td + 2) * (th + 2) * (tw + 2) * 4 <= 768 * wm * wn and cs.cout % (64 * wn) == 0
    return cfg


def _mfma(cs, ver, wg=None, box=None, splitk=1, prior=None, rows=False, passes=3, bar=BAR, ref=None, tag=""):
    """One bfm_conv3x3x3_mfma_ex launch of variant `ver`, checked against float64 (or `ref`).  Returns (out, rows, n, err)."""
    L, lib = _lib()
    D, H, W = cs.dims
    cfg = _plan(cs, ver, wg, box, splitk, prior is not None)
    wp, wexp = cs.pack(PACKER[ver])
    flat, out = _out_buf(cs.dims, cs.cout, prior)
    nws = max(256, lib.bfm_conv3x3x3_mfma_workspace(cs.cin, cs.cout, D, H, W, cfg[5]))
    ws = torch.full((nws // 4,), NAN, device=_dev())
    n, rbuf = 0, None
    if rows:
        n = lib.bfm_conv3x3x3_mfma_rows(cs.cin, cs.cout, D, H, W, cfg)
        assert n > 0, "this plan must emit moment rows"
        rbuf = _rows_buf(n, cs.cout)
    rc = lib.bfm_conv3x3x3_mfma_ex(L.ptr(cs.dA), cs.ca, L.ptr(cs.dB), cs.cb, D, H, W, C.byref(cs.up) if cs.cb else None,
                                   L.ptr(cs.dscale), L.ptr(cs.dshift), L.ptr(cs.dbound), G, L.ptr(wp), wexp, cs.cout, SLOPE,
                                   passes, cfg, L.ptr(out), L.ptr(ws), ws.numel() * 4, L.ptr(rbuf), L.stream_ptr())
    label = "%s %d+%d->%d %s wg %dx%d box %s splitk %d->%d%s%s p%d%s" % (
        KERNEL[ver], cs.ca, cs.cb, cs.cout, cs.dims, cfg[0], cfg[1], (cfg[2], cfg[3], cfg[4]), cfg[5],
        _eff_splitk(cs.cin, cfg[5]), " acc" if prior is not None else "", " rows" if rows else "", passes, tag)
    assert rc == 0, (label, L.ERR.get(rc, rc))
    e = _check_out(label, flat, out, cs.ref(prior) if ref is None else ref, cs.f32, bar)
    if rows:
        _check_rows(label, rbuf, n, out)
    return out, rbuf, n, e


def _prior(cs, seed=3):
    return torch.randn(cs.dims + (cs.cout,), generator=torch.Generator().manual_seed(seed))


# --------------------------------------------------------------------------------------- a. bfm_conv3x3x3_mfma_ex
VOLUMES = [(5, 6, 19), (9, 11, 21), (2, 2, 2), (1, 1, 1), (1, 1, 33)]


@pytest.mark.parametrize("chan", [(16, 64), (48, 64), (128, 128), (48, 192)])
@pytest.mark.parametrize("ver", [0, 1, 2])
def test_mfma_variants_vs_float64_channels_and_volumes(ver, chan):
    """One K chunk, an odd chunk count, eight chunks (the planner's threshold for variant 1), three N tiles; the planner's
    box on ragged volumes, one smaller than any box, one voxel, and W past the cap of 32 on TW.  Cout = 128 runs as 2 x 2
    and as 4 x 1 waves.  splitk = 1: variant 1 runs as choose_plan produces it."""
    cin, cout = chan
    for dims in VOLUMES:
        cs = _case(dims, cin, cout)
        for wg in ((2, 2), (4, 1)) if cout % 128 == 0 else ((4, 1),):
            _mfma(cs, ver, wg=wg)


@pytest.mark.parametrize("ver", [0, 2])
def test_mfma_forced_boxes_shift_and_division_paths(ver):
    """box_coords has a shift path (TW and TH*TW powers of two) and a division path; the planner's boxes on small volumes
    rarely take the second with a multi-row box.  (9, 11, 21): no box divides it."""
    dims = (9, 11, 21)
    c41, c22 = _case(dims, 48, 64), _case(dims, 128, 128)
    _mfma(c41, ver, wg=(4, 1), box=(4, 4, 16))
    _mfma(c22, ver, wg=(2, 2), box=(4, 4, 8))
    _mfma(c41, ver, wg=(4, 1), box=(3, 5, 7))
    _mfma(c22, ver, wg=(2, 2), box=(3, 5, 7))


@pytest.mark.parametrize("ver", [0, 2])
def test_mfma_split_k_reduce_epilogues(ver):
    """Five K chunks: cfg[5] = 2 leaves a short last split (3 + 2), 4 is reduced to 3 (2 + 2 + 1), 9 is clamped to 5;
    splitk_reduce (no rows) and splitk_reduce_rows, each plain and accumulating onto a random prior."""
    cs = _case((5, 4, 5), 80, 64)
    prior = _prior(cs)
    for s, eff in ((2, 2), (4, 3), (9, 5)):
        assert _eff_splitk(80, s) == eff
        for rows in (False, True):
            for pr in (None, prior):
                _mfma(cs, ver, splitk=s, rows=rows, prior=pr)


@pytest.mark.parametrize("geom", [((5, 4, 5), (2, 2, 2)), ((6, 4, 8), (3, 2, 4))], ids=["maps2to5", "exact2x"])
@pytest.mark.parametrize("ver", [0, 2])
def test_mfma_two_sources(ver, geom):
    """The virtual concat: CA = 64 skip channels and CB = 128 nearest-upsampled ones (the non-exact 2 -> 5 maps, and the
    exact 2x case), group bounds over the concatenation.  Plain, split-K with a split that holds chunks of both sources
    (12 chunks in 4 splits of 3, the skip tensor ends after chunk 3), and accumulate mode onto a random prior."""
    dims, lo = geom
    cs = _case(dims, 64, 64, cb=128, lo=lo)
    _mfma(cs, ver)
    assert _eff_splitk(192, 5) == 4
    _mfma(cs, ver, splitk=5)
    _mfma(cs, ver, prior=_prior(cs))


MAG_DIMS, MAG_CH = (5, 6, 19), (48, 64)


@pytest.mark.parametrize("ver", [0, 1, 2])
def test_mfma_magnitudes(ver):
    """The affine-applied input scaled by 1e-6 and by 1e5 (the pre-scale exponent at +34 and -3), the eight groups'
    magnitudes spread over 1e4 under per-group bounds, and an all-zero input with zero shift: exactly 0, rows included."""
    for mag in (("mul", 1e-6), ("mul", 1e5), "spread"):
        _mfma(_case(MAG_DIMS, *MAG_CH, mag=mag), ver, rows=ver != 1, tag=" mag %s" % (mag,))
    cs = _case(MAG_DIMS, *MAG_CH, mag="zero")
    assert float(cs.bound.abs().max()) == 0.0
    out, rbuf, n, _ = _mfma(cs, ver, rows=ver != 1, tag=" zero")
    assert bool((out == 0).all())
    if rbuf is not None:
        assert bool((rbuf == 0).all())                  # sums, squares, minima and maxima: all +0.0


@pytest.mark.parametrize("ver", [0, 1, 2])
def test_mfma_one_pass_equals_hi_hi_emulation(ver):
    """passes = 1 against split_emulation(terms = 1): exact fp16 products with fp32 accumulation are the same error class
    as passes = 3, so the bar is the same 1e-5 (measured 5.3e-7, all three variants bit-equal to each other).  The hi plane is
    the one-pass kernels' own, R.affine_hi_once: their staging compiles to v_fma_mixlo_f16, which rounds the exact
    x * scale + shift to fp16 ONCE, where the three-pass kernels round it to fp32 first (they need that value for lo).
    On this case one operand of 27 360 is an fp16 tie in fp32 (1343.5 -> 1344) that the exact value is not (-> 1343): one
    such operand moves the result by 1.26e-5 of max |y|, which is what this test measured against fp16(fp32 affine), fused
    or separately rounded (both printed).  Against plain float64 the launch must sit within 3x the emulation's own
    distance (measured 1.00x)."""
    cs = _case(MAG_DIMS, *MAG_CH)
    bmax, wmax = float(cs.bound.max()), float(cs.w.abs().max())
    once = R.affine_hi_once(R.join(cs.A, cs.B, cs.maps), cs.scale, cs.shift, bmax)
    emu = R.lrelu(R.split_emulation(cs.y32, cs.w, bmax, wmax, 1, a_hi=once), SLOPE)
    fus = R.lrelu(R.split_emulation(cs.y32_fused, cs.w, bmax, wmax, 1), SLOPE)
    sep = R.lrelu(R.split_emulation(cs.y32, cs.w, bmax, wmax, 1), SLOPE)
    d_emu = R.rel_err(emu, cs.ref())
    out, _, _, e = _mfma(cs, ver, passes=1, ref=emu, tag=" vs hi*hi emulation")
    e64 = R.rel_err(out, cs.ref())
    print("%s p1: vs hi*hi emulation %.2e (hi = fp16(fp32 affine): fused %.2e, separate %.2e), vs float64 %.2e, "
          "emulation vs float64 %.2e" % (KERNEL[ver], e, R.rel_err(out, fus), R.rel_err(out, sep), e64, d_emu))
    assert e64 <= 3 * d_emu


@pytest.mark.parametrize("ver", [0, 2])
def test_mfma_moment_rows_without_split(ver):
    """The epilogue's own rows (one per M tile): both workgroup shapes, a ragged volume, plain and accumulate mode.  The
    split-K rows are checked in test_mfma_split_k_reduce_epilogues."""
    for cs, wg in ((_case((5, 6, 19), 48, 64), (4, 1)), (_case((9, 11, 21), 128, 128), (2, 2)),
                   (_case((9, 11, 21), 128, 128), (4, 1)), (_case((1, 1, 33), 16, 64), (4, 1))):
        _mfma(cs, ver, wg=wg, rows=True)
        _mfma(cs, ver, wg=wg, rows=True, prior=_prior(cs))


@pytest.mark.parametrize("splitk", [1, 2])
@pytest.mark.parametrize("ver", [0, 2])
def test_mfma_batch_per_sample_statistics(ver, splitk):
    """bfm_conv3x3x3_mfma_batch, S = 3 two-source samples with their own scale / shift / bound, the affine rows padded to
    CA + CB + 4: every sample within the bar of float64, and its output and moment rows the bits of its own S = 1 launch."""
    L, lib = _lib()
    dev = _dev()
    S, dims, lo, ca, cb, cout = 3, (5, 4, 5), (2, 2, 2), 32, 16, 64
    D, H, W = dims
    cin, pitch = ca + cb, ca + cb + 4
    css = [_case(dims, ca, cout, cb=cb, lo=lo, seed=11 + s, wseed=77) for s in range(S)]
    cfg = _plan(css[0], ver, splitk=splitk)
    wp, wexp = css[0].pack(PACKER[ver])
    A = torch.stack([c.dA for c in css]).contiguous()
    B = torch.stack([c.dB for c in css]).contiguous()
    aff = torch.full((2, S, pitch), NAN, device=dev)
    for s, c in enumerate(css):
        aff[0, s, :cin], aff[1, s, :cin] = c.dscale, c.dshift
    bound = torch.stack([c.dbound for c in css]).contiguous()
    nvo = D * H * W * cout
    flat = torch.full((S * nvo + TAIL,), SENT, device=dev)
    flat[:S * nvo] = NAN
    out = flat[:S * nvo].view((S,) + dims + (cout,))
    n = lib.bfm_conv3x3x3_mfma_rows(cin, cout, D, H, W, cfg)
    assert n > 0
    rows = _rows_buf(S * n, cout)
    ws = torch.full((max(256, lib.bfm_conv3x3x3_mfma_batch_workspace(cin, cout, S, D, H, W, splitk)) // 4,), NAN, device=dev)
    rc = lib.bfm_conv3x3x3_mfma_batch(L.ptr(A), ca, L.ptr(B), cb, S, D, H, W, C.byref(css[0].up), L.ptr(aff[0]), L.ptr(aff[1]),
                                      L.ptr(bound), G, L.ptr(wp), wexp, cout, SLOPE, 3, cfg, L.ptr(out), L.ptr(ws),
                                      ws.numel() * 4, L.ptr(rows), pitch, L.stream_ptr())
    assert rc == 0, L.ERR.get(rc, rc)
    torch.cuda.synchronize()
    assert bool((flat[S * nvo:] == SENT).all())
    k, K = n * cout, S * n * cout
    for s, c in enumerate(css):
        assert bool(torch.isfinite(out[s]).all())
        e = R.rel_err(out[s], c.ref())
        print("%s batch S=%d sample %d %d+%d->%d %s splitk %d: err %.2e, torch fp32 %.2e"
              % (KERNEL[ver], S, s, ca, cb, cout, dims, splitk, e, c.f32))
        assert e <= BAR, (s, e)
        one, r1, n1, _ = _mfma(c, ver, splitk=splitk, rows=True, tag=" (S=1 of the batch)")
        assert n1 == n and torch.equal(out[s], one), s
        for lo_, hi_, width in ((0, 8, 8), (8, 16, 8), (16, 20, 4), (20, 24, 4)):          # sums, squares, minima, maxima
            assert torch.equal(rows[K * lo_ + s * k * width: K * lo_ + (s + 1) * k * width], r1[k * lo_: k * hi_]), (s, lo_)


# --------------------------------------------------------------------------------------- b. bfm_conv3x3x3_wino_ex
def _wino(cs, prior=None, passes=3, bar=BAR, ref=None, tag="", rows=True):
    L, lib = _lib()
    D, H, W = cs.dims
    n = lib.bfm_conv3x3x3_wino_rows(D, H, W, passes)
    wp, wexp = cs.pack("wino", passes)
    flat, out = _out_buf(cs.dims, cs.cout, prior)
    rbuf = _rows_buf(n, cs.cout) if rows and n > 0 else None
    rc = lib.bfm_conv3x3x3_wino_ex(L.ptr(cs.dA), cs.ca, D, H, W, L.ptr(cs.dscale), L.ptr(cs.dshift), L.ptr(cs.dbound), G,
                                   L.ptr(wp), wexp, cs.cout, SLOPE, passes, 1 if prior is not None else 0, L.ptr(out),
                                   L.ptr(rbuf), L.stream_ptr())
    box = (C.c_int * 3)()
    lib.bfm_conv3x3x3_wino_box(D, H, W, passes, box)
    label = "conv_wino F(2,3) %d->%d %s box %s%s p%d%s" % (cs.ca, cs.cout, cs.dims, tuple(box), " acc" if prior is not None else "",
                                                          passes, tag)
    if n == 0:                                           # no box fits: refused, nothing written
        torch.cuda.synchronize()
        assert rc == E_SHAPE, (label, rc)
        assert bool(torch.isnan(out).all()) if prior is None else torch.equal(out.cpu(), prior)
        assert bool((flat[out.numel():] == SENT).all())
        return out, None, 0, None
    assert rc == 0, (label, L.ERR.get(rc, rc))
    e = _check_out(label, flat, out, cs.ref(prior) if ref is None else ref, cs.f32, bar)
    if rbuf is not None:
        _check_rows(label, rbuf, n, out)
    return out, rbuf, n, e


@pytest.mark.parametrize("case", [((8, 8, 16), 16, 64), ((9, 11, 21), 32, 64), ((12, 8, 30), 64, 128), ((5, 13, 7), 16, 64),
                                  ((17, 6, 35), 48, 192), ((2, 2, 2), 16, 64), ((1, 1, 3), 16, 64)])
def test_wino_f23_vs_float64(case):
    """The shapes of test_winograd_f43_kernel_vs_float64_convolution plus two volumes smaller than any box (an odd width: a
    pair whose second voxel is outside), plain and accumulate mode, moment rows of the stored output."""
    dims, cin, cout = case
    cs = _case(dims, cin, cout)
    _wino(cs)
    _wino(cs, prior=_prior(cs))


def test_wino_f23_magnitudes():
    for mag in (("mul", 1e-6), ("mul", 1e5), "spread"):
        _wino(_case(MAG_DIMS, *MAG_CH, mag=mag), tag=" mag %s" % (mag,))
    out, rbuf, _, _ = _wino(_case(MAG_DIMS, *MAG_CH, mag="zero"), tag=" zero")
    assert bool((out == 0).all()) and bool((rbuf == 0).all())


def test_wino_f23_one_pass_within_three_times_the_hi_hi_emulation():
    """passes = 1: the input transform sums two operands before the split and the split truncates (v_cvt_pkrtz), so the
    launch is not the emulation bit for bit; its distance to float64 must stay within 3x the emulation's own (measured
    5.45e-4 against 2.77e-4: ratio 1.97)."""
    cs = _case(MAG_DIMS, *MAG_CH)
    emu = R.lrelu(R.split_emulation(cs.y32, cs.w, float(cs.bound.max()), float(cs.w.abs().max()), 1), SLOPE)
    d_emu = R.rel_err(emu, cs.ref())
    out, _, _, _ = _wino(cs, passes=1, bar=3 * d_emu, tag=" (bar = 3x emulation)")
    print("conv_wino p1: vs float64 %.2e, emulation vs float64 %.2e, ratio %.2f"
          % (R.rel_err(out, cs.ref()), d_emu, R.rel_err(out, cs.ref()) / d_emu))


# --------------------------------------------------------------------------------------- c. bfm_conv3x3x3_direct
def _direct(cs):
    L, lib = _lib()
    D, H, W = cs.dims
    wp, _ = cs.pack("direct")
    flat, out = _out_buf(cs.dims, cs.cout)
    rc = lib.bfm_conv3x3x3_direct(L.ptr(cs.dA), cs.ca, L.ptr(cs.dB), cs.cb, D, H, W, C.byref(cs.up) if cs.cb else None,
                                  L.ptr(cs.dscale), L.ptr(cs.dshift), L.ptr(wp), cs.cout, SLOPE, L.ptr(out), L.stream_ptr())
    label = "conv_direct %d+%d->%d %s" % (cs.ca, cs.cb, cs.cout, cs.dims)
    assert rc == 0, (label, rc)
    return _check_out(label, flat, out, cs.ref(), cs.f32)


@pytest.mark.parametrize("cin", [1, 3, 5, 8, 17])
def test_direct_vs_float64(cin):
    """The exact-fp32 fallback: output tiles of 8 channels, ragged for Cout 1, 7 and 33; (3, 3, 3): every voxel on a face;
    (5, 6, 37): more than one block of 256 voxels, the last one ragged; one voxel."""
    for cout in (1, 7, 33, 64):
        for dims in ((3, 3, 3), (5, 6, 37), (1, 1, 1)):
            _direct(_case(dims, cin, cout))


@pytest.mark.parametrize("cout", [7, 33])
def test_direct_two_sources(cout):
    _direct(_case((5, 4, 5), 5, cout, cb=3, lo=(2, 2, 2)))


# --------------------------------------------------------------------------------------- d. bfm_conv3x3x3_stem_ex
@pytest.mark.parametrize("cout", [32, 64])
def test_stem_vs_float64(cout):
    """The single-channel stem of the shipped network at the shapes of test_stem_mc_kernel_against_float64 plus one voxel
    and two whole 32-voxel row blocks; scale 100, shift -20; the moment rows are the stored output's moments."""
    L, lib = _lib()
    dev = _dev()
    for i, dims in enumerate([(3, 3, 3), (5, 6, 37), (2, 1, 70), (1, 1, 1), (4, 4, 64)]):
        D, H, W = dims
        g = torch.Generator().manual_seed(100 + cout + i)
        x = torch.randn(dims + (1,), generator=g)
        w = torch.randn(cout, 1, 3, 3, 3, generator=g) / 27.0 ** 0.5
        scale = torch.tensor([100.0]) * (1.0 + 0.1 * torch.rand(1, generator=g))
        shift = torch.tensor([-20.0])
        y32 = R.affine_fp32(x, scale, shift)
        bound = y32.abs().max().reshape(1)
        ref = R.conv_ref(x, None, None, scale, shift, w, SLOPE)
        f32 = R.rel_err(R.lrelu(R._conv_cl(y32, w), SLOPE), ref)
        xd, wd, sc, sh, bd = (t.to(dev).contiguous() for t in (x, w, scale, shift, bound))
        wp = torch.empty(27 * cout, dtype=torch.float32, device=dev)
        L.check(lib.bfm_pack_conv_weights_direct(L.ptr(wd), 1, cout, L.ptr(wp), L.stream_ptr()), "pack_direct")
        flat, out = _out_buf(dims, cout)
        n = lib.bfm_conv3x3x3_stem_rows(D, H, W)
        assert n > 0
        rbuf = _rows_buf(n, cout)
        rc = lib.bfm_conv3x3x3_stem_ex(L.ptr(xd), D, H, W, L.ptr(sc), L.ptr(sh), L.ptr(bd), L.ptr(wp), cout, SLOPE, L.ptr(out),
                                       L.ptr(rbuf), L.stream_ptr())
        label = "conv_stem_mfma 1->%d %s" % (cout, dims)
        assert rc == 0, (label, rc)
        _check_out(label, flat, out, ref, f32)
        _check_rows(label, rbuf, n, out)               # waves without a row block keep +inf / -inf, which min / max ignore


# --------------------------------------------------------------------------------------- e. refusals write nothing
def test_refused_launches_return_their_code_and_write_nothing():
    """All four exports: null pointers, CA % 16, Cout % 64, passes = 2, an A that is 4 bytes off its 16-byte alignment, a
    split-K workspace that is too small, a stem width other than 32 / 64 -- the documented code comes back and the output,
    filled with 7.0, is unchanged."""
    L, lib = _lib()
    dev = _dev()
    dims, ca, cout = (4, 4, 8), 32, 64
    D, H, W = dims
    cs = _case(dims, ca, cout)
    out = torch.full(dims + (cout,), 7.0, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    skew = torch.zeros(D * H * W * ca + 4, device=dev)[1:]
    assert skew.data_ptr() % 16 == 4
    st = L.stream_ptr()
    wm, wexp = cs.pack("mfma")
    ww, wwexp = cs.pack("wino", 3)
    wd, _ = cs.pack("direct")
    p = L.ptr

    def mfma(A=cs.dA, ca_=ca, sc=cs.dscale, wp=wm, cout_=cout, passes=3, o=out, splitk=1, wsb=ws.numel()):
        cfg = _plan(cs, 0, splitk=splitk)
        return lib.bfm_conv3x3x3_mfma_ex(p(A), ca_, None, 0, D, H, W, None, p(sc), p(cs.dshift), p(cs.dbound), G, p(wp), wexp,
                                         cout_, SLOPE, passes, cfg, p(o), p(ws), wsb, None, st)

    def wino(A=cs.dA, ca_=ca, sc=cs.dscale, wp=ww, cout_=cout, passes=3, o=out, flags=0):
        return lib.bfm_conv3x3x3_wino_ex(p(A), ca_, D, H, W, p(sc), p(cs.dshift), p(cs.dbound), G, p(wp), wwexp, cout_, SLOPE,
                                         passes, flags, p(o), None, st)

    def direct(A=cs.dA, sc=cs.dscale, wp=wd, cout_=cout, o=out):
        return lib.bfm_conv3x3x3_direct(p(A), ca, None, 0, D, H, W, None, p(sc), p(cs.dshift), p(wp), cout_, SLOPE, p(o), st)

    def stem(A=cs.dA, sc=cs.dscale, wp=wd, cout_=64, o=out, bd=cs.dbound):
        return lib.bfm_conv3x3x3_stem_ex(p(A), D, H, W, p(sc), p(cs.dshift), p(bd), p(wp), cout_, SLOPE, p(o), None, st)

    for fn in (mfma, wino, direct, stem):
        for null in ("A", "sc", "wp", "o"):
            assert fn(**{null: None}) == E_ARG, (fn.__name__, null)
    assert stem(bd=None) == E_ARG
    for fn in (mfma, wino):
        assert fn(ca_=24) == E_SHAPE and fn(ca_=8) == E_SHAPE, fn.__name__
        assert fn(cout_=48) == E_SHAPE and fn(cout_=96) == E_SHAPE, fn.__name__
        assert fn(passes=2) == E_ARG, fn.__name__
        assert fn(A=skew) == E_ARG, fn.__name__
    assert wino(flags=2) == E_ARG
    assert mfma(splitk=2, wsb=2 * D * H * W * cout * 4 - 4) == E_WORKSPACE
    assert mfma(splitk=2, wsb=0) == E_WORKSPACE
    assert direct(cout_=0) == E_ARG
    assert stem(cout_=48) == E_SHAPE and stem(cout_=16) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
