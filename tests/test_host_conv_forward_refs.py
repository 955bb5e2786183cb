"""The float64 references of tests/conv_forward_refs.py pinned on the CPU: conv_ref against torch's float64 conv3d of
the materialised concat, and the split emulation against conv_ref -- three terms sit at fp32 rounding, one term or a
dropped lo term sits above 1e-4 of max |y|, which is what lets the 1e-5 bar of tests/test_gpu_conv_forward.py see a lost
pass.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import conv_forward_refs as R

SLOPE = 0.01
# (dims, CA, CB, lo dims, Cout): the deep split-K decoder shape with its non-exact 2 -> 5 maps, a mid level, a shallow one
CASES = [((5, 4, 5), 256, 512, (2, 2, 2), 256), ((9, 11, 21), 256, 0, None, 128), ((5, 6, 19), 16, 0, None, 64)]


def _operands(dims, ca, cb, lo, cout):
    g = torch.Generator().manual_seed(ca + cb + dims[2])
    A = torch.randn(dims + (ca,), generator=g) * 1.7 + 0.2
    B = torch.randn(lo + (cb,), generator=g) * 0.8 - 0.1 if cb else None
    cin = ca + cb
    scale = torch.rand(cin, generator=g) + 0.5
    shift = torch.randn(cin, generator=g) * 0.3
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.05
    maps = R.up_maps(lo, dims) if cb else None
    return A, B, maps, scale, shift, w


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%dx%dx%d_%d+%d_%d" % (c[0] + (c[1], c[2], c[4])))
def case(request):
    dims, ca, cb, lo, cout = request.param
    A, B, maps, scale, shift, w = _operands(dims, ca, cb, lo, cout)
    ref = R.conv_ref(A, B, maps, scale, shift, w, SLOPE)
    y32 = R.affine_fp32(R.join(A, B, maps), scale, shift)
    return dict(dims=dims, A=A, B=B, maps=maps, scale=scale, shift=shift, w=w, ref=ref, y32=y32, lo=lo)


def test_conv_ref_equals_torch_float64_conv_of_the_materialised_concat(case):
    """Built a second way: NCDHW, F.interpolate(mode='nearest'), torch.cat, F.pad of the affine output, an unpadded conv."""
    c = case
    x = c["A"].double().permute(3, 0, 1, 2)[None]
    if c["B"] is not None:
        up = F.interpolate(c["B"].double().permute(3, 0, 1, 2)[None], size=c["dims"], mode="nearest")
        x = torch.cat((x, up), 1)
    x = x * c["scale"].double().view(1, -1, 1, 1, 1) + c["shift"].double().view(1, -1, 1, 1, 1)
    want = F.leaky_relu(F.conv3d(F.pad(x, (1,) * 6), c["w"].double()), SLOPE)[0].permute(1, 2, 3, 0)
    assert R.rel_err(c["ref"], want) <= 1e-13
    # the shift is not zero, so padding before the affine is a different function: the reference must not be that one
    wrong = F.leaky_relu(F.conv3d(F.pad(x - c["shift"].double().view(1, -1, 1, 1, 1), (1,) * 6) +
                                  c["shift"].double().view(1, -1, 1, 1, 1), c["w"].double()), SLOPE)[0].permute(1, 2, 3, 0)
    assert R.rel_err(wrong, want) > 1e-3


def test_conv_ref_prior_and_slope(case):
    c = case
    g = torch.Generator().manual_seed(5)
    prior = torch.randn(c["ref"].shape, generator=g)
    pre = R.conv_ref(c["A"], c["B"], c["maps"], c["scale"], c["shift"], c["w"], 1.0)          # slope 1: the conv itself
    got = R.conv_ref(c["A"], c["B"], c["maps"], c["scale"], c["shift"], c["w"], 0.25, prior=prior)
    want = F.leaky_relu(pre + prior.double(), 0.25)
    assert R.rel_err(got, want) <= 1e-14
    assert bool((got < 0).any()) and bool((got > 0).any())


def test_three_terms_sit_at_fp32_rounding_and_a_lost_term_above_the_kernel_bar(case):
    c = case
    bmax, wmax = float(c["y32"].abs().max()), float(c["w"].abs().max())
    err = {}
    for terms in (3, 1, ("hh", "hl"), ("hh", "lh")):
        err[terms] = R.rel_err(R.lrelu(R.split_emulation(c["y32"], c["w"], bmax, wmax, terms), SLOPE), c["ref"])
    f32 = R.rel_err(R.lrelu(R._conv_cl(c["y32"], c["w"].float()), SLOPE), c["ref"])
    print("split emulation %s: 3 terms %.2e, torch fp32 %.2e, hi*hi %.2e, no lh %.2e, no hl %.2e"
          % (c["dims"], err[3], f32, err[1], err[("hh", "hl")], err[("hh", "lh")]))
    assert err[3] <= 5e-7
    assert f32 <= 2e-6
    for terms in (1, ("hh", "hl"), ("hh", "lh")):
        assert err[terms] > 1e-4, terms


def test_prescale_and_split_follow_the_header():
    """14 - frexp exponent, clamped; hi is round-to-nearest-even fp16; hi + lo restores 21-22 bits."""
    assert R.prescale_exp(1.0) == 13 and R.prescale_exp(0.99) == 14 and R.prescale_exp(3.0) == 12
    assert R.prescale_exp(0.0) == 0 and R.prescale_exp(float("inf")) == 0 and R.prescale_exp(float("nan")) == 0
    assert R.prescale_exp(1e-30) == 60 and R.prescale_exp(1e30) == -60
    v = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 0.3333333])
    hi, lo = R.split_hi_lo(v, 0)
    assert hi.tolist()[:3] == [1.0, 1.0 + 2.0 ** -9, -1.0]              # ties go to the even mantissa
    assert float(((hi + lo) - v.double()).abs().max()) <= 2.0 ** -22
    # the largest operand the bound admits lands below 2^14 after the pre-scale: nothing overflows fp16
    for b in (0.7, 1.0, 5.3, 1e-6, 1e5):
        assert 2.0 ** 13 <= b * 2.0 ** R.prescale_exp(b) < 2.0 ** 14


def test_fused_affine_is_one_rounding_and_differs_by_the_product_rounding_alone(case):
    """affine_fp32(fused=True) is the correctly rounded x * scale + shift (the kernels' fmaf): never further from the
    float64 value than the two-rounding form, different from it in some elements, and never by more than the roundings of
    the product and of the sum.  With three terms the two operands give the same convolution to fp32 rounding; with hi*hi
    alone an ulp can land on the other fp16 neighbour (up to 1.1e-5 of max |y| here), so a one-pass kernel is compared with
    the emulation of ITS affine."""
    c = case
    X = R.join(c["A"], c["B"], c["maps"])
    sep, fus = c["y32"], R.affine_fp32(X, c["scale"], c["shift"], fused=True)
    exact = X.double() * c["scale"].double() + c["shift"].double()
    assert bool(((fus.double() - exact).abs() <= (sep.double() - exact).abs()).all())
    assert 0 < int((sep != fus).sum()) < sep.numel() // 2
    two_roundings = ((X * c["scale"]).abs() + sep.abs()).double() * 2.0 ** -24 * 1.0001
    assert bool(((sep.double() - fus.double()).abs() <= two_roundings + (fus.double() - exact).abs()).all())
    bmax, wmax = float(sep.abs().max()), float(c["w"].abs().max())
    d3 = R.rel_err(R.split_emulation(fus, c["w"], bmax, wmax, 3), R.split_emulation(sep, c["w"], bmax, wmax, 3))
    d1 = R.rel_err(R.split_emulation(fus, c["w"], bmax, wmax, 1), R.split_emulation(sep, c["w"], bmax, wmax, 1))
    print("fused vs separate affine %s: three terms %.2e, hi*hi %.2e" % (c["dims"], d3, d1))
    assert d3 <= 2e-7


def test_hi_rounded_once_differs_from_hi_rounded_twice_on_fp16_ties_only(case):
    """affine_hi_once (the passes = 1 kernels: v_fma_mixlo_f16) against fp16(fused fp32 affine) (the passes = 3 kernels,
    which keep the fp32 value for the lo plane): equal except where the fp32 value sits exactly between two fp16 values,
    and there one fp16 ulp apart.  A built example: 1 + 3 * 2^-11 - 2^-30 rounds to the tie 1 + 3 * 2^-11 in fp32 and
    from there to the even 1 + 2^-9, but to 1 + 2^-10 at once."""
    x = torch.tensor([1.0 + 3 * 2.0 ** -11])
    one, off = torch.ones(1), torch.tensor([-2.0 ** -30])
    assert float(R.affine_fp32(x, one, off, fused=True)) == 1.0 + 3 * 2.0 ** -11
    assert float(R.split_hi_lo(R.affine_fp32(x, one, off, fused=True), 13)[0]) == (1.0 + 2.0 ** -9) * 2.0 ** 13
    assert float(R.affine_hi_once(x, one, off, 1.0)) == (1.0 + 2.0 ** -10) * 2.0 ** 13
    c = case
    X = R.join(c["A"], c["B"], c["maps"])
    bmax = float(c["y32"].abs().max())
    aexp = R.prescale_exp(bmax)
    fus = R.affine_fp32(X, c["scale"], c["shift"], fused=True)
    twice = R.split_hi_lo(fus, aexp)[0]
    once = R.affine_hi_once(X, c["scale"], c["shift"], bmax)
    diff = once != twice
    t = fus.double() * 2.0 ** aexp
    assert int(diff.sum()) < 1e-3 * diff.numel()
    assert bool((t[diff] == 0.5 * (once[diff] + twice[diff])).all())        # the fp32 value is the midpoint of the two
    assert bool(((once - twice).abs()[diff] <= 2.0 ** -10 * twice.abs()[diff]).all())


def test_group_bound_is_per_group():
    Y = torch.zeros(2, 2, 2, 16)
    Y[0, 0, 0, 3] = -5.0
    Y[1, 1, 1, 15] = 2.0
    assert R.group_bound(Y, 8).tolist() == [0.0, 5.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0]
