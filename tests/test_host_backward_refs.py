"""The float64 references of tests/backward_refs.py against torch's own float64 autograd on the CPU, each built a second,
independent way (NCDHW tensors, F.interpolate, the nn modules, max_pool3d): what tests/test_gpu_backward.py holds the
HIP kernels to is itself held to torch here, without a GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backward_refs as R

SLOPE = 0.01


def _ncdhw(t):
    return t.permute(3, 0, 1, 2)[None]


def _cl(t):
    return t[0].permute(1, 2, 3, 0)


@pytest.mark.parametrize("kind", ["ties", "zeros", "distinct"])
@pytest.mark.parametrize("dims", [(2, 2, 2), (3, 3, 3), (4, 5, 6), (5, 4, 7), (7, 6, 3)])
def test_maxpool2_bwd_ref_equals_torch_bitwise(dims, kind):
    """First-maximum routing is what torch's CPU max_pool3d backward does, ties and constants included: bit for bit."""
    gen = torch.Generator().manual_seed(sum(dims))
    for c in (3, 4):
        x = R.pool_input(kind, dims, c, gen).double()
        dOut = torch.randn((dims[0] // 2, dims[1] // 2, dims[2] // 2, c), generator=gen, dtype=torch.float64)
        xt = _ncdhw(x).clone().requires_grad_(True)
        (F.max_pool3d(xt, 2) * _ncdhw(dOut)).sum().backward()
        ref = R.maxpool2_bwd_ref(x, dOut)
        assert torch.equal(ref, _cl(xt.grad)), (dims, kind, c)
        assert int((ref != 0).sum()) <= dOut.numel()


@pytest.mark.parametrize("ca,cb,groups,dims,lo", [(6, 0, 2, (3, 5, 9), None), (32, 64, 8, (7, 9, 11), (3, 4, 5))])
def test_gn_bwd_ref_vs_torch_modules_and_closed_form(ca, cb, groups, dims, lo):
    """gn_bwd_ref (index maps of the engine, channels-last) against autograd through F.interpolate(mode='nearest') +
    nn.GroupNorm on NCDHW tensors, and against the closed form the kernel restates:
    dx = rstd (gamma dXn - m1 - xhat m2), a low-res voxel summing over its replicas."""
    gen = torch.Generator().manual_seed(ca + cb)
    A = torch.randn(dims + (ca,), generator=gen, dtype=torch.float64) * 1.5 + 30.0
    B = torch.randn(lo + (cb,), generator=gen, dtype=torch.float64) if cb else None
    gamma = torch.rand(ca + cb, generator=gen, dtype=torch.float64) + 0.5
    dXn = torch.randn(dims + (ca + cb,), generator=gen, dtype=torch.float64)
    maps = R.up_maps(lo, dims) if cb else None
    ref = R.gn_bwd_ref(A, B, maps, gamma, groups, dXn)
    # (1) torch's modules
    a = _ncdhw(A).clone().requires_grad_(True)
    b = _ncdhw(B).clone().requires_grad_(True) if cb else None
    gn = torch.nn.GroupNorm(groups, ca + cb, eps=R.GN_EPS).double()
    with torch.no_grad():
        gn.weight.copy_(gamma)
    x = a if b is None else torch.cat([a, F.interpolate(b, size=dims, mode="nearest")], dim=1)
    (gn(x) * _ncdhw(dXn)).sum().backward()
    assert R.rel_err(ref["dA"], _cl(a.grad)) <= 1e-12
    assert R.rel_err(ref["dgamma"], gn.weight.grad) <= 1e-12
    assert R.rel_err(ref["dbeta"], gn.bias.grad) <= 1e-12
    if cb:
        assert R.rel_err(ref["dB"], _cl(b.grad)) <= 1e-12
    # (2) the closed form, and the statistics that the kernel is handed
    X = R.join(A, B, maps)
    cpg = (ca + cb) // groups
    mean, rstd = ref["mean"].repeat_interleave(cpg), ref["rstd"].repeat_interleave(cpg)
    xg = X.reshape(-1, groups, cpg)
    assert torch.allclose(ref["mean"], xg.mean(dim=(0, 2)), rtol=1e-13, atol=0)
    assert torch.allclose(ref["rstd"], (xg.var(dim=(0, 2), unbiased=False) + R.GN_EPS).rsqrt(), rtol=1e-13, atol=0)
    xh = (X - mean) * rstd
    gd = gamma * dXn
    m1 = gd.reshape(-1, groups, cpg).mean(dim=(0, 2)).repeat_interleave(cpg)
    m2 = (gd * xh).reshape(-1, groups, cpg).mean(dim=(0, 2)).repeat_interleave(cpg)
    dX = rstd * (gd - m1 - xh * m2)
    assert R.rel_err(dX[..., :ca], ref["dA"]) <= 1e-10
    assert R.rel_err((dXn * xh).sum(dim=(0, 1, 2)), ref["dgamma"]) <= 1e-10
    assert R.rel_err(dXn.sum(dim=(0, 1, 2)), ref["dbeta"]) <= 1e-12
    if cb:
        dB = torch.zeros_like(B)
        zz, yy, xx = torch.meshgrid(*maps, indexing="ij")
        dB.index_put_((zz, yy, xx), dX[..., ca:], accumulate=True)
        assert R.rel_err(dB, ref["dB"]) <= 1e-10


@pytest.mark.parametrize("ca,cb,cout,dims,lo", [(64, 0, 64, (1, 2, 3), None), (8, 8, 16, (5, 7, 9), (2, 3, 4))])
def test_wgrad_ref_vs_conv3d_autograd(ca, cb, cout, dims, lo):
    """The 27-tap correlation equals d/dW of sum(conv3d(X, W, padding=1) * dP)."""
    gen = torch.Generator().manual_seed(cout)
    A = torch.randn(dims + (ca,), generator=gen, dtype=torch.float64)
    B = torch.randn(lo + (cb,), generator=gen, dtype=torch.float64) if cb else None
    scale = torch.rand(ca + cb, generator=gen, dtype=torch.float64) + 0.5
    shift = torch.randn(ca + cb, generator=gen, dtype=torch.float64) * 0.1
    X = R.join(A, B, R.up_maps(lo, dims) if cb else None) * scale + shift
    dP = torch.randn(dims + (cout,), generator=gen, dtype=torch.float64)
    w = torch.zeros((cout, ca + cb, 3, 3, 3), dtype=torch.float64, requires_grad=True)
    (F.conv3d(_ncdhw(X), w, None, padding=1) * _ncdhw(dP)).sum().backward()
    assert R.rel_err(R.wgrad_ref(X, dP), w.grad.reshape(cout, ca + cb, 27)) <= 1e-13


@pytest.mark.parametrize("ca,cb,cout,groups,dims,lo", [(1, 0, 32, 1, (6, 7, 9), None),
                                                       (64, 128, 64, 8, (7, 9, 11), (3, 4, 5))])
def test_single_conv_ref_vs_torch_modules(ca, cb, cout, groups, dims, lo):
    """single_conv_ref against nn.GroupNorm -> nn.Conv3d -> nn.LeakyReLU on NCDHW tensors (forward and all five
    gradients), against the oracle's forward, and the mask argument: the layer's own sign reproduces the layer, another
    mask is used as given and takes no gradient."""
    from oracle import unet_ref as O
    gen = torch.Generator().manual_seed(cout + ca)
    cin = ca + cb

    def rnd(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64)
    A = rnd(*dims, ca) * 1.5 + 1.0
    B = rnd(*lo, cb) if cb else None
    gamma, beta = 1.0 + 0.2 * rnd(cin), 0.1 * rnd(cin)
    w = rnd(cout, cin, 3, 3, 3) / np.sqrt(27.0 * cin)
    dY = rnd(*dims, cout)
    maps = R.up_maps(lo, dims) if cb else None
    ref = R.single_conv_ref(A, B, maps, gamma, beta, w, groups, SLOPE, dY=dY)
    a = _ncdhw(A).clone().requires_grad_(True)
    b = _ncdhw(B).clone().requires_grad_(True) if cb else None
    gn = torch.nn.GroupNorm(groups, cin, eps=R.GN_EPS).double()
    conv = torch.nn.Conv3d(cin, cout, 3, padding=1, bias=False).double()
    with torch.no_grad():
        gn.weight.copy_(gamma)
        gn.bias.copy_(beta)
        conv.weight.copy_(w)
    x = a if b is None else torch.cat([a, F.interpolate(b, size=dims, mode="nearest")], dim=1)
    y = torch.nn.LeakyReLU(SLOPE)(conv(gn(x)))
    (y * _ncdhw(dY)).sum().backward()
    assert R.rel_err(ref["out"], _cl(y)) <= 1e-13
    assert R.rel_err(ref["dA"], _cl(a.grad)) <= 1e-12
    assert R.rel_err(ref["dW"], conv.weight.grad.reshape(cout, cin, 27)) <= 1e-12
    assert R.rel_err(ref["dgamma"], gn.weight.grad) <= 1e-12
    assert R.rel_err(ref["dbeta"], gn.bias.grad) <= 1e-12
    if cb:
        assert R.rel_err(ref["dB"], _cl(b.grad)) <= 1e-12
    else:
        sd = {"p.groupnorm.weight": gamma, "p.groupnorm.bias": beta, "p.conv.weight": w}
        assert R.rel_err(ref["out"], _cl(O.single_conv(_ncdhw(A), sd, "p", num_groups=8))) <= 1e-13
    # the mask is a constant: the layer's own sign gives the same numbers, a flipped element changes exactly itself
    mask = ref["out"] > 0
    same = R.single_conv_ref(A, B, maps, gamma, beta, w, groups, SLOPE, mask=mask, dY=dY)
    for k in ("out", "dA", "dW", "dgamma", "dbeta"):
        assert torch.equal(same[k], ref[k]), k
    flipped = mask.clone()
    flipped[0, 0, 0, 0] = not bool(mask[0, 0, 0, 0])
    other = R.single_conv_ref(A, B, maps, gamma, beta, w, groups, SLOPE, mask=flipped)
    diff = other["out"] != ref["out"]
    assert int(diff.sum()) == 1 and bool(diff[0, 0, 0, 0])
    # float32 arguments give a float32 evaluation: the yardstick of the GPU test
    f32 = R.single_conv_ref(A.float(), B.float() if cb else None, maps, gamma.float(), beta.float(), w.float(), groups,
                            SLOPE, mask=mask, dY=dY.float())
    assert f32["dW"].dtype == torch.float32 and 0 < R.rel_err(f32["dW"], ref["dW"]) <= 1e-4
