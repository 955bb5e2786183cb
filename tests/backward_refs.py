"""Float64 references of the backward-pass kernels (brainfm_amd/csrc/backward.hip), written from the definitions.

Plain helpers, no test in here: tests/test_host_backward_refs.py proves each one against torch's float64 autograd on
the CPU, tests/test_gpu_backward.py compares the HIP kernels with them.  Tensors are channels-last, (D, H, W, C), as
the kernels see them; weights and their gradients are (Cout, Cin, 27) with tap = (kd * 3 + kh) * 3 + kw.  Every
function computes in the dtype and on the device of what it is handed (float64 for a reference; the float32 run of
single_conv_ref is the yardstick of the SingleConv test).
"""
import torch
import torch.nn.functional as F

from brainfm_amd.engine import nearest_index_map

GN_EPS = 1e-5


def rel_err(got, ref):
    """max |got - ref| / max |ref| in float64 (0 / 0 counts as 0)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    den = float(ref.abs().max())
    err = float((got - ref).abs().max())
    return err / den if den > 0 else err


def up_maps(lo_dims, dims, device="cpu"):
    """The three nearest-neighbour index maps (int64 tensors) of lo_dims -> dims, from engine.nearest_index_map."""
    return [torch.from_numpy(nearest_index_map(lo_dims[a], dims[a])).long().to(device) for a in range(3)]


def join(A, B=None, maps=None):
    """cat(A, B[mapD][:, mapH][:, :, mapW]) over the channels: the input of a SingleConv (B: the low-res tensor or None)."""
    if B is None:
        return A
    return torch.cat([A, B[maps[0]][:, maps[1]][:, :, maps[2]]], dim=-1)


def pool_input(kind, dims, c, gen):
    """The three input kinds of the MaxPool3d tests: many ties, one constant, no ties."""
    if kind == "ties":
        return torch.randint(0, 3, dims + (c,), generator=gen).float()
    if kind == "zeros":
        return torch.zeros(dims + (c,))
    assert kind == "distinct"
    return torch.randperm(dims[0] * dims[1] * dims[2] * c, generator=gen).float().reshape(dims + (c,)) - 7.0


def maxpool2_bwd_ref(inp, dOut):
    """MaxPool3d(2) backward: dOut (d, h, w, C) goes to the first maximum of each 2x2x2 window of inp (D, H, W, C) in
    (z, y, x) scan order, zeros elsewhere (odd trailing slices included).  float64."""
    D, H, W, Cn = inp.shape
    d, h, w = D // 2, H // 2, W // 2
    assert tuple(dOut.shape) == (d, h, w, Cn)
    x = inp.double()
    win = [x[dz:2 * d:2, dy:2 * h:2, dx:2 * w:2] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    best = win[0].clone()
    idx = torch.zeros(best.shape, dtype=torch.int64, device=inp.device)
    for k in range(1, 8):
        later = win[k] > best                              # strictly larger: of equal values the first one stays
        best = torch.where(later, win[k], best)
        idx = torch.where(later, torch.full_like(idx, k), idx)
    dIn = torch.zeros((D, H, W, Cn), dtype=torch.float64, device=inp.device)
    g = dOut.double()
    k = 0
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                dIn[dz:2 * d:2, dy:2 * h:2, dx:2 * w:2] = torch.where(idx == k, g, torch.zeros_like(g))
                k += 1
    return dIn


def group_stats(X, groups, eps=GN_EPS):
    """Per-group mean and 1 / sqrt(biased variance + eps) of X (D, H, W, C), in X's dtype."""
    Cn = X.shape[-1]
    xg = X.reshape(-1, groups, Cn // groups)
    mean = xg.mean(dim=(0, 2))
    var = ((xg - mean[None, :, None]) ** 2).mean(dim=(0, 2))
    return mean, 1.0 / torch.sqrt(var + eps)


def _group_norm_cl(X, gamma, beta, groups, eps):
    """F.group_norm of a channels-last (D, H, W, C) tensor, channels-last out."""
    return F.group_norm(X.permute(3, 0, 1, 2)[None], groups, gamma, beta, eps)[0].permute(1, 2, 3, 0)


def gn_bwd_ref(A, B, maps, gamma, groups, dXn, eps=GN_EPS):
    """GroupNorm backward of y = group_norm(cat(A, up(B))): autograd of sum(y * dXn) in float64.
    Returns dict(dA, dB (None without B), dgamma, dbeta, mean, rstd); mean / rstd are the float64 group statistics."""
    a = A.double().detach().clone().requires_grad_(True)
    b = None if B is None else B.double().detach().clone().requires_grad_(True)
    ga = gamma.double().detach().clone().requires_grad_(True)
    be = torch.zeros_like(ga).requires_grad_(True)
    X = join(a, b, maps)
    y = _group_norm_cl(X, ga, be, groups, eps)
    (y * dXn.double()).sum().backward()
    mean, rstd = group_stats(X.detach(), groups, eps)
    return dict(dA=a.grad, dB=None if b is None else b.grad, dgamma=ga.grad, dbeta=be.grad, mean=mean, rstd=rstd)


def wgrad_ref(X, dP):
    """dW[co][ci][tap] = sum_v dP[v][co] * X[v + tap - 1][ci] with X (D, H, W, Cin) zero outside the volume: the 27-tap
    correlation of the (GroupNorm-applied) conv input with the gradient of the conv output, float64, (Cout, Cin, 27)."""
    D, H, W, cin = X.shape
    cout = dP.shape[-1]
    Xp = F.pad(X.double().permute(3, 0, 1, 2)[None], (1, 1, 1, 1, 1, 1))[0]
    d64 = dP.double().reshape(-1, cout)
    ref = torch.empty((cout, cin, 27), dtype=torch.float64, device=X.device)
    for t in range(27):
        kd, kh, kw = t // 9, (t // 3) % 3, t % 3
        ref[:, :, t] = (Xp[:, kd:kd + D, kh:kh + H, kw:kw + W].reshape(cin, -1) @ d64).t()
    return ref


def single_conv_ref(A, B, maps, gamma, beta, weight, groups, slope, mask=None, dY=None, eps=GN_EPS):
    """One SingleConv 'gcl': GroupNorm(eps) -> conv3d(padding=1, no bias) -> LeakyReLU, in the dtype of its arguments.
    weight: (Cout, Cin, 3, 3, 3).  mask: boolean (D, H, W, Cout), True where LeakyReLU passes the value unchanged; it is a
    CONSTANT of the graph (None: the sign of the pre-activation itself, the real layer).  With dY (D, H, W, Cout) the
    gradients of sum(out * dY) come back too.  Returns dict(out, xn (GroupNorm output), pre (conv output)[, dA, dB,
    dW (Cout, Cin, 27), dgamma, dbeta])."""
    leaves = [t.detach().clone().requires_grad_(dY is not None) if t is not None else None
              for t in (A, B, gamma, beta, weight)]
    a, b, ga, be, w = leaves
    xn = _group_norm_cl(join(a, b, maps), ga, be, groups, eps)
    p = F.conv3d(xn.permute(3, 0, 1, 2)[None], w, None, padding=1)[0].permute(1, 2, 3, 0)
    if mask is None:
        mask = p.detach() > 0
    out = p * torch.where(mask, torch.ones((), dtype=p.dtype, device=p.device),
                          torch.full((), slope, dtype=p.dtype, device=p.device))
    res = dict(out=out.detach(), xn=xn.detach(), pre=p.detach())
    if dY is not None:
        (out * dY).sum().backward()
        res.update(dA=a.grad, dB=None if b is None else b.grad, dW=w.grad.reshape(w.shape[0], w.shape[1], 27),
                   dgamma=ga.grad, dbeta=be.grad)
    return res
