"""Float64 references for the conditioned stem's backward (bfm_stem_mc_bwd) and the condition inputs
(bfm_condition_input), shared by tests/test_host_condtrain.py (which checks them against torch autograd and the torch
expressions) and tests/test_gpu_condtrain.py.  Closed forms on shifted slices: no autograd, no conv3d."""
import numpy as np
import torch

MODES = {"mask": 0, "flip": 1, "mask+flip": 2}


def group_stats(x, eps=1e-5):
    """mean, rstd of GroupNorm(1, Cin) over a channels-last (D,H,W,Cin) tensor, float64."""
    x = x.double()
    mean = x.mean()
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean() + eps)
    return mean, rstd


def stem_bwd_ref(dP, x, w, gamma, beta, eps=1e-5):
    """dP (D,H,W,Cout): gradient after the LeakyReLU; x (D,H,W,Cin): the layer's raw input; w (Cout,Cin,3,3,3).
    Returns float64 dW (Cout,Cin,3,3,3), dgamma (Cin), dbeta (Cin) of  conv3d(group_norm(x, 1, gamma, beta), w, padding=1)."""
    dP, x, w, gamma, beta = (t.double() for t in (dP, x, w, gamma, beta))
    D, H, W, cin = x.shape
    cout = dP.shape[-1]
    mean, rstd = group_stats(x, eps)
    xhat = (x - mean) * rstd
    xn = torch.zeros((D + 2, H + 2, W + 2, cin), dtype=torch.float64)
    xn[1:-1, 1:-1, 1:-1] = xhat * gamma + beta
    dPp = torch.zeros((D + 2, H + 2, W + 2, cout), dtype=torch.float64)
    dPp[1:-1, 1:-1, 1:-1] = dP
    dW = torch.zeros((cout, cin, 3, 3, 3), dtype=torch.float64)
    dXn = torch.zeros((D, H, W, cin), dtype=torch.float64)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                # out[v] += w[.,.,k] xn[v + k - 1]  =>  dW[k] = sum_v dP[v] xn[v + k - 1],  dXn[u] += dP[u - k + 1] w[k]
                dW[:, :, kd, kh, kw] = torch.einsum("dhwo,dhwc->oc", dP, xn[kd:kd + D, kh:kh + H, kw:kw + W])
                dXn += torch.einsum("dhwo,oc->dhwc", dPp[2 - kd:2 - kd + D, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W],
                                    w[:, :, kd, kh, kw])
    return dW, (dXn * xhat).sum(dim=(0, 1, 2)), dXn.sum(dim=(0, 1, 2))


def stem_bwd_autograd(dP, x, w, gamma, beta, eps=1e-5):
    """The same three gradients from torch float64 autograd of group_norm -> conv3d."""
    import torch.nn.functional as F
    x5 = x.double().permute(3, 0, 1, 2).unsqueeze(0)
    w, gamma, beta = (t.double().clone().requires_grad_(True) for t in (w, gamma, beta))
    y = F.conv3d(F.group_norm(x5, 1, gamma, beta, eps), w, padding=1)
    y.backward(dP.double().permute(3, 0, 1, 2).unsqueeze(0))
    return w.grad, gamma.grad, beta.grad


def condition_ref(x, p, condition):
    """The torch expressions of the reference's training loop for one (1,1,D,H,W) sample (in x's dtype): returns the
    channels-last network input (D,H,W,Cin) = image, flipped image, mask; the image as left in the sample; its flip
    (or None).  Masking multiplies by 1 - p in place, the flip is along the first spatial axis."""
    x = x.clone()
    chans, flipped = [], None
    names = condition.split("+")
    if "mask" in names:
        x *= 1 - p
        chans.append(p.to(x.dtype))
    if "flip" in names:
        flipped = torch.flip(x, dims=[2])
        chans.insert(0, flipped)
    full = torch.concat([x] + chans, dim=1)
    return full[0].permute(1, 2, 3, 0).contiguous(), x, flipped


def rel_err(a, b):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))
