"""Float64 references for the joint two-stage training step: the input gradient of the multi-channel stem with respect to
one channel (bfm_stem_mc_dgrad), its chain through the masking into the stage-0 logit (bfm_mask_chain_bwd) and the stage-1
training input (bfm_twostage_train_input).  Shared by tests/test_host_twostage_train.py (which checks them against torch
autograd) and tests/test_gpu_twostage_train.py.  Closed forms on shifted slices: no autograd, no conv3d."""
import numpy as np
import torch

import stem_bwd_refs as SR


def channel_G(dP, w, channel):
    """G_c[u] = sum_{o,k} dP[u - k + 1, o] W[o, c, k], zero outside the volume.  dP (D,H,W,Cout), w (Cout,Cin,3,3,3)."""
    dP, w = dP.double(), w.double()
    D, H, W, cout = dP.shape
    dPp = torch.zeros((D + 2, H + 2, W + 2, cout), dtype=torch.float64)
    dPp[1:-1, 1:-1, 1:-1] = dP
    G = torch.zeros((D, H, W), dtype=torch.float64)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                G += torch.einsum("dhwo,o->dhw", dPp[2 - kd:2 - kd + D, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W],
                                  w[:, channel, kd, kh, kw])
    return G


def stem_dgrad_ref(dP, x_cl, w, gamma, channel, dgamma=None, dbeta=None, eps=1e-5):
    """dX_c (D,H,W) float64 of conv3d(group_norm(x, 1, gamma, beta), w, padding=1) for the channels-last input x_cl
    (D,H,W,Cin):  dX_c = rstd (gamma_c G_c - m1 - xhat_c m2),  m1 = sum gamma dbeta / N,  m2 = sum gamma dgamma / N.
    dgamma / dbeta: the layer's parameter gradients (default: the float64 ones of stem_bwd_refs.stem_bwd_ref)."""
    x = x_cl.double()
    gamma = gamma.double()
    if dgamma is None or dbeta is None:
        _, dgamma, dbeta = SR.stem_bwd_ref(dP, x, w, gamma, torch.zeros_like(gamma), eps)
    mean, rstd = SR.group_stats(x, eps)
    xhat = (x[..., channel] - mean) * rstd
    n = float(x.numel())
    m1 = float((gamma * dbeta.double()).sum()) / n
    m2 = float((gamma * dgamma.double()).sum()) / n
    return rstd * (gamma[channel] * channel_G(dP, w, channel) - m1 - xhat * m2)


def mask_chain_ref(dx, x_raw, p):
    """The increment of dRaw: d/d(raw) of x_raw (1 - sigmoid(raw)) against dx, with p = sigmoid(raw)."""
    dx, x_raw, p = dx.double(), x_raw.double(), p.double()
    return -x_raw * dx * p * (1.0 - p)


def chain_autograd(dP, x_raw, r, others, w, gamma, beta, channel, eps=1e-5):
    """d/dr of <dP, conv3d(group_norm(cat(...), 1, gamma, beta), w, padding=1)> by torch float64 autograd, where the
    input's channel `channel` is x_raw (1 - sigmoid(r)) and the other channels are `others` (D,H,W,Cin-1), in order."""
    import torch.nn.functional as F
    r = r.double().clone().requires_grad_(True)
    masked = x_raw.double() * (1 - torch.sigmoid(r))
    chans = [others[..., j].double() for j in range(others.shape[-1])]
    chans.insert(channel, masked)
    x5 = torch.stack(chans, dim=0).unsqueeze(0)
    y = F.conv3d(F.group_norm(x5, 1, gamma.double(), beta.double(), eps), w.double(), padding=1)
    y.backward(dP.double().permute(3, 0, 1, 2).unsqueeze(0))
    return r.grad, x5[0].permute(1, 2, 3, 0).detach()


def sigmoid64(raw):
    return torch.sigmoid(raw.double())


def train_input_ref(x, p, t):
    """torch's expressions of Trainer/engine.py:238 and the joiner's concat, in the dtype of x: ({x (1 - p), t} channels-last
    (n, 2), x (1 - p)).  t None: a zero mask."""
    masked = x * (1 - p)
    tt = torch.zeros_like(x) if t is None else t.to(x.dtype)
    return torch.stack([masked.reshape(-1), tt.reshape(-1)], dim=1).contiguous(), masked


def rel_err(a, b):
    return SR.rel_err(a, b)
