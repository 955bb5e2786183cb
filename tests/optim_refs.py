"""Plain restatements of the four optimiser steps brainfm_amd/csrc/optim.hip runs, for float64 torch tensors: what
torch.optim.Adam, torch.optim.AdamW, torch.optim.SGD(momentum, dampening 0, nesterov off) and the reference's utils.LARS
(utils/misc.py:1291-1317) compute, with the unscale * clip coefficient `grad_scale` in front.  tests/test_host_optim.py pins
them against torch's own optimisers and against the LARS fixture of tests/golden/optim.npz; the GPU tests then compare the
kernels with them.
Every function returns new tensors and leaves its arguments alone."""
import torch


def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0, one_minus_beta2=None):
    """-> (p, m, v) after step `step` (1-based): coupled weight decay, bias-corrected moments.  one_minus_beta2: the factor of
    g^2 where it is not the exact 1 - beta2 (the AdamW kernel forms it in float32)."""
    g = grad_scale * g + weight_decay * p
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2 if one_minus_beta2 is None else one_minus_beta2) * g * g
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / (bc2 ** 0.5) + eps)
    return p, m, v


def adamw_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0, one_minus_beta2=None):
    """-> (p, m, v): the decay shrinks the parameter and stays out of the gradient; otherwise adam_step."""
    return adam_step(p * (1 - lr * weight_decay), g, m, v, step, lr, beta1, beta2, eps, 0.0, grad_scale, one_minus_beta2)


def sgd_step(p, g, buf, lr, momentum=0.9, weight_decay=0.0, grad_scale=1.0):
    """-> (p, buf); a zero buffer reproduces torch's first step (buf = g)."""
    g = grad_scale * g + weight_decay * p
    buf = momentum * buf + g
    return p - lr * buf, buf


def lars_step(p, g, mu, lr, weight_decay=0.0, momentum=0.9, eta=1e-3, ndim=None, grad_scale=1.0):
    """-> (p, mu).  ndim: the parameter's dimension count in the reference (default: p's own); 1-D parameters get neither
    decay nor the trust ratio."""
    ndim = p.dim() if ndim is None else ndim
    dp = grad_scale * g
    if ndim != 1:
        dp = dp + weight_decay * p
        pn, un = float(p.norm()), float(dp.norm())
        q = eta * pn / un if (pn > 0.0 and un > 0.0) else 1.0
        dp = dp * q
    mu = momentum * mu + dp
    return p - lr * mu, mu


def clip_coef(g, clip, unscale=1.0, norm=None):
    """utils/misc.py:1329-1338 on the unscaled gradient: the factor the parameter's gradient is multiplied by.  norm: the
    unscaled gradient's norm where the caller has measured it."""
    if clip <= 0:
        return 1.0
    c = clip / ((float((g * unscale).norm()) if norm is None else norm) + 1e-6)
    return c if c < 1 else 1.0
