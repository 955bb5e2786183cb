"""Float64 closed forms of one hidden task-head layer (Trainer/models/head.py:152-167: ConvBlock = Conv3d(3, padding 1,
bias) + LeakyReLU(0.2)) and of its three gradients, written out tap by tap so that they share nothing with the code they
check -- neither the HIP kernels nor torch's convolution.  Channels-last arrays throughout: x (D,H,W,Cin), w
(Cout,Cin,3,3,3), b (Cout,), y / dy (D,H,W,Cout).  tests/test_host_headlayers.py pins them to torch float64 autograd."""
import numpy as np

SLOPE = 0.2


def _taps():
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                yield kz, ky, kx


def _shifted(xp, kz, ky, kx, dims):
    D, H, W = dims
    return xp[kz:kz + D, ky:ky + H, kx:kx + W]


def conv_bias(x, w, b):
    """The pre-activation p[v, o] = b[o] + sum_{tap, c} w[o, c, tap] x[v + tap - 1, c] (zero padding)."""
    x, w, b = (np.asarray(a, dtype=np.float64) for a in (x, w, b))
    dims = x.shape[:3]
    xp = np.pad(x, ((1, 1), (1, 1), (1, 1), (0, 0)))
    p = np.zeros(dims + (w.shape[0],)) + b
    for kz, ky, kx in _taps():
        p += _shifted(xp, kz, ky, kx, dims) @ w[:, :, kz, ky, kx].T
    return p


def forward(x, w, b, slope=SLOPE):
    p = conv_bias(x, w, b)
    return np.where(p > 0, p, slope * p)


def lrelu_bwd(dy, y, slope=SLOPE):
    """dP from the OUTPUT y (its sign is the pre-activation's for a positive slope)."""
    return np.asarray(dy, dtype=np.float64) * np.where(np.asarray(y) > 0, 1.0, slope)


def dbias(dp):
    dp = np.asarray(dp, dtype=np.float64)
    return dp.reshape(-1, dp.shape[-1]).sum(0)


def dweight(x, dp):
    """dW[o, c, tap] = sum_v dP[v, o] x[v + tap - 1, c]."""
    x, dp = np.asarray(x, dtype=np.float64), np.asarray(dp, dtype=np.float64)
    dims = x.shape[:3]
    xp = np.pad(x, ((1, 1), (1, 1), (1, 1), (0, 0)))
    dw = np.zeros((dp.shape[-1], x.shape[-1], 3, 3, 3))
    for kz, ky, kx in _taps():
        xs = _shifted(xp, kz, ky, kx, dims).reshape(-1, x.shape[-1])
        dw[:, :, kz, ky, kx] = dp.reshape(-1, dp.shape[-1]).T @ xs
    return dw


def dinput(dp, w):
    """dX[u, c] = sum_{tap, o} w[o, c, tap] dP[u - tap + 1, o]."""
    dp, w = np.asarray(dp, dtype=np.float64), np.asarray(w, dtype=np.float64)
    dims = dp.shape[:3]
    pp = np.pad(dp, ((1, 1), (1, 1), (1, 1), (0, 0)))
    dx = np.zeros(dims + (w.shape[1],))
    for kz, ky, kx in _taps():
        dx += _shifted(pp, 2 - kz, 2 - ky, 2 - kx, dims) @ w[:, :, kz, ky, kx]
    return dx


def rel_err(a, b):
    a = np.asarray(a.detach().cpu() if hasattr(a, "detach") else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if hasattr(b, "detach") else b, dtype=np.float64)
    return float(np.abs(a - b).max()) / max(1e-30, float(np.abs(b).max()))
