"""SSIM / MS-SSIM of 3-D volumes restated from the public algorithm of pytorch_msssim 1.0 (ssim / ms_ssim with data_range 1,
K = (0.01, 0.03), an 11-tap Gaussian window, size_average=False) with torch's own F.conv3d and F.avg_pool3d.  It runs in the
dtype of its inputs: float64 is what the kernels are held to, float32 gives the rounding of an fp32 run of the same
algorithm (the tests' ref32).

pytorch_msssim itself is not installed where this project is built, so parity with the LIBRARY is not pinned by any test:
what is pinned is this restatement, which tests/test_host_evaluator.py checks against a brute-force 11^3 window sum.
"""
import numpy as np
import torch
import torch.nn.functional as F

WIN = 11
WEIGHTS = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]


def window(sigma, dtype):
    """_fspecial_gauss_1d: built in fp32 as the library builds it, then cast to the working dtype."""
    coords = torch.arange(WIN, dtype=torch.float)
    coords -= WIN // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    g /= g.sum()
    return g.to(dtype)


def gaussian_filter(x, win):
    """Separable 'valid' filtering of (B,C,D,H,W) along every spatial axis of length >= 11; shorter axes are skipped."""
    C = x.shape[1]
    out = x
    for i, s in enumerate(x.shape[2:]):
        if s >= WIN:
            shape = [C, 1, 1, 1, 1]
            shape[2 + i] = WIN
            out = F.conv3d(out, win.reshape(1, 1, *shape[2:]).repeat(C, 1, 1, 1, 1), stride=1, padding=0, groups=C)
    return out


def ssim_cs(X, Y, sigma):
    """(ssim per (b, c), cs per (b, c)) of two (B,C,D,H,W) tensors in [0, 1]."""
    win = window(sigma, X.dtype)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = gaussian_filter(X, win), gaussian_filter(Y, win)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = gaussian_filter(X * X, win) - mu1_sq
    sigma2_sq = gaussian_filter(Y * Y, win) - mu2_sq
    sigma12 = gaussian_filter(X * Y, win) - mu1_mu2
    cs_map = (2 * sigma12 + C2) / (sigma1_sq + sigma2_sq + C2)
    ssim_map = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_map
    return torch.flatten(ssim_map, 2).mean(-1), torch.flatten(cs_map, 2).mean(-1)


def ssim(X, Y, sigma=1.5):
    """ssim(..., size_average=False): one value per batch item (mean over channels)."""
    return ssim_cs(X, Y, sigma)[0].mean(1)


def ms_ssim(X, Y, sigma=1.5):
    """ms_ssim(..., size_average=False): one value per batch item."""
    assert min(X.shape[-2:]) > (WIN - 1) * 2 ** 4, \
        "Image size should be larger than %d due to the 4 downsamplings in ms-ssim" % ((WIN - 1) * 2 ** 4)
    w = torch.tensor(WEIGHTS, dtype=X.dtype)
    mcs = []
    for i in range(len(WEIGHTS)):
        s, cs = ssim_cs(X, Y, sigma)
        if i < len(WEIGHTS) - 1:
            mcs.append(torch.relu(cs))
            padding = [n % 2 for n in X.shape[2:]]
            X = F.avg_pool3d(X, kernel_size=2, padding=padding)
            Y = F.avg_pool3d(Y, kernel_size=2, padding=padding)
    s = torch.relu(s)
    stack = torch.stack(mcs + [s], dim=0)
    return torch.prod(stack ** w.view(-1, 1, 1), dim=0).mean(1)


def minmax(x):
    """get_ssim / get_ms_ssim's normalisation (evaluator.py:125-126)."""
    return (x - x.min()) / (x.max() - x.min())


def get_ssim(o, t, sigma=1.5):
    """Evaluator.get_ssim's value (a 0-d tensor in the inputs' dtype)."""
    return ssim(minmax(o), minmax(t), sigma).mean()


def get_ms_ssim(o, t, sigma=1.5):
    return ms_ssim(minmax(o), minmax(t), sigma).mean()


def brute_ssim_cs(X, Y, sigma):
    """The same maps from non-separable window sums over every 'valid' position, in float64 numpy: (mean ssim, mean cs) of
    one (D,H,W) volume whose axes are all >= 11."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    g = window(sigma, torch.float64).numpy()
    w3 = g[:, None, None] * g[None, :, None] * g[None, None, :]
    od = [n - WIN + 1 for n in X.shape]
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ss, cc = [], []
    for i in range(od[0]):
        for j in range(od[1]):
            for k in range(od[2]):
                x = X[i:i + WIN, j:j + WIN, k:k + WIN]
                y = Y[i:i + WIN, j:j + WIN, k:k + WIN]
                m1, m2 = (w3 * x).sum(), (w3 * y).sum()
                s1 = (w3 * x * x).sum() - m1 * m1
                s2 = (w3 * y * y).sum() - m2 * m2
                s12 = (w3 * x * y).sum() - m1 * m2
                cs = (2 * s12 + C2) / (s1 + s2 + C2)
                cc.append(cs)
                ss.append((2 * m1 * m2 + C1) / (m1 * m1 + m2 * m2 + C1) * cs)
    return float(np.mean(ss)), float(np.mean(cc))


def smooth_pair(shape, seed, noise=0.15):
    """A clean smooth random volume in fp32 and a noisy copy of it (scores sit well away from 0 and 1): (noisy, clean) with
    the given (D,H,W), (C,D,H,W) or (B,C,D,H,W) shape."""
    g = torch.Generator().manual_seed(seed)
    full = tuple(shape)
    lead, sp = full[:-3], full[-3:]
    n = int(np.prod(lead)) if lead else 1
    coarse = torch.rand((n, 1) + tuple(max(2, (s + 3) // 4) for s in sp), generator=g, dtype=torch.float64)
    clean = F.interpolate(coarse, size=sp, mode="trilinear", align_corners=True).reshape(full)
    noisy = clean + noise * torch.randn(full, generator=g, dtype=torch.float64)
    return noisy.float(), clean.float()
