"""Yardstick of the image metrics (tests only, CPU): the textbook formula with torch.nn.functional.conv3d in a chosen dtype.

    ssim = ((2 mu_x mu_y + c1)(2 s_xy + c2)) / ((mu_x^2 + mu_y^2 + c1)(s_x^2 + s_y^2 + c2)),  s_x^2 = E[x^2] - mu_x^2, s_xy = E[xy] - mu_x mu_y

with valid-mode windowed moments, c1 = (k1 L)^2, c2 = (k2 L)^2.  dtype=torch.float64 is the truth; dtype=torch.float32 is the "naive"
formula (raw E[x^2] - mu^2 in single precision) whose error sets the gates of tests/test_gpu_metrics.py.  The window is separable, so
the moments are three 1-D passes (the same numbers as one dense win^3 convolution up to summation order)."""
import math

import torch
import torch.nn.functional as F


def window_1d(kernel_type="gaussian", win_size=11, kernel_sigma=1.5, dtype=torch.float64):
    if kernel_type == "uniform":
        return torch.full((win_size,), 1.0 / win_size, dtype=dtype)
    d = torch.arange((1 - win_size) / 2, (1 + win_size) / 2, dtype=dtype)
    g = torch.exp(-((d / kernel_sigma) ** 2) / 2)
    return g / g.sum()


def _moment(v, w):
    """Valid-mode separable filter of [B, C, D, H, W] with the 1-D weights w along D, H and W."""
    B, C = v.shape[:2]
    v = v.reshape(B * C, 1, *v.shape[2:])
    n = w.numel()
    v = F.conv3d(v, w.reshape(1, 1, n, 1, 1))
    v = F.conv3d(v, w.reshape(1, 1, 1, n, 1))
    v = F.conv3d(v, w.reshape(1, 1, 1, 1, n))
    return v.reshape(B, C, *v.shape[2:])


def ssim_map(x, y, data_range=1.0, kernel_type="gaussian", win_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03, dtype=torch.float64):
    x, y = x.detach().cpu().to(dtype), y.detach().cpu().to(dtype)
    w = window_1d(kernel_type, win_size, kernel_sigma, dtype)
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    mx, my = _moment(x, w), _moment(y, w)
    sxx = _moment(x * x, w) - mx * mx
    syy = _moment(y * y, w) - my * my
    sxy = _moment(x * y, w) - mx * my
    return ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))


def metrics(x, y, data_range=1.0, dtype=torch.float64, **ssim_kw):
    """dict of [B] tensors (dtype) ssim, psnr, mse, mae, nrmse, plus ssim_map [B, C, D', H', W']."""
    m = ssim_map(x, y, data_range=data_range, dtype=dtype, **ssim_kw)
    x, y = x.detach().cpu().to(dtype), y.detach().cpu().to(dtype)
    B = x.shape[0]
    diff = (x - y).reshape(B, -1)
    mse = (diff * diff).mean(dim=1)
    return {"ssim": m.reshape(B, -1).mean(dim=1), "mse": mse, "mae": diff.abs().mean(dim=1),
            "psnr": 20 * math.log10(data_range) - 10 * torch.log10(mse),
            "nrmse": torch.sqrt((diff * diff).sum(dim=1) / (y.reshape(B, -1) ** 2).sum(dim=1)), "ssim_map": m}
