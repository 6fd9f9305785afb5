"""Image-quality metrics on the GPU: 3-D SSIM, PSNR, MSE, MAE and NRMSE of a prediction against a target, all from ONE launch
of ``ldm_op_image_metrics`` (csrc/metrics.h).  Constructor arguments and semantics follow MONAI's ``monai.metrics.SSIMMetric`` /
``PSNRMetric`` (restated from MONAI's published source, DESIGN.md section 7: MONAI is not a dependency):

    ssim = ((2 mu_x mu_y + c1)(2 s_xy + c2)) / ((mu_x^2 + mu_y^2 + c1)(s_x^2 + s_y^2 + c2)),  c1 = (k1 L)^2, c2 = (k2 L)^2, L = data_range

over a separable valid-mode window (Gaussian ``exp(-(d / sigma)^2 / 2)`` over ``d = arange((1 - win) / 2, (1 + win) / 2)`` or uniform,
normalised per axis), averaged over the channels and the map; ``psnr = 20 log10(max_val) - 10 log10(mse)``.  There is no CPU path:
CPU tensors raise ``LdmError``."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib

_OUT = ("ssim", "psnr", "mse", "mae", "nrmse", "y_min", "y_max")


def window_weights(kernel_type: str = "gaussian", win_size: int = 11, kernel_sigma: float = 1.5) -> List[float]:
    """The ``win_size`` normalised 1-D weights (Python floats; the library takes them as fp32)."""
    win = int(win_size)
    if win < 1:
        raise ValueError(f"win_size must be positive, got {win_size}")
    if kernel_type == "uniform":
        return [1.0 / win] * win
    if kernel_type != "gaussian":
        raise ValueError(f"kernel_type must be 'gaussian' or 'uniform', got {kernel_type!r}")
    if not kernel_sigma > 0:
        raise ValueError(f"kernel_sigma must be positive, got {kernel_sigma}")
    g = [math.exp(-((i + (1 - win) / 2.0) / kernel_sigma) ** 2 / 2.0) for i in range(win)]
    s = math.fsum(g)
    return [v / s for v in g]


def _check_pair(pred: torch.Tensor, target: torch.Tensor, win: int) -> None:
    if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise TypeError("image metrics take torch tensors")
    if pred.shape != target.shape:
        raise ValueError(f"y_pred and y must have the same shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if pred.dim() != 5:
        raise ValueError(f"expected [B, C, D, H, W] volumes, got {tuple(pred.shape)}")
    if pred.numel() == 0:
        raise ValueError(f"empty volume {tuple(pred.shape)}")
    if win % 2 == 0 or win < 3 or win > 11:
        raise ValueError(f"win_size must be odd and in 3..11, got {win}")
    if min(pred.shape[2:]) < win:
        raise ValueError(f"volume {tuple(pred.shape[2:])} is smaller than the {win}^3 window")
    if not pred.is_cuda or not target.is_cuda:
        raise _lib.LdmError("image metrics run on the GPU only: CUDA tensors expected (there is no CPU path)")
    if pred.device != target.device:
        raise ValueError(f"y_pred is on {pred.device}, y on {target.device}")


def _w_contiguous(t: torch.Tensor) -> torch.Tensor:
    """fp32, W stride 1 and no negative stride: a crop of a padded buffer passes through as the view it is."""
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.stride(4) != 1 and t.shape[4] > 1:
        t = t.contiguous()
    return t


def _metrics_raw(pred: torch.Tensor, target: torch.Tensor, data_range: float, kernel_type: str, win_size: int, kernel_sigma: float,
                 k1: float, k2: float, full_image: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    win = int(win_size)
    _check_pair(pred, target, win)
    if not data_range > 0:
        raise ValueError(f"data_range must be positive, got {data_range}")
    weights = window_weights(kernel_type, win, kernel_sigma)
    x, y = _w_contiguous(pred), _w_contiguous(target)
    B, Cn, D, H, W = x.shape
    L = _lib.lib()
    out = torch.empty((B, 8), dtype=torch.float32, device=x.device)
    ssim_map = torch.empty((B, Cn, D - win + 1, H - win + 1, W - win + 1), dtype=torch.float32, device=x.device) if full_image else None
    scratch = torch.empty((L.ldm_op_image_metrics_scratch_bytes(B, Cn, D, H, W, win),), dtype=torch.uint8, device=x.device)
    xs = (C.c_int64 * 5)(*x.stride()[:4], 1)
    ys = (C.c_int64 * 5)(*y.stride()[:4], 1)
    wv = (C.c_float * win)(*weights)
    with torch.cuda.device(x.device):
        _lib.check(L.ldm_op_image_metrics(x.data_ptr(), xs, y.data_ptr(), ys, B, Cn, D, H, W, wv, win, float(data_range), float(k1), float(k2),
                                          out.data_ptr(), _lib.ptr(ssim_map), scratch.data_ptr(), scratch.numel(), _lib.current_stream()))
    return out, ssim_map


def image_metrics(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0, kernel_type: str = "gaussian", win_size: int = 11,
                  kernel_sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03, return_full_image: bool = False) -> Dict[str, torch.Tensor]:
    """``ssim, psnr, mse, mae, nrmse`` (and ``y_min, y_max`` of the target) of ``pred`` against ``target`` ([B, C, D, H, W] CUDA tensors):
    device tensors of shape [B], nothing is read back.  ``return_full_image`` adds ``ssim_map`` [B, C, D-win+1, H-win+1, W-win+1]."""
    out, ssim_map = _metrics_raw(pred, target, data_range, kernel_type, win_size, kernel_sigma, k1, k2, return_full_image)
    res = {name: out[:, i] for i, name in enumerate(_OUT)}
    if ssim_map is not None:
        res["ssim_map"] = ssim_map
    return res


def _reduce(v: torch.Tensor, reduction: str) -> torch.Tensor:
    if reduction == "mean":
        return v.mean()
    if reduction == "sum":
        return v.sum()
    if reduction == "none":
        return v
    raise ValueError(f"reduction must be 'mean', 'sum' or 'none', got {reduction!r}")


class SSIMMetric:
    """MONAI's ``SSIMMetric`` for 3-D volumes: ``__call__(y_pred, y)`` returns the per-volume SSIM [B, 1]; ``aggregate()`` reduces what
    the calls since ``reset()`` returned."""

    def __init__(self, spatial_dims: int = 3, data_range: float = 1.0, kernel_type: str = "gaussian", win_size: int = 11,
                 kernel_sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03, reduction: str = "mean"):
        if spatial_dims != 3:
            raise NotImplementedError(f"SSIMMetric: only spatial_dims=3 is implemented, got {spatial_dims}")
        _reduce(torch.zeros(1), reduction)
        window_weights(kernel_type, win_size, kernel_sigma)
        if int(win_size) % 2 == 0 or not 3 <= int(win_size) <= 11:
            raise ValueError(f"win_size must be odd and in 3..11, got {win_size}")
        self.spatial_dims, self.data_range, self.kernel_type, self.win_size = 3, float(data_range), kernel_type, int(win_size)
        self.kernel_sigma, self.k1, self.k2, self.reduction = float(kernel_sigma), float(k1), float(k2), reduction
        self._buffer: List[torch.Tensor] = []

    def __call__(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        out, _ = _metrics_raw(y_pred, y, self.data_range, self.kernel_type, self.win_size, self.kernel_sigma, self.k1, self.k2, False)
        v = out[:, 0:1]
        self._buffer.append(v)
        return v

    def aggregate(self, reduction: Optional[str] = None) -> torch.Tensor:
        if not self._buffer:
            raise ValueError("aggregate() before any call")
        return _reduce(torch.cat(self._buffer, dim=0), reduction or self.reduction)

    def reset(self) -> None:
        self._buffer = []


class PSNRMetric:
    """MONAI's ``PSNRMetric``: ``20 log10(max_val) - 10 log10(mse)`` per volume, [B, 1]; identical inputs give +inf."""

    def __init__(self, max_val: float, reduction: str = "mean"):
        if not max_val > 0:
            raise ValueError(f"max_val must be positive, got {max_val}")
        _reduce(torch.zeros(1), reduction)
        self.max_val, self.reduction = float(max_val), reduction
        self._buffer: List[torch.Tensor] = []

    def __call__(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        win = min(11, (min(y_pred.shape[2:]) - 1) // 2 * 2 + 1) if isinstance(y_pred, torch.Tensor) and y_pred.dim() == 5 else 11
        out, _ = _metrics_raw(y_pred, y, self.max_val, "gaussian", max(win, 3), 1.5, 0.01, 0.03, False)
        v = out[:, 1:2]
        self._buffer.append(v)
        return v

    aggregate = SSIMMetric.aggregate
    reset = SSIMMetric.reset
