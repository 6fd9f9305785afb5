"""Sliding-window geometry for latent sampling of volumes larger than the UNet's training patch (``ldm_window_*``).

The UNet is trained on patches (3d_ldm/utils.py:86-91); a whole scan's latent is larger and of any size.  Every denoising step cuts
the latent into overlapping windows of the trained size, runs the UNet on the batch of windows and blends their eps predictions
with an importance map before one scheduler step on the whole latent (``DiffusionModelUNet.denoise_step_windows``,
``LatentDiffusionInferer.sample_sliding_window``).  This module builds the grid on the host: window starts, per-axis weight
tables and cover tables; the device handle owns copies of them."""
from __future__ import annotations

import ctypes as C
import itertools
import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib


_UIDS = itertools.count(1)


def window_starts(dim: int, roi: int, overlap: float = 0.25) -> List[int]:
    """Window starts along one axis, MONAI's ``dense_patch_slices`` rule (with ``_get_scan_interval``):
    interval = roi if roi == dim else max(int(roi * (1 - overlap)), 1); the number of windows is the first d with
    d * interval + roi >= dim, plus 1; start_d = min(d * interval, dim - roi)."""
    dim, roi = int(dim), int(roi)
    if not 1 <= roi <= dim:
        raise ValueError(f"window size {roi} must be in [1, {dim}]")
    if not 0.0 <= overlap < 1.0:
        raise ValueError(f"overlap must be in [0, 1), got {overlap}")
    interval = roi if roi == dim else max(int(roi * (1 - overlap)), 1)
    d = 0
    while d * interval + roi < dim:
        d += 1
    return [min(i * interval, dim - roi) for i in range(d + 1)]


def axis_profile(roi: int, mode: str = "gaussian", sigma_scale: float = 0.125) -> np.ndarray:
    """Unnormalised importance of each offset in a window of ``roi`` voxels (float64)."""
    if mode == "constant":
        return np.ones(roi, dtype=np.float64)
    if mode == "gaussian":
        sigma = sigma_scale * roi
        u = np.arange(roi, dtype=np.float64) - (roi - 1) / 2.0
        return np.exp(-(u * u) / (2.0 * sigma * sigma))
    raise ValueError(f"mode must be 'gaussian' or 'constant', got {mode!r}")


def axis_tables(dim: int, roi: int, starts: Sequence[int], profile: np.ndarray):
    """Normalised weight table t[i][p - s_i] = g(p - s_i) / sum over the windows i' covering p of g(p - s_i'), [n][roi] float64,
    and the cover table [dim][2] = {first covering window, count} (int32)."""
    n = len(starts)
    den = np.zeros(dim, dtype=np.float64)
    cover = np.zeros((dim, 2), dtype=np.int32)
    cover[:, 0] = -1
    for i, s in enumerate(starts):
        den[s:s + roi] += profile
        seg = cover[s:s + roi]
        seg[seg[:, 0] < 0, 0] = i
        seg[:, 1] += 1
    tab = np.empty((n, roi), dtype=np.float64)
    for i, s in enumerate(starts):
        tab[i] = profile / den[s:s + roi]
    return tab, cover


class WindowGrid:
    """The windows of a latent of spatial ``shape``: per axis roi = min(roi_size, dim), starts by ``window_starts``, windows in
    C order over (d, h, w) starts (MONAI's order).  The weight of window (i, j, k) at voxel p is t_d[i] * t_h[j] * t_w[k] with
    per-axis tables normalised over the windows covering p, so the weights at every voxel sum to one and an axis with a single
    window has weight exactly 1.0 (one window over the whole latent blends to its eps bit for bit).

    Not MONAI's importance map bit for bit: MONAI filters a delta centred at roi // 2 with a Gaussian of sigma = sigma_scale * roi,
    clamps the map's minimum and divides by the accumulated 3-D map; here the Gaussian is centred at (roi - 1) / 2 and the
    normalisation is separable (same blend for a grid of windows, no clamp)."""

    def __init__(self, shape: Sequence[int], roi: Sequence[int] | int, overlap: float = 0.25, mode: str = "gaussian",
                 sigma_scale: float = 0.125):
        shape = [int(v) for v in shape]
        if len(shape) != 3:
            raise ValueError(f"expected a 3-D spatial shape, got {shape}")
        roi = [int(roi)] * 3 if isinstance(roi, (int, np.integer)) else [int(v) for v in roi]
        if len(roi) != 3 or min(roi) < 1:
            raise ValueError(f"bad window size {roi}")
        self.shape = tuple(shape)
        self.roi = tuple(min(r, d) for r, d in zip(roi, shape))
        self.overlap, self.mode, self.sigma_scale = float(overlap), mode, float(sigma_scale)
        self.axis_starts = [window_starts(d, r, overlap) for d, r in zip(self.shape, self.roi)]
        self.n = tuple(len(s) for s in self.axis_starts)
        self.tables64, self.covers = [], []
        for d, r, st in zip(self.shape, self.roi, self.axis_starts):
            tab, cov = axis_tables(d, r, st, axis_profile(r, mode, sigma_scale))
            self.tables64.append(tab)
            self.covers.append(cov)
        self.uid = next(_UIDS)                              # never reused (denoise_step_windows: which grid its window buffer holds)
        self._h = None

    @property
    def n_windows(self) -> int:
        return self.n[0] * self.n[1] * self.n[2]

    @property
    def starts(self) -> List[tuple]:
        """Start (d, h, w) of every window in window order."""
        return [(a, b, c) for a in self.axis_starts[0] for b in self.axis_starts[1] for c in self.axis_starts[2]]

    def check_model(self, unet) -> None:
        """Fail loudly unless ``unet``'s inference plan takes a window of this size (a multiple of 2^(levels-1))."""
        L = _lib.lib()
        if L.ldm_unet_workspace_bytes(unet._h, 1, *self.roi) == 0:
            msg = L.ldm_last_error()
            raise _lib.LdmError(f"window {self.roi} is not a size the UNet takes: {msg.decode() if msg else '?'}")

    # -- device handle ---------------------------------------------------------------------------------------------------
    def handle(self) -> C.c_void_p:
        if self._h is None:
            dims = (C.c_int * 3)(*self.shape)
            roi = (C.c_int * 3)(*self.roi)
            n = (C.c_int * 3)(*self.n)
            starts = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.int32) for s in self.axis_starts]))
            weights = np.ascontiguousarray(np.concatenate([t.astype(np.float32).reshape(-1) for t in self.tables64]))
            cover = np.ascontiguousarray(np.concatenate([c.reshape(-1) for c in self.covers]).astype(np.int32))
            h = C.c_void_p()
            _lib.check(_lib.lib().ldm_window_grid_create(dims, roi, n, starts.ctypes.data, weights.ctypes.data, cover.ctypes.data,
                                                         C.byref(h)))
            self._h = h
        return self._h

    def _vol(self, vol: torch.Tensor, what: str) -> torch.Tensor:
        if vol.dim() == 5:
            if vol.shape[0] != 1:
                raise ValueError(f"{what}: one volume at a time, got batch {vol.shape[0]}")
            vol = vol[0]
        if vol.dim() != 4 or tuple(vol.shape[1:]) != self.shape:
            raise ValueError(f"{what}: expected [C, {', '.join(map(str, self.shape))}], got {tuple(vol.shape)}")
        if not vol.is_cuda:
            raise _lib.LdmError(f"{what}: tensor is on {vol.device}; the window kernels run on the GPU only")
        return vol.detach().to(torch.float32).contiguous()

    def gather(self, vol: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[C, D, H, W] (or [1, C, D, H, W]) -> windows [nW, C, rd, rh, rw]."""
        vol = self._vol(vol, "WindowGrid.gather")
        Cc = vol.shape[0]
        if out is None:
            out = torch.empty((self.n_windows, Cc) + self.roi, dtype=torch.float32, device=vol.device)
        elif not (out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (self.n_windows, Cc) + self.roi):
            raise ValueError("WindowGrid.gather: out must be a contiguous fp32 [nW, C, rd, rh, rw] tensor")
        with torch.cuda.device(vol.device):
            _lib.check(_lib.lib().ldm_window_gather(self.handle(), vol.data_ptr(), out.data_ptr(), Cc, _lib.current_stream()))
        return out

    def blend(self, win: torch.Tensor) -> torch.Tensor:
        """windows [nW, C, rd, rh, rw] -> importance-weighted blend [1, C, D, H, W]."""
        if win.dim() != 5 or win.shape[0] != self.n_windows or tuple(win.shape[2:]) != self.roi:
            raise ValueError(f"WindowGrid.blend: expected [{self.n_windows}, C, {', '.join(map(str, self.roi))}], got {tuple(win.shape)}")
        if not win.is_cuda:
            raise _lib.LdmError("WindowGrid.blend: the window kernels run on the GPU only")
        win = win.detach().to(torch.float32).contiguous()
        out = torch.empty((1, win.shape[1]) + self.shape, dtype=torch.float32, device=win.device)
        with torch.cuda.device(win.device):
            _lib.check(_lib.lib().ldm_window_blend(self.handle(), win.data_ptr(), out.data_ptr(), win.shape[1], _lib.current_stream()))
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                _lib.lib().ldm_window_grid_destroy(self._h)
                self._h = None
        except Exception:
            pass


def default_batch(unet, n: int, spatial: Sequence[int], device, guided: bool = False) -> int:
    """All ``n`` samples of ``spatial`` in one UNet call, halved until the workspace fits in half of the device's free memory
    (``guided``: the workspace of the classifier-free-guidance step, which runs twice the samples per call)."""
    L = _lib.lib()
    free = torch.cuda.mem_get_info(device)[0]
    b = int(n)
    while b > 1:
        nbytes = (L.ldm_unet_guided_workspace_bytes if guided else L.ldm_unet_workspace_bytes)(unet._h, b, *[int(s) for s in spatial])
        if nbytes and nbytes <= free // 2:
            break
        b = max(1, math.ceil(b / 2))
    return b


def default_sw_batch(unet, grid: WindowGrid, device, guided: bool = False) -> int:
    """``default_batch`` over the windows of ``grid``."""
    return default_batch(unet, grid.n_windows, grid.roi, device, guided)
