"""Latent cache of stage-2 (diffusion) training.

``train_diffusion.py`` centre-crops (``randcrop=False``, 3d_ldm/train_diffusion.py:70-80), scales by fixed percentiles and encodes with
a frozen ``eval()`` autoencoder, so the latent mean and sigma of a sample never change between steps; the only fresh quantity is the
reparameterisation draw of ``z = mu + sigma * eps``.  ``LatentCache`` encodes the set once, keeps ``(mu, sigma)`` of the label and of
the image on the device, and ``batch`` turns a list of dataset indices into the three tensors a training step needs (noisy latent,
condition, regression target) in ONE launch (``ldm_latent_batch``): no autoencoder, no loader copy and no host-side ``randn`` in the step.
The reference asked MONAI for a cache of the decoded volumes (``cache=1.0``, 3d_ldm/utils.py:73); this one sits behind the encoder.

The draws are either passed in (``eps_label``, ``eps_image``, ``noise``) or made inside the kernel by Philox4x32-10 as a function of
``(seed, step, dataset index, stream, element)`` alone (include/ldm3d.h), so a sample's draws do not depend on where in which batch, or on
which rank, it lands.  Nothing is written to disk: a stale cache would silently train on the wrong autoencoder, and a rebuild costs two
encodes per sample."""
from __future__ import annotations

import ctypes as C
import time
from typing import List, Optional, Sequence

import torch

from . import _lib

MAX_BATCH = 64                                  # the indices travel to the kernel by value (LATENT_BATCH_MAX in csrc/norm_elem.h)


def cache_bytes(n_samples: int, latent_shape: Sequence[int]) -> int:
    """Device bytes of a cache: four fp32 tensors [n_samples, *latent_shape] (mu and sigma, label and image)."""
    per_sample = 1
    for s in latent_shape:
        per_sample *= int(s)
    return 4 * 4 * int(n_samples) * per_sample


def check_fits(needed: int, free: int) -> None:
    """The cache may take at most half of the free device memory: the rest belongs to the UNet's training workspace."""
    if needed > free // 2:
        raise MemoryError(f"latent cache needs {needed} bytes, more than half of the {free} bytes free on the device; "
                          "train without --cache-latents")


class LatentCache:
    """``mu_label``, ``sigma_label``, ``mu_image``, ``sigma_image``: fp32 ``[N, L, d, h, w]`` on one device."""

    def __init__(self, mu_label: torch.Tensor, sigma_label: torch.Tensor, mu_image: torch.Tensor, sigma_image: torch.Tensor):
        ts = (mu_label, sigma_label, mu_image, sigma_image)
        for t in ts:
            if t.dim() < 2 or t.dtype != torch.float32 or t.shape != mu_label.shape or t.device != mu_label.device:
                raise ValueError("LatentCache: four fp32 tensors [N, ...] of one shape on one device")
        self.mu_label, self.sigma_label, self.mu_image, self.sigma_image = (t.contiguous() for t in ts)
        self.n = int(mu_label.shape[0])
        self.latent_shape = tuple(int(s) for s in mu_label.shape[1:])
        self.per_sample = mu_label[0].numel() if self.n else 0
        self.device = mu_label.device
        self.build_seconds = 0.0

    def __len__(self) -> int:
        return self.n

    @property
    def nbytes(self) -> int:
        return cache_bytes(self.n, self.latent_shape)

    @classmethod
    @torch.no_grad()
    def build(cls, autoencoder, dataset, device, encode_batch: int = 1) -> "LatentCache":
        """Walk a ``PairVolumes`` dataset once and keep ``autoencoder.encode``'s (mu, sigma) of every image and label; no draw is taken.
        ``encode_batch`` stays 1 unless asked: the encoder's plans differ by batch size and its results are not bitwise independent of
        it, so a cache built one sample at a time holds exactly what a batch-1 training step would have computed."""
        if getattr(dataset, "randcrop", False):
            raise ValueError("LatentCache.build: the dataset crops at random (randcrop=True); a cache would freeze one crop per sample")
        n = len(dataset)
        if n < 1 or encode_batch < 1:
            raise ValueError(f"LatentCache.build: {n} samples, encode_batch {encode_batch}")
        device = torch.device(device)
        t0 = time.perf_counter()
        first = dataset[0]
        f = int(getattr(autoencoder, "factor", 4))
        lat = (int(autoencoder.latent_channels),) + tuple(int(s) // f for s in first["image"].shape[-3:])
        check_fits(cache_bytes(n, lat), int(torch.cuda.mem_get_info(device)[0]))
        mu_l, sg_l, mu_i, sg_i = (torch.empty((n,) + lat, dtype=torch.float32, device=device) for _ in range(4))
        scale_on_device = not getattr(dataset, "scale_on_host", True)
        if scale_on_device:
            from .data import scale_percentiles_gpu
        for lo in range(0, n, encode_batch):
            hi = min(lo + encode_batch, n)
            items = [first if i == 0 else dataset[i] for i in range(lo, hi)]
            for key, mu, sg in (("image", mu_i, sg_i), ("label", mu_l, sg_l)):
                x = torch.stack([it[key] for it in items]).to(device).float()
                if scale_on_device:
                    x = scale_percentiles_gpu(x)
                m, s = autoencoder.encode(x)
                if tuple(m.shape[1:]) != lat:
                    raise ValueError(f"LatentCache.build: sample {lo} encodes to {tuple(m.shape[1:])}, sample 0 to {lat}")
                mu[lo:hi].copy_(m)
                sg[lo:hi].copy_(s)
        cache = cls(mu_l, sg_l, mu_i, sg_i)
        torch.cuda.synchronize(device)
        cache.build_seconds = time.perf_counter() - t0
        return cache

    def check_idx(self, idx) -> list:
        """The dataset indices of one batch as a list of ints: 1 .. 64 of them, each inside the cache."""
        if isinstance(idx, torch.Tensor):
            idx = idx.reshape(-1).tolist()
        idx = [int(i) for i in idx]
        if not 1 <= len(idx) <= MAX_BATCH:
            raise ValueError(f"LatentCache: a batch holds 1 .. {MAX_BATCH} indices, got {len(idx)}")
        for i in idx:
            if not 0 <= i < self.n:
                raise IndexError(f"LatentCache: index {i} outside the cache's {self.n} samples")
        return idx

    def batch(self, idx, scheduler, timesteps: torch.Tensor, scale_factor: float, *, eps_label: Optional[torch.Tensor] = None,
              eps_image: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, seed: int = 0, step: int = 0,
              return_draws: bool = False):
        """-> ``(noisy, cond, target)``, each ``[B, L, d, h, w]``: the scaled, noised label latent, the unscaled image latent and the
        regression target of the scheduler's prediction type (z - noise for an ``RFlowScheduler``: ``ldm_latent_batch_rflow``, with
        the coefficients ``sample_timesteps`` wrote or those of explicit timesteps), for the samples ``idx`` at the device ``timesteps`` [B].  Either all
        three draws are given or none; without them the kernel draws with ``(seed, step)``.  ``return_draws`` appends the tuple
        ``(eps_label, eps_image, noise)`` that was used, so that the call can be repeated with explicit draws."""
        idx = self.check_idx(idx)
        B = len(idx)
        given = [t is not None for t in (eps_label, eps_image, noise)]
        if any(given) and not all(given):
            raise ValueError("LatentCache.batch: eps_label, eps_image and noise are given together or not at all")
        if not self.mu_label.is_cuda:
            raise _lib.LdmError("LatentCache.batch: CUDA tensors only (no CPU fallback)")
        dev, shape = self.device, (B,) + self.latent_shape
        sa, sb = scheduler._noising_coefs(timesteps, dev)
        if sa.numel() != B:
            raise ValueError(f"LatentCache.batch: {B} indices but {sa.numel()} timesteps")
        draws = None
        if all(given):
            draws = tuple(t.detach().to(device=dev, dtype=torch.float32).contiguous() for t in (eps_label, eps_image, noise))
            for t in draws:
                if tuple(t.shape) != shape:
                    raise ValueError(f"LatentCache.batch: a draw has shape {tuple(t.shape)}, expected {shape}")
        noisy, cond, target = (torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(3))
        out = torch.empty((3,) + shape, dtype=torch.float32, device=dev) if return_draws and draws is None else None
        e = draws or (None, None, None)
        head = (self.mu_label.data_ptr(), self.sigma_label.data_ptr(), self.mu_image.data_ptr(), self.sigma_image.data_ptr(),
                self.n, self.per_sample, (C.c_int * B)(*idx), B, sa.data_ptr(), sb.data_ptr(), float(scale_factor))
        tail = (_lib.ptr(e[0]), _lib.ptr(e[1]), _lib.ptr(e[2]), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF,
                noisy.data_ptr(), cond.data_ptr(), target.data_ptr(), _lib.ptr(out), _lib.current_stream())
        with torch.cuda.device(dev):
            _lib.check(scheduler._latent_batch(head, tail))      # the scheduler's own entry: its regression target
        if return_draws:
            return noisy, cond, target, (draws if draws is not None else (out[0], out[1], out[2]))
        return noisy, cond, target


def cond_dropout(cond: torch.Tensor, p: float, fill: float = -1.0, idx=None, seed: int = 0, step: int = 0, mask=None) -> List[bool]:
    """Condition dropout IN PLACE (``ldm_cond_dropout``, the training side of classifier-free guidance): sample b of the contiguous fp32
    CUDA tensor ``cond`` [B, ...] is overwritten with ``fill`` where the decision says so, and the decisions are returned.  ``mask`` ([B]
    truthy = drop) wins if given; otherwise sample b drops with probability ``p``, decided by Philox4x32-10 keyed by ``(seed, step)``
    and the dataset index ``idx[b]`` (default: the batch slot), never by the slot or the batch size."""
    if not (cond.is_cuda and cond.dtype == torch.float32 and cond.is_contiguous() and cond.dim() >= 1):
        raise _lib.LdmError("cond_dropout: cond must be a contiguous fp32 CUDA tensor [B, ...] (no CPU fallback)")
    B = cond.shape[0]
    ids = None
    if idx is not None:
        idx = [int(i) for i in (idx.reshape(-1).tolist() if isinstance(idx, torch.Tensor) else idx)]
        if len(idx) != B:
            raise ValueError(f"cond_dropout: {B} samples but {len(idx)} indices")
        ids = (C.c_int * B)(*idx)
    m_in = None
    if mask is not None:
        mask = [bool(v) for v in (mask.reshape(-1).tolist() if isinstance(mask, torch.Tensor) else mask)]
        if len(mask) != B:
            raise ValueError(f"cond_dropout: {B} samples but a mask of {len(mask)}")
        m_in = (C.c_ubyte * B)(*[int(v) for v in mask])
    m_out = (C.c_ubyte * max(B, 1))()
    with torch.cuda.device(cond.device):
        _lib.check(_lib.lib().ldm_cond_dropout(cond.data_ptr(), B, cond.numel() // max(B, 1), ids, float(p), float(fill), m_in,
                                               int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF, m_out, _lib.current_stream()))
    return [bool(m_out[b]) for b in range(B)]


def describe(name: str, cache: LatentCache) -> str:
    """The line train_diffusion.py logs per cache."""
    return (f"latent cache ({name}): {cache.n} samples of {'x'.join(map(str, cache.latent_shape))}, {cache.nbytes} bytes, "
            f"built in {cache.build_seconds:.2f} s")
