"""Measurement-guided sampling (diffusion posterior sampling, Chung et al. 2023; reconstruction guidance): a chain steered by the
gradient of a loss on the model's own UNCLIPPED prediction of the clean latent.

``ConsistencyGuidance`` is the built-in measurement, a weighted pooled quadratic in latent space: the denoised latent keeps the
regional means of a measured one.  Per step at timestep t, a = sqrt(abar_t), s = sqrt(1 - abar_t), m = UNet(x_t, t, cond)::

    x0_hat = (x - s m) / a   (epsilon)  |  m  (sample)  |  a x - s m  (v_prediction)
    r      = weight * (P x0_hat - target)         P: mean over non-overlapping pool^3 cubes, per channel
    L_b    = 1/2 |r_b|^2
    g      = dL/dx0_hat = pool^-3 upsample_nearest(weight * r)
    grad_x L = c_x g + J^T(c_m g)                 (c_x, c_m) = (1/a, -s/a) | (0, 1) | (a, -s);  J^T: the UNet's input VJP
    x_{t-1}  = scheduler.step(m, t, x_t) - zeta_b grad_x L_b,   zeta_b = scale / max(|r_b|, 1e-12) (normalize) or scale

The fused path (``DiffusionModelUNet.denoise_step_measured``) runs this on the device sampler with nothing read by the host inside a
chain; the host-driven path (``host_correction``) differentiates the loss through the module's forward with torch autograd, which is
also the path any other differentiable loss would take.

``ImageConsistencyGuidance`` is the same measurement on the DECODED prediction: the chain keeps the regional means of a measured IMAGE
(the low-count volume), which are unbiased estimates of the clean volume's; the latent of a noisy scan estimates nothing.  With sf the
inferer's ``scale_factor`` and Dec the AutoencoderKL decoder (differentiable w.r.t. its latent, ``AutoencoderKL.decode``)::

    y_hat  = Dec(x0_hat / sf)
    r      = weight * (P y_hat - target)          P over pool^3 cubes of the image, per image channel
    g_img  = pool^-3 upsample_nearest(weight * r);  dz = Dec'^T g_img
    grad_x L = c_x (dz / sf) + J^T(c_m (dz / sf))

fused in ``DiffusionModelUNet.denoise_step_measured(..., autoencoder=)`` (``ldm_unet_denoise_step_measured_image``).  Not built: image
gradients through the ENCODER, measurements other than the weighted pooled quadratic (PSF blur, projections), and guidance together
with sliding windows, ensembles, cfg, RePaint or ``sample_concurrent``.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _lib

PREDICTION_TYPES = ("epsilon", "sample", "v_prediction")


def coefficients(prediction_type: str, abar: float) -> Tuple[float, float]:
    """(c_x, c_m): d x0_hat / d x_t and d x0_hat / d m at cumulative alpha ``abar`` for the scheduler's prediction type."""
    a, s = math.sqrt(abar), math.sqrt(1.0 - abar)
    if prediction_type == "epsilon":
        return 1.0 / a, -s / a
    if prediction_type == "sample":
        return 0.0, 1.0
    if prediction_type == "v_prediction":
        return a, -s
    raise ValueError(f"prediction_type given as {prediction_type!r} must be one of {list(PREDICTION_TYPES)}")


def check_measurable(scheduler, *, cfg=None, inpaint=False, windows=False, ensemble=False, concurrent=False) -> None:
    """The refusal table of measurement guidance: NotImplementedError naming what was refused.  The scheduler speaks for itself
    (``measurable``): DDPM and DDIM are, the multistep solvers and rectified flow are not."""
    if not getattr(scheduler, "measurable", False):
        raise NotImplementedError(f"measurement guidance is not implemented for {type(scheduler).__name__}: it is built on the "
                                  "single-step DDPM / DDIM update and their x0_hat")
    for on, what in ((cfg is not None, "classifier-free guidance (cfg)"), (inpaint, "inpainting"), (windows, "sliding windows"),
                     (ensemble, "ensembles"), (concurrent, "sample_concurrent")):
        if on:
            raise NotImplementedError(f"measurement guidance together with {what} is not implemented")


class ConsistencyGuidance:
    """``target`` [1 or B, C, d/pool, h/pool, w/pool]: the pooled latent the chain is held to (e.g. the low-count scan's latent);
    ``weight`` >= 0, broadcastable to ``target`` (None: 1; fractional values are a soft mask); ``pool``: edge of the averaging cubes
    (1: voxel identity); ``scale``: the step size zeta, divided by |r_b| per sample when ``normalize`` (DPS).

    After a chain ``norms`` holds |r_b| per step, [n_steps, B] on the CPU (read once, after the chain)."""

    space = "latent"                                  # what ``target`` is a pooled copy of, and ``check`` takes the shape of

    def __init__(self, target: torch.Tensor, weight: Optional[torch.Tensor] = None, pool: int = 1, scale: float = 1.0,
                 normalize: bool = True):
        if not isinstance(pool, int) or pool < 1:
            raise ValueError(f"pool must be a positive integer, got {pool!r}")
        if target.dim() != 5:
            raise ValueError(f"target must be [1 or B, C, d/pool, h/pool, w/pool], got {tuple(target.shape)}")
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32)
            if bool((weight < 0).any()):
                raise ValueError("weight must be >= 0")
            try:
                shape = torch.broadcast_shapes(tuple(weight.shape), tuple(target.shape))
            except RuntimeError as e:
                raise ValueError(f"weight {tuple(weight.shape)} is not broadcastable to target {tuple(target.shape)}") from e
            if shape != tuple(target.shape):
                raise ValueError(f"weight {tuple(weight.shape)} is not broadcastable to target {tuple(target.shape)}")
        self.target, self.weight = target, weight
        self.pool, self.scale, self.normalize = pool, float(scale), bool(normalize)
        self.norms: Optional[torch.Tensor] = None

    # -- validation against a chain's latent ------------------------------------------------------------------------
    def measured_shape(self, latent_shape, autoencoder=None) -> tuple:
        """The shape of the tensor the measurement pools, for a chain on latents of ``latent_shape``: here, the latent itself."""
        return tuple(int(v) for v in latent_shape)

    def check(self, shape) -> None:
        """ValueError unless a latent (``ImageConsistencyGuidance``: an image) of ``shape`` [B, C, d, h, w] pools onto ``target``."""
        B, C, d, h, w = (int(v) for v in shape)
        p = self.pool
        if d % p or h % p or w % p:
            raise ValueError(f"pool {p} does not divide the {self.space} dims {(d, h, w)}")
        want = (C, d // p, h // p, w // p)
        if self.target.shape[0] not in (1, B) or tuple(self.target.shape[1:]) != want:
            raise ValueError(f"target must be [1 or {B}, {', '.join(map(str, want))}], got {tuple(self.target.shape)}")

    def device_tensors(self, shape, device):
        """(target, weight | None) as the kernels read them: contiguous fp32 on ``device``, the weight expanded to the target's
        per-sample shape with batch 1 or B.  Copies: the caller's tensors are never written."""
        self.check(shape)
        tgt = self.target.detach().to(device=device, dtype=torch.float32).contiguous()
        wgt = None
        if self.weight is not None:
            w = self.weight.detach().to(device=device, dtype=torch.float32)
            w = w.reshape((1,) * (5 - w.dim()) + tuple(w.shape))
            wgt = w.expand((w.shape[0],) + tuple(tgt.shape[1:])).contiguous()      # batch 1 or the target's
        return tgt, wgt

    # -- the host-driven arithmetic (fp32 torch; what tests/guidance_ref.py restates in fp64) ------------------------------
    def pooled(self, x: torch.Tensor) -> torch.Tensor:
        return x if self.pool == 1 else torch.nn.functional.avg_pool3d(x, self.pool)

    def residual(self, x0_hat: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor]) -> torch.Tensor:
        r = self.pooled(x0_hat) - target
        return r if weight is None else weight * r

    def zeta(self, norm: torch.Tensor) -> torch.Tensor:
        """Per-sample step size [B] from |r_b| [B]."""
        return self.scale / norm.clamp_min(1e-12) if self.normalize else torch.full_like(norm, self.scale)

    def host_correction(self, forward, x: torch.Tensor, timestep, scheduler, target: torch.Tensor, weight: Optional[torch.Tensor]):
        """-> (m, zeta_b grad_x L_b [B, ...], |r_b| [B]) for a host-driven step: ``forward(x)`` is differentiated w.r.t. ``x`` by torch
        autograd (the module's input VJP behind it), the loss is this measurement on the unclipped x0_hat."""
        return self._correction(forward, None, x, timestep, scheduler, target, weight)

    def _correction(self, forward, decode, x, timestep, scheduler, target, weight):
        """``host_correction`` of both measurements: ``decode`` (None: identity) maps x0_hat to what is measured."""
        abar = float(scheduler.alphas_cumprod[int(timestep)])
        a, s = math.sqrt(abar), math.sqrt(1.0 - abar)
        with torch.enable_grad():
            xg = x.detach().clone().requires_grad_(True)
            m = forward(xg)
            pt = scheduler.prediction_type
            x0 = (xg - s * m) / a if pt == "epsilon" else m if pt == "sample" else a * xg - s * m
            r = self.residual(x0 if decode is None else decode(x0), target, weight)
            n2 = r.reshape(r.shape[0], -1).pow(2).sum(1)
            grad, = torch.autograd.grad(0.5 * n2.sum(), xg)
        norm = n2.detach().sqrt()
        z = self.zeta(norm).reshape((-1,) + (1,) * (x.dim() - 1))
        return m.detach(), z * grad, norm

    # -- the device state of a fused chain -------------------------------------------------------------------------------
    def device_state(self, shape, device, n_steps: int):
        """The ``ldm_measurement`` of a fused chain over ``n_steps`` rows on latents of ``shape``, with the tensors it points at."""
        tgt, wgt = self.device_tensors(shape, device)
        B = int(shape[0])
        bufs = dict(target=tgt, weight=wgt,
                    grad_out=torch.empty(tuple(shape), dtype=torch.float32, device=device),
                    gx=torch.empty(tuple(shape), dtype=torch.float32, device=device),
                    dx=torch.empty(tuple(shape), dtype=torch.float32, device=device),
                    norm2=torch.zeros((B,), dtype=torch.float32, device=device),
                    norm_table=torch.zeros((int(n_steps), B), dtype=torch.float32, device=device))
        rec = _lib.Measurement()
        rec.target, rec.target_batch = tgt.data_ptr(), int(tgt.shape[0])
        rec.weight, rec.weight_batch = (wgt.data_ptr(), int(wgt.shape[0])) if wgt is not None else (None, 1)
        rec.pool, rec.scale, rec.normalize = self.pool, self.scale, int(self.normalize)
        for k in ("grad_out", "gx", "dx", "norm2", "norm_table"):
            setattr(rec, k, bufs[k].data_ptr())
        return rec, bufs

    def record(self, sample: int = 0) -> dict:
        """What ``inference.py`` writes per volume: pool, scale and the first and last per-step residual norm of volume ``sample`` of
        the batch (the first and last rows of ``norms`` that were stepped: a warm chain leaves its skipped rows at 0)."""
        n = self.norms
        first = last = None
        if n is not None and n.numel():
            col = n[:, int(sample)]
            col = col[col > 0] if bool((col > 0).any()) else col
            first, last = float(col[0]), float(col[-1])
        return dict(pool=self.pool, scale=self.scale, normalize=self.normalize, residual_norm_first=first, residual_norm_last=last)


class ImageConsistencyGuidance(ConsistencyGuidance):
    """``ConsistencyGuidance`` on the decoded prediction: ``target`` [1 or B, C_img, Di/pool, Hi/pool, Wi/pool] holds the pooled IMAGE the
    chain is held to (e.g. the low-count volume), (Di, Hi, Wi) = the latent dims times the AutoencoderKL's factor; ``weight``, ``pool``,
    ``scale``, ``normalize``, ``zeta``, ``norms`` and ``record()`` as there.  ``LatentDiffusionInferer.sample`` needs its
    ``autoencoder_model`` to be the differentiable ``AutoencoderKL`` whose latent the UNet denoises."""

    space = "image"

    def measured_shape(self, latent_shape, autoencoder=None) -> tuple:
        """[B, C_img, Di, Hi, Wi] of the image ``autoencoder`` decodes a latent of ``latent_shape`` to; ValueError when the latent's
        channel count is not the autoencoder's."""
        if autoencoder is None:
            raise ValueError("an image-space measurement needs the autoencoder_model that decodes the latent")
        B, C, d, h, w = (int(v) for v in latent_shape)
        if C != int(autoencoder.latent_channels):
            raise ValueError(f"the autoencoder's latent_channels ({int(autoencoder.latent_channels)}) differ from the latent's channels ({C})")
        f = int(autoencoder.factor)
        return (B, int(autoencoder.out_channels), d * f, h * f, w * f)

    def host_correction(self, forward, decode, x: torch.Tensor, timestep, scheduler, target: torch.Tensor, weight: Optional[torch.Tensor]):
        """As ``ConsistencyGuidance.host_correction``, the loss on ``decode(x0_hat)``: ``decode`` (x0_hat -> image, the division by the
        scale factor included) is differentiated by torch autograd too (``AutoencoderKL.decode``'s data-only backward behind it)."""
        return self._correction(forward, decode, x, timestep, scheduler, target, weight)

    def device_state(self, shape, device, n_steps: int, autoencoder=None, scale_factor: float = 1.0):
        """The ``ldm_image_measurement`` of a fused chain over ``n_steps`` rows on latents of ``shape``, with the tensors it points at
        (the decoder's gradient workspace among them: ``autoencoder`` owns it)."""
        ishape = self.measured_shape(shape, autoencoder)
        tgt, wgt = self.device_tensors(ishape, device)
        B, (_, d, h, w) = int(shape[0]), (int(v) for v in shape[1:])
        L = _lib.lib()
        nbytes = int(L.ldm_image_residual_scratch_bytes(*ishape, self.pool))
        if nbytes == 0:
            _lib.check(-1)                               # the library's own message: the shape or the pool was refused

        def lat():
            return torch.empty(tuple(shape), dtype=torch.float32, device=device)
        bufs = dict(target=tgt, weight=wgt, z0=lat(), dz=lat(), grad_out=lat(), gx=lat(), dx=lat(),
                    recon=torch.empty(ishape, dtype=torch.float32, device=device),
                    norm2=torch.zeros((B,), dtype=torch.float32, device=device),
                    norm_table=torch.zeros((int(n_steps), B), dtype=torch.float32, device=device),
                    partials=torch.zeros((nbytes // 8,), dtype=torch.float64, device=device),
                    vae_workspace=autoencoder._decode_grad_workspace(B, d, h, w, device))
        rec = _lib.ImageMeasurement()
        rec.target, rec.target_batch = tgt.data_ptr(), int(tgt.shape[0])
        rec.weight, rec.weight_batch = (wgt.data_ptr(), int(wgt.shape[0])) if wgt is not None else (None, 1)
        rec.pool, rec.scale, rec.normalize, rec.inv_scale_factor = self.pool, self.scale, int(self.normalize), 1.0 / float(scale_factor)
        for k in ("z0", "recon", "dz", "grad_out", "gx", "dx", "norm2", "norm_table", "partials", "vae_workspace"):
            setattr(rec, k, bufs[k].data_ptr())
        rec.vae_workspace_bytes = bufs["vae_workspace"].numel()
        return rec, bufs

    def record(self, sample: int = 0) -> dict:
        return dict(super().record(sample), space="image")
