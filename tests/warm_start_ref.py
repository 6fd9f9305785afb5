"""Float64 restatements for the warm-start tests, written from the formulae alone (nothing of ldm3d is imported):

  noised_start     x = a z0 + s e from given coefficients (DDPM / DDIM: a = sqrt(abar_t), s = sqrt(1 - abar_t); flow: a = 1 - tau, s = tau)
  alphas_cumprod   the fp64 beta / alpha-bar table of the "scaled_linear_beta" and "linear_beta" schedules
  reversed_step    MONAI's DDIMScheduler.reversed_step for the three prediction types, with and without the x0 clip
  ddim_step        the deterministic (eta = 0) DDIM step, the inverse walk of reversed_step
  start_step       the strength -> start step map of diffusers' image-to-image pipelines
"""
import numpy as np
import torch


def noised_start(z0: torch.Tensor, eps: torch.Tensor, a: float, s: float) -> torch.Tensor:
    """x[b] = a z0[b or 0] + s eps[b] in float64; z0 [1 or B, ...] broadcasts over eps [B, ...]."""
    return float(a) * z0.double().cpu() + float(s) * eps.double().cpu()


def start_gate(z0: torch.Tensor, eps: torch.Tensor, a: float, s: float, flow: bool) -> torch.Tensor:
    """The per-element bound on |fp32 kernel - noised_start| from the kernel's roundings: the product s e and the fused multiply-add
    round once each, at most 2^-24 relative apiece of |s e| and of |a z0| + |s e| (up to second order): together under
    2^-23 (|a z0| + |s e|).  A flow start forms a = 1 - tau in fp32, one more rounding of at most 2^-24 a <= 2^-24, times |z0|."""
    z, e = z0.double().cpu().abs(), eps.double().cpu().abs()
    gate = 2.0 ** -23 * (abs(float(a)) * z + abs(float(s)) * e)
    return gate + (2.0 ** -24 * z if flow else 0.0)


def alphas_cumprod(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0195) -> np.ndarray:
    if schedule == "scaled_linear_beta":
        betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=np.float64) ** 2
    else:
        betas = np.linspace(beta_start, beta_end, num_train_timesteps, dtype=np.float64)
    return np.cumprod(1.0 - betas)


def coefs(a_t: float, a_to: float):
    """(sqrt(abar_t), sqrt(1 - abar_t), sqrt(abar_to), sqrt(1 - abar_to)) of a step from timestep t to the timestep it lands on."""
    return float(a_t) ** 0.5, (1.0 - float(a_t)) ** 0.5, float(a_to) ** 0.5, (1.0 - float(a_to)) ** 0.5


def reversed_step(pred: str, c, m, x, clip: bool):
    """MONAI's reversed_step from the four coefficients ``c`` (``coefs``, or the fp32 values a kernel was given) -> (post_sample,
    pred_original_sample): x0_hat and eps_hat by prediction type, x0_hat clipped to [-1, 1] when ``clip`` (eps_hat comes from the
    unclipped quantities, as in ``step``), post = sqrt(abar_next) x0_hat + sqrt(1 - abar_next) eps_hat.  m, x: float64 tensors."""
    sa, sb, sn, sbn = (float(v) for v in c)
    if pred == "epsilon":
        x0, eps = (x - sb * m) / sa, m
    elif pred == "sample":
        x0, eps = m, (x - sa * m) / sb
    else:
        assert pred == "v_prediction", pred
        x0, eps = sa * x - sb * m, sa * m + sb * x
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    return sn * x0 + sbn * eps, x0


def ddim_step(pred: str, c, m, x, clip: bool):
    """The eta = 0 DDIM step -> (prev_sample, pred_original_sample): the same formula towards less noise (``c`` ends in the
    coefficients of the PREVIOUS timestep)."""
    return reversed_step(pred, c, m, x, clip)


def start_step(n_steps: int, strength: float) -> int:
    """k0 = n - min(int(n * strength), n): the chain runs its last int(n * strength) steps."""
    return n_steps - min(int(n_steps * strength), n_steps)
