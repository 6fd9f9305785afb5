"""MONAI >= 1.4 ``DiffusionInferer.get_likelihood`` restated on torch CPU (monai/inferers/inferer.py: get_likelihood, _get_decoder_log_likelihood,
_approx_standard_normal_cdf; monai/networks/schedulers/ddpm.py: _get_mean, _get_variance).  MONAI is not installed here: this is written from
its published source, in its op order (the two posterior means are formed and subtracted), with the beta / alpha-bar tables computed in
fp32 exactly as ``ldm3d.schedulers.DDPMScheduler`` computes them.

``dtype=torch.float64`` is the reference the kernels are gated against (the fp32 tables upcast, every tensor op in fp64);
``dtype=torch.float32`` is MONAI's own arithmetic and gives the yardstick error of a correct fp32 evaluation."""
import math

import numpy as np
import torch


class Tables:
    def __init__(self, num_train_timesteps=1000, schedule="linear_beta", beta_start=1e-4, beta_end=2e-2, variance_type="fixed_small",
                 clip_sample=True, prediction_type="epsilon"):
        if schedule == "scaled_linear_beta":
            self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        else:
            self.betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.one = torch.tensor(1.0)
        self.variance_type, self.clip_sample, self.prediction_type = variance_type, clip_sample, prediction_type

    def coefs(self, t, dtype):
        """0-dim tensors of ``dtype`` from the fp32 tables: a, a_prev, beta_t, alpha_t, c0, c1, var (c0 / c1 / var in fp32 op order first,
        as the scheduler tabulates them)."""
        a = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[t - 1] if t > 0 else self.one
        beta_prod, beta_prod_prev = 1 - a, 1 - a_prev
        c0 = (a_prev ** 0.5 * self.betas[t]) / beta_prod
        c1 = self.alphas[t] ** 0.5 * beta_prod_prev / beta_prod
        var = (1 - a_prev) / (1 - a) * self.betas[t]
        var = torch.clamp(var, min=1e-20) if self.variance_type == "fixed_small" else self.betas[t].clone()
        return tuple(v.to(dtype) for v in (a, a_prev, c0, c1, var))


def approx_standard_normal_cdf(x):
    return 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3))))


def x0_hat(tab, a, x_t, m):
    b = 1 - a
    if tab.prediction_type == "epsilon":
        xh = (x_t - b ** 0.5 * m) / a ** 0.5
    elif tab.prediction_type == "sample":
        xh = m
    else:
        xh = a ** 0.5 * x_t - b ** 0.5 * m
    return torch.clamp(xh, -1, 1) if tab.clip_sample else xh


def noisy(tab, t, x0, z, dtype=torch.float64):
    a = tab.alphas_cumprod[t].to(dtype)
    return a ** 0.5 * x0.to(dtype) + (1 - a) ** 0.5 * z.to(dtype)


def term_map(tab, t, x0, x_t, m, bin_width=1.0 / 255.0, dtype=torch.float64, parts=False):
    """The per-element term of timestep t, MONAI's op order, every tensor op in ``dtype``.  ``parts``: also x0_hat, c0, var and (t == 0) cx."""
    x0, x_t, m = x0.to(dtype), x_t.to(dtype), m.to(dtype)
    a, _, c0, c1, var = tab.coefs(t, dtype)
    xh = x0_hat(tab, a, x_t, m)
    mean_p = c0 * xh + c1 * x_t
    mean_q = c0 * x0 + c1 * x_t
    lv_p = lv_q = torch.log(var)
    cx = None
    if t > 0:
        kl = 0.5 * (-1.0 + lv_p - lv_q + torch.exp(lv_q - lv_p) + ((mean_q - mean_p) ** 2) * torch.exp(-lv_p))
    else:
        log_scales = 0.5 * lv_p
        cx = x0 - mean_p
        inv_stdv = torch.exp(-log_scales)
        cdf_plus = approx_standard_normal_cdf(inv_stdv * (cx + bin_width / 2))
        cdf_min = approx_standard_normal_cdf(inv_stdv * (cx - bin_width / 2))
        log_cdf_plus = torch.log(cdf_plus.clamp(min=1e-12))
        log_one_minus_cdf_min = torch.log((1.0 - cdf_min).clamp(min=1e-12))
        cdf_delta = cdf_plus - cdf_min
        log_probs = torch.where(x0 < -0.999, log_cdf_plus,
                                torch.where(x0 > 0.999, log_one_minus_cdf_min, torch.log(cdf_delta.clamp(min=1e-12))))
        kl = -log_probs
    return (kl, dict(x0_hat=xh, c0=c0, var=var, cx=cx)) if parts else kl


def nearest_index(n_in, n_out):
    """PyTorch's nearest source index of every destination index: min(floor(dst * float32(in) / out), in - 1), the scale in fp32."""
    scale = np.float32(n_in) / np.float32(n_out)
    idx = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, n_in - 1)


def resize_nearest(x, size):
    d, h, w = (torch.from_numpy(nearest_index(i, o)) for i, o in zip(x.shape[2:], size))
    return x[:, :, d][:, :, :, h][:, :, :, :, w]
