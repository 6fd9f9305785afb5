"""DPM-Solver++ (2M multistep; ODE and SDE form) in fp64, written independently of ldm3d.schedulers in the op order of diffusers'
``DPMSolverMultistepScheduler`` (restated from its formulae: diffusers is not installed here): per step lambda, h, r, then D0 / D1, then
the update, never a collapsed coefficient.  CPU torch only; the three timestep spacings included.

  alpha_t = sqrt(abar_t), sigma_t = sqrt(1 - abar_t), lambda_t = log(alpha_t) - log(sigma_t)
  after the last timestep the chain goes to sigma = 0, alpha = 1 (final_sigmas_type="zero"), lambda = +inf
  x0_hat: sample m | epsilon (x - sigma_s m) / alpha_s | v_prediction alpha_s x - sigma_s m; then the optional clamp
  first order    ODE  x_t = (sigma_t / sigma_s) x - alpha_t (exp(-h) - 1) D0
                 SDE  x_t = (sigma_t / sigma_s) exp(-h) x + alpha_t (1 - exp(-2h)) D0 + sigma_t sqrt(1 - exp(-2h)) z
  second order   D0 = x0_hat, D1 = (x0_hat - x0_hat_prev) / r, r = (lambda_s - lambda_prev) / h     (midpoint form)
                 ODE  ... - 0.5 alpha_t (exp(-h) - 1) D1        SDE  ... + 0.5 alpha_t (1 - exp(-2h)) D1
  first order when solver_order == 1, on the first step and on the last."""
import math

import numpy as np
import torch


def timesteps(spacing, T, N, steps_offset=0):
    if spacing == "linspace":
        ts = np.round(np.linspace(0, T - 1, N + 1))[::-1][:-1]
    elif spacing == "trailing":
        ts = np.round(np.arange(T, 0, -T / N)) - 1
    elif spacing == "leading":                  # the project's DDIM grid, not diffusers' N + 1-point one
        ts = (np.arange(0, N) * (T // N))[::-1] + steps_offset
    else:
        raise ValueError(spacing)
    return [int(t) for t in ts]


class DPMRef:
    def __init__(self, num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=1e-4, beta_end=2e-2, solver_order=2,
                 algorithm_type="dpmsolver++", timestep_spacing="linspace", prediction_type="epsilon", clip_sample=False,
                 clip_sample_min=-1.0, clip_sample_max=1.0, steps_offset=0):
        T = num_train_timesteps
        # the beta table in fp32 with the op order of the schedulers under test (the abar table is their input, not their arithmetic)
        if schedule == "scaled_linear_beta":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float32) ** 2
        else:
            betas = torch.linspace(beta_start, beta_end, T, dtype=torch.float32)
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0).double()
        self.T, self.order, self.sde = T, solver_order, algorithm_type == "sde-dpmsolver++"
        self.spacing, self.pred, self.offset = timestep_spacing, prediction_type, steps_offset
        self.clip = (clip_sample_min, clip_sample_max) if clip_sample else None
        self.set_timesteps(T // 2 if timestep_spacing != "leading" else T)

    def set_timesteps(self, N):
        self.ts = timesteps(self.spacing, self.T, N, self.offset)
        self.timesteps = torch.tensor(self.ts, dtype=torch.int64)
        self.counter, self.prev_x0 = 0, None

    def alpha_sigma(self, k):
        """(alpha, sigma) of the state before call k; k == len(ts) is the end of the chain"""
        if k >= len(self.ts):
            return 1.0, 0.0
        a = float(self.alphas_cumprod[self.ts[k]])
        return math.sqrt(a), math.sqrt(1.0 - a)

    @staticmethod
    def lam(alpha, sigma):
        return math.inf if sigma == 0.0 else math.log(alpha) - math.log(sigma)

    def convert(self, m, x, k):
        alpha_s, sigma_s = self.alpha_sigma(k)
        if self.pred == "sample":
            x0 = m
        elif self.pred == "epsilon":
            x0 = (x - sigma_s * m) / alpha_s
        else:
            x0 = alpha_s * x - sigma_s * m
        return x0 if self.clip is None else x0.clamp(self.clip[0], self.clip[1])

    def step(self, m, t, x, z=None):
        """-> (x_t, x0_hat); fp64 tensors.  z: the SDE form's draw (ignored where nothing is drawn)."""
        k = self.counter
        assert int(t) == self.ts[k], (t, self.ts[k])
        m, x = m.double(), x.double()
        x0 = self.convert(m, x, k)
        alpha_s, sigma_s = self.alpha_sigma(k)
        alpha_t, sigma_t = self.alpha_sigma(k + 1)
        lam_s, lam_t = self.lam(alpha_s, sigma_s), self.lam(alpha_t, sigma_t)
        h = lam_t - lam_s
        last = k + 1 == len(self.ts)
        first_order = self.order == 1 or k == 0 or last
        D0 = x0
        if self.sde:
            out = (sigma_t / sigma_s * math.exp(-h)) * x + (alpha_t * (1.0 - math.exp(-2.0 * h))) * D0
        else:
            out = (sigma_t / sigma_s) * x - (alpha_t * (math.exp(-h) - 1.0)) * D0
        if not first_order:
            alpha_p, sigma_p = self.alpha_sigma(k - 1)
            h_0 = lam_s - self.lam(alpha_p, sigma_p)
            r = h_0 / h
            D1 = (1.0 / r) * (x0 - self.prev_x0)
            if self.sde:
                out = out + 0.5 * (alpha_t * (1.0 - math.exp(-2.0 * h))) * D1
            else:
                out = out - 0.5 * (alpha_t * (math.exp(-h) - 1.0)) * D1
        if self.sde and not last:
            out = out + sigma_t * math.sqrt(1.0 - math.exp(-2.0 * h)) * z.double()
        self.prev_x0 = x0
        self.counter += 1
        return out, x0
