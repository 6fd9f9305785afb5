"""DDPM / DDIM / PNDM / rectified-flow schedulers with MONAI's interface, element-wise math on the GPU through libldm3d.so.

Mirror of monai.networks.schedulers.{DDPMScheduler, DDIMScheduler} as the reference constructs them
(3d_ldm/train_diffusion.py:140-145, 3d_ldm/inference.py:79-84: T=1000, "scaled_linear_beta", 0.0015 -> 0.0195).
The beta / alpha-bar tables and the per-timestep scalar coefficients are computed on the host in fp32 with the
same torch op order MONAI uses; ``step`` / ``add_noise`` launch one fused element-wise kernel each
(ldm_scheduler_step / ldm_add_noise, include/ldm3d.h).  CUDA tensors only - no CPU fallback.

``prediction_type`` is MONAI's: "epsilon" (the reference's), "sample" (the model predicts x0) or "v_prediction" (the model predicts
v = sqrt(abar_t) eps - sqrt(1 - abar_t) x0, ``get_velocity``).  Every type of DDPM and DDIM steps through ldm_scheduler_step with one
coefficient row (``_row``) by value: the device sampler's own per-element arithmetic on the row the device sampler would read, so the
host-driven ``step`` and ``device_sampler`` agree bit for bit.  The two extra types train on the target of ldm_add_noise_target.

``PNDMScheduler`` (MONAI >= 1.4 monai.networks.schedulers.PNDMScheduler, restated) is the multistep sampler: a Runge-Kutta warm-up (PRK,
4 UNet calls per step for 3 steps) or none (``skip_prk_steps``), then 4th-order linear multistep steps (PLMS), one UNet call each.  Each
UNet call is one row of a coefficient table (``_table``) that says what the step kernel reads, writes and weighs; ``step`` passes the
row by value (ldm_pndm_step) and the device sampler reads it from a device table (ldm_sampler_create_pndm).

``DPMSolverMultistepScheduler`` (diffusers' class of that name, restated) is DPM-Solver++ in its data-prediction form: the 2M multistep
solver or its first-order step, as an ODE solver or with fresh noise every step, one UNet call per step.  Each call is one row
(``_row``: x := cx x + c0 x0_hat + c1 x0_hat_prev + cz z) that ``step`` passes by value (ldm_dpm_step) and the device sampler reads from a
device table (ldm_sampler_create_dpm); the state is the previous x0_hat.

``RFlowScheduler`` (MONAI >= 1.4 monai.networks.schedulers.RFlowScheduler, restated) is rectified flow: a straight noise-to-data path,
trained on the velocity x0 - noise and sampled by 10 - 30 Euler steps; it shares the device sampler, the windowed step and the cached
latent batch with the others through entries of its own (ldm_rflow_*, ldm_sampler_create_rflow, ldm_latent_batch_rflow).

Warm starts: ``DDIMScheduler.reversed_step`` (MONAI's, restated) is one step of DDIM inversion on the same step kernel with the row
``_inversion_row``; ``DeviceSampler.seek`` / ``start`` begin a chain at row k0 from a given latent (ldm_sampler_seek / _start) and
``start_step_for_strength`` maps a strength to k0.

Inpainting: ``repaint_schedule`` / ``repaint_rows`` build the row table of a RePaint chain (non-monotonic timesteps, the known region's and
the jump's coefficients per row), ``RepaintSampler`` (``scheduler.repaint_sampler``) steps it on the device with the known latent and the keep
mask bound to the handle (ldm_sampler_create_repaint / _bind_known), and ``repaint_merge`` is the host-driven merge and jump.

``DeviceLikelihood`` (with ``DDPMScheduler.likelihood_rows``) is the state of ``LatentDiffusionInferer.get_likelihood``'s loop, next to
``DeviceSampler``: a row table, a device step counter and a Philox noise tensor behind ``ldm_likelihood_*`` (DDPM only, as in MONAI).
"""
from __future__ import annotations

import copy
import itertools
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib

# MONAI's prediction_type names -> the type argument of ldm_scheduler_step / ldm_sampler_create / ldm_add_noise_target
PREDICTION_TYPES = {"epsilon": 0, "sample": 1, "v_prediction": 2}
LIK_ROW = 16                                  # floats per row of the likelihood table (include/ldm3d.h LDM_LIK_ROW)


def refuse_multistep(scheduler, inpainting: bool) -> None:
    """The one refusal of a ``multistep`` scheduler: its chain has no warm start, and no inpainting."""
    if not scheduler.multistep:
        return
    name = type(scheduler).__name__
    if inpainting:
        raise NotImplementedError(f"inpainting is not implemented for {name}: its multistep history is not defined across jumps")
    raise NotImplementedError(f"warm starts are not implemented for {name}: its multistep chain is defined from its first timestep")


class _NoisingScheduler:
    """What training and every sampling chain ask of a scheduler, whatever its arithmetic: the noising of a clean sample (``add_noise``
    on the coefficients of ``_noising_coefs``), the device samplers, and what the scheduler says of itself.  A
    subclass provides ``_noising_coefs``, ``add_noise_and_target``, ``step``, ``_table``, ``_create_sampler``, ``_create_repaint_sampler`` and
    ``_latent_batch``."""

    kind: Optional[int] = None                # the sampler kind of the C ABI: 0 DDPM, 1 DDIM, 2 PNDM, 3 rectified flow, 4 DPM-Solver++
    multistep = False                         # ``step`` keeps a history: the device sampler binds state; no warm start, no inpainting
    repaint_kind: Optional[int] = None        # the base step of ldm_sampler_create_repaint: 0 DDPM, 1 DDIM, 2 rectified flow
    measurable = False                        # measurement guidance (guidance.py) is built on this scheduler's single step and x0_hat

    def _noising_args(self, x0, noise, timesteps, what):
        """fp32 contiguous x0 and noise, and the two per-sample coefficient vectors [B] of ``_noising_coefs`` on x0's device."""
        if not x0.is_cuda:
            raise _lib.LdmError(f"{what}: CUDA tensors only (no CPU fallback)")
        a, b = self._noising_coefs(timesteps, x0.device)
        x0c = x0.detach().to(torch.float32).contiguous()
        if a.numel() != x0c.shape[0]:
            raise ValueError(f"{what}: {x0c.shape[0]} samples but {a.numel()} timesteps")
        return x0c, noise.detach().to(device=x0.device, dtype=torch.float32).contiguous(), a, b

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        """a_b x0 + b_b noise with per-sample t: sqrt(abar_t) x0 + sqrt(1 - abar_t) eps (inside inferer.__call__,
        3d_ldm/train_diffusion.py:197-205), rectified flow (1 - tau_b) x0 + tau_b noise."""
        x0c, ec, a, b = self._noising_args(original_samples, noise, timesteps, "add_noise")
        out = torch.empty_like(x0c)
        B = x0c.shape[0]
        with torch.cuda.device(x0c.device):
            _lib.check(_lib.lib().ldm_add_noise(x0c.data_ptr(), ec.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), B,
                                                x0c.numel() // B, _lib.current_stream()))
        return out

    def device_sampler(self, seed: int = 0, eta: float = 0.0) -> "DeviceSampler":
        """The fused, device-resident form of ``step`` over ``self.timesteps`` (see DeviceSampler).  ``seed`` keys the draws of a
        sampler that draws (DDPM, DDIM with ``eta`` > 0, the SDE form of DPM-Solver++); ``eta`` is DDIM's."""
        return DeviceSampler(self, seed, eta)

    def repaint_sampler(self, known: torch.Tensor, keep_mask: torch.Tensor, jump_length: int = 1, n_resample: int = 1,
                        seed: int = 0, eta: float = 0.0) -> "RepaintSampler":
        """The device sampler of an inpainting chain over ``self.timesteps`` (see RepaintSampler): ``known`` [1 or B, C, d, h, w] is the
        scaled latent to keep where ``keep_mask`` [d, h, w] is 1.  ``seed`` keys the step noise and the known-region and jump draws.  A
        ``multistep`` scheduler raises NotImplementedError."""
        return RepaintSampler(self, known, keep_mask, jump_length, n_resample, seed, eta)

    def chain_scheduler(self):
        """The object whose ``step`` drives ONE sampling chain from its first timestep: this scheduler itself where ``step`` keeps
        no state between calls; a ``multistep`` one returns a copy with a fresh state, so that chains never share one."""
        if not self.multistep:
            return self
        sch = copy.copy(self)
        sch.reset_state()
        return sch

    def _step_kwargs(self, ts: list, k: int) -> dict:
        """What a host-driven ``step`` number k over the timesteps ``ts`` takes beside (model_output, timestep, sample)."""
        return {}

    @staticmethod
    def _draw(model_output: torch.Tensor, generator: Optional[torch.Generator]) -> torch.Tensor:
        # MONAI draws with the generator's device and moves to the sample; a None / CUDA generator draws in place.
        if generator is not None and generator.device.type == "cpu":
            return torch.randn(model_output.size(), dtype=torch.float32, generator=generator).to(model_output.device)
        return torch.randn(model_output.size(), dtype=torch.float32, device=model_output.device, generator=generator)


class _Scheduler(_NoisingScheduler):
    """The schedulers on a beta schedule: the abar tables, ``prediction_type`` and the variance-preserving noising."""

    def __init__(self, num_train_timesteps: int = 1000, schedule: str = "linear_beta", beta_start: float = 1e-4,
                 beta_end: float = 2e-2, clip_sample: bool = True, prediction_type: str = "epsilon"):
        if prediction_type not in PREDICTION_TYPES:
            raise ValueError(f"prediction_type given as {prediction_type!r} must be one of {list(PREDICTION_TYPES)}")
        self.num_train_timesteps = num_train_timesteps
        self.prediction_type = prediction_type
        self._pred = PREDICTION_TYPES[prediction_type]
        self.clip_sample = clip_sample
        if schedule == "scaled_linear_beta":
            self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif schedule == "linear_beta":
            self.betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise NotImplementedError(f"schedule '{schedule}' is not used by the reference")
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.one = torch.tensor(1.0)
        self.num_inference_steps = num_train_timesteps
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy())
        self._sqrt_ac = self.alphas_cumprod ** 0.5
        self._sqrt_1mac = (1 - self.alphas_cumprod) ** 0.5
        # the two extra coefficients of the sample / v_prediction step, per t: sqrt(abar_t) and 1 / sqrt(1 - abar_t) (a multiply by
        # the reciprocal stands in for MONAI's divide, <= 1 ulp)
        self._sqrt_a = self._sqrt_ac.tolist()
        self._inv_sqrt_b = (1.0 / self._sqrt_1mac).tolist()
        self._dev_tables = {}

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        if num_inference_steps > self.num_train_timesteps:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                             f"`self.num_train_timesteps`: {self.num_train_timesteps}")
        self.num_inference_steps = num_inference_steps
        step_ratio = self.num_train_timesteps // self.num_inference_steps
        ts = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.int64)
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)
        self._on_set_timesteps()

    def _on_set_timesteps(self):
        pass

    def _noising_coefs(self, timesteps, dev):
        """The per-sample sqrt(abar_t), sqrt(1 - abar_t) [B], gathered on ``dev`` from the device copies of the tables: no host read of
        the timesteps."""
        tab = self._dev_tables.get(dev)
        if tab is None:
            tab = (self._sqrt_ac.to(dev), self._sqrt_1mac.to(dev))
            self._dev_tables[dev] = tab
        t = timesteps.to(device=dev, dtype=torch.long).reshape(-1)
        return tab[0][t].contiguous(), tab[1][t].contiguous()

    def _noise_and_target(self, x0, noise, timesteps, noisy: bool):
        x0c, ec, sa, sb = self._noising_args(x0, noise, timesteps, "get_velocity" if not noisy else "add_noise_and_target")
        out = torch.empty_like(x0c) if noisy else None
        target = torch.empty_like(x0c)
        B = x0c.shape[0]
        pred = PREDICTION_TYPES["v_prediction"] if not noisy else self._pred
        with torch.cuda.device(x0c.device):
            _lib.check(_lib.lib().ldm_add_noise_target(x0c.data_ptr(), ec.data_ptr(), sa.data_ptr(), sb.data_ptr(), _lib.ptr(out),
                                                       target.data_ptr(), B, x0c.numel() // B, pred, _lib.current_stream()))
        return out, target

    def get_velocity(self, sample: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        """v = sqrt(abar_t) noise - sqrt(1 - abar_t) sample with per-sample t: the v_prediction training target (MONAI's
        Scheduler.get_velocity)."""
        return self._noise_and_target(sample, noise, timesteps, noisy=False)[1]

    def add_noise_and_target(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor
                             ) -> Tuple[torch.Tensor, torch.Tensor]:
        """(add_noise(x0, noise, t), the regression target of this scheduler's prediction_type): the target is ``noise`` itself for
        "epsilon" (the reference's add_noise, unchanged), ``x0`` for "sample" and get_velocity(x0, noise, t) for "v_prediction"; the
        two extra types write both in one kernel pass (ldm_add_noise_target)."""
        if self._pred == PREDICTION_TYPES["epsilon"]:
            return self.add_noise(original_samples=original_samples, noise=noise, timesteps=timesteps), noise
        return self._noise_and_target(original_samples, noise, timesteps, noisy=True)

    def _step(self, model_output, timestep, sample, eta: float, noisy: bool, generator, noise):
        """``step`` of DDPM and DDIM -> (x_{t-1}, x0_hat): ldm_scheduler_step with the sampler row of the timestep (``_row``) by value.
        z is ``noise`` or a torch.randn draw where the step is ``noisy``, absent (sigma = 0) otherwise."""
        import ctypes as C
        if not sample.is_cuda:
            raise _lib.LdmError(f"{type(self).__name__}.step: CUDA tensors only (no CPU fallback)")
        m = model_output.detach().to(torch.float32).contiguous()
        x = sample.detach().to(torch.float32).contiguous()
        z = None
        if noisy:
            z = noise if noise is not None else self._draw(m, generator)
            z = z.to(device=x.device, dtype=torch.float32).contiguous()
        row = (C.c_float * 8)(*self._row(int(timestep), eta))
        prev = torch.empty_like(x)
        x0 = torch.empty_like(x)
        with torch.cuda.device(x.device):
            # x0 = (x - sqrt_b eps) / sqrt_a is evaluated as a multiply by 1/sqrt_a (<= 1 ulp from MONAI's divide)
            _lib.check(_lib.lib().ldm_scheduler_step(m.data_ptr(), x.data_ptr(), _lib.ptr(z), prev.data_ptr(), x0.data_ptr(), x.numel(),
                                                     self.kind, self._pred, row, int(self.clip_sample), _lib.current_stream()))
        return prev, x0

    def _table(self, eta: float = 0.0) -> list:
        """The device sampler's coefficient table (host only, no device work): one 8-float row per step in sampling order,
        {1/sqrt(abar_t), sqrt(1 - abar_t), c0, c1 (DDPM) | dir (DDIM), sigma, t, sqrt(abar_t), 1/sqrt(1 - abar_t)}, exactly the row ``step``
        passes by value (the last two are read by the sample / v_prediction kernels only).  PNDM and DPM-Solver++ have their own."""
        return [self._row(int(t), eta) for t in self.timesteps.tolist()]

    def _create_sampler(self, coef: int, n_rows: int, seed: int, handle) -> int:
        """The ``ldm_sampler_create*`` entry of this class on a device table of ``_table``'s layout: the status."""
        return _lib.lib().ldm_sampler_create(coef, n_rows, self.kind, self._pred, int(self.clip_sample), seed, handle)

    def _latent_batch(self, head: tuple, tail: tuple) -> int:
        """``LatentCache.batch``'s launch for this scheduler's regression target (``head`` ends with the two ``_noising_coefs``)."""
        return _lib.lib().ldm_latent_batch(*head, self._pred, *tail)

    def _create_repaint_sampler(self, coef: int, n_rows: int, seed: int, handle) -> int:
        """ldm_sampler_create_repaint on a device table of ``repaint_rows``: the status, the handle written through ``handle``."""
        return _lib.lib().ldm_sampler_create_repaint(coef, n_rows, self.repaint_kind, self._pred, int(self.clip_sample), seed, handle)

    def _repaint_marginals(self) -> list:
        """The marginal of the state at every level 0 .. n of a chain over ``self.timesteps``, as Python floats (fp64): abar (tau for
        rectified flow).  Level 0 is the first timestep's own; level L + 1 is where ``step`` at ``timesteps[L]`` arrives
        (``_prev_alpha_cumprod``: the one place that says so)."""
        ts = self.timesteps.tolist()
        return [float(self.alphas_cumprod[int(ts[0])])] + [float(self._prev_alpha_cumprod(int(t))) for t in ts]

    @staticmethod
    def _repaint_coefs(m_a: float, m_b: Optional[float] = None) -> tuple:
        """(ka, ks, ja, js) of ``repaint_rows`` at a level of marginal ``m_a``, jumping back to the level of ``m_b`` (None: no jump)."""
        ratio = 1.0 if m_b is None else m_b / m_a
        return m_a ** 0.5, (1.0 - m_a) ** 0.5, ratio ** 0.5, max(1.0 - ratio, 0.0) ** 0.5


class DDPMScheduler(_Scheduler):
    """variance_type fixed_small / fixed_large, clip_sample=True (MONAI default, not overridden by the reference)."""

    kind = repaint_kind = 0
    measurable = True

    def __init__(self, num_train_timesteps: int = 1000, schedule: str = "linear_beta", variance_type: str = "fixed_small",
                 clip_sample: bool = True, prediction_type: str = "epsilon", **schedule_args):
        super().__init__(num_train_timesteps, schedule, clip_sample=clip_sample, prediction_type=prediction_type,
                         **schedule_args)
        if variance_type not in ("fixed_small", "fixed_large"):
            raise NotImplementedError("learned variance is not on the reference's path")
        self.variance_type = variance_type
        ac = self.alphas_cumprod
        ac_prev = self._ac_prev = torch.cat([self.one.reshape(1), ac[:-1]])
        beta_prod = 1 - ac
        beta_prod_prev = 1 - ac_prev
        self._inv_sqrt_a = (1.0 / ac ** 0.5).tolist()
        self._sqrt_b = (beta_prod ** 0.5).tolist()
        self._c0 = ((ac_prev ** 0.5 * self.betas) / beta_prod).tolist()
        self._c1 = (self.alphas ** 0.5 * beta_prod_prev / beta_prod).tolist()
        var = (1 - ac_prev) / (1 - ac) * self.betas
        var = torch.clamp(var, min=1e-20) if variance_type == "fixed_small" else self.betas.clone()
        self._sigma = (var ** 0.5).tolist()
        self._var = var

    def likelihood_rows(self) -> list:
        """The coefficient table of ``get_likelihood`` over ``self.timesteps`` (ldm_likelihood_create; host only): one LIK_ROW-float row
        per timestep, {sqrt(abar_t), sqrt(1 - abar_t), 1/sqrt(abar_t), c0, 1/var, t, 1/sqrt(var), c1, 0 ...} with the sampler's own
        fp32 coefficients and var the step's fixed variance (fixed_small: clamped at 1e-20, so 1/var(0) = 1e20).  1/var = exp(-log var)
        and 1/sqrt(var) = exp(-log(var) / 2) are formed in fp64 from the fp32 table and rounded once."""
        var = self._var.to(torch.float64)
        inv_var, inv_std = (1.0 / var).to(torch.float32).tolist(), (1.0 / var.sqrt()).to(torch.float32).tolist()
        return [[self._sqrt_a[t], self._sqrt_b[t], self._inv_sqrt_a[t], self._c0[t], inv_var[t], float(t), inv_std[t], self._c1[t]]
                + [0.0] * (LIK_ROW - 8) for t in (int(t) for t in self.timesteps.tolist())]

    def _prev_alpha_cumprod(self, t: int) -> torch.Tensor:
        """abar of the state ``step`` at timestep t arrives at: abar[t - 1], 1 at t = 0 (the table c0 / c1 / sigma are built from)."""
        return self._ac_prev[t]

    def _row(self, t: int, eta: float = 0.0) -> list:
        """The device sampler's coefficient row of timestep t (see ``_table``); eta is DDIM's and ignored here."""
        return [self._inv_sqrt_a[t], self._sqrt_b[t], self._c0[t], self._c1[t], self._sigma[t] if t > 0 else 0.0, float(t),
                self._sqrt_a[t], self._inv_sqrt_b[t]]

    def step(self, model_output: torch.Tensor, timestep: int, sample: torch.Tensor,
             generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None
             ) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (x_{t-1}, x0_hat).  ``noise`` (extension) supplies z explicitly; otherwise torch.randn."""
        return self._step(model_output, timestep, sample, 0.0, int(timestep) > 0, generator, noise)


class DDIMScheduler(_Scheduler):
    """eta = 0 by default, set_alpha_to_one=True, steps_offset=0 (MONAI defaults; BASELINE configs 1 and 5)."""

    kind = repaint_kind = 1
    measurable = True

    def __init__(self, num_train_timesteps: int = 1000, schedule: str = "linear_beta", clip_sample: bool = True,
                 set_alpha_to_one: bool = True, steps_offset: int = 0, prediction_type: str = "epsilon", **schedule_args):
        super().__init__(num_train_timesteps, schedule, clip_sample=clip_sample, prediction_type=prediction_type,
                         **schedule_args)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        # abar beyond the last training timestep, read by ``reversed_step`` alone: 0 = pure noise (MONAI's first_alpha_cumprod, restated;
        # not pinned against a MONAI install)
        self.first_alpha_cumprod = torch.tensor(0.0)
        self.steps_offset = steps_offset

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        super().set_timesteps(num_inference_steps, device)
        if self.steps_offset:
            self.timesteps = self.timesteps + self.steps_offset

    def _inversion_row(self, t: int) -> list:
        """The sampler row of ``reversed_step`` at timestep t: ``_row(t)`` with abar_next = abar[t + T // n] (``first_alpha_cumprod``
        beyond the table) where abar_prev stands, and sigma = 0.  A DDIM step is prev = c0 x0_hat + c1 eps_hat + sigma z with c0 =
        sqrt(abar_prev), c1 = sqrt(1 - abar_prev - sigma^2); the reversed step is the same formula towards more noise, so the step
        kernels take this row as they take any DDIM row."""
        nxt = t + self.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_next = self.alphas_cumprod[nxt] if nxt < self.num_train_timesteps else self.first_alpha_cumprod
        return [float(1.0 / a_t ** 0.5), float((1 - a_t) ** 0.5), float(a_next ** 0.5), float((1 - a_next) ** 0.5), 0.0, float(t),
                self._sqrt_a[t], self._inv_sqrt_b[t]]

    def reversed_step(self, model_output: torch.Tensor, timestep: int, sample: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """MONAI's ``DDIMScheduler.reversed_step`` (restated): one step of DDIM inversion, from ``sample`` at ``timestep`` to the next
        noisier timestep t + T // n -> (post_sample, pred_original_sample).  x0_hat and eps_hat by prediction type as ``step`` forms them
        (x0_hat clipped when ``clip_sample``), post = sqrt(abar_next) x0_hat + sqrt(1 - abar_next) eps_hat: ldm_scheduler_step with the
        row ``_inversion_row(timestep)``."""
        import ctypes as C
        if not sample.is_cuda:
            raise _lib.LdmError("DDIMScheduler.reversed_step: CUDA tensors only (no CPU fallback)")
        m = model_output.detach().to(torch.float32).contiguous()
        x = sample.detach().to(torch.float32).contiguous()
        row = (C.c_float * 8)(*self._inversion_row(int(timestep)))
        post, x0 = torch.empty_like(x), torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().ldm_scheduler_step(m.data_ptr(), x.data_ptr(), None, post.data_ptr(), x0.data_ptr(), x.numel(),
                                                     self.kind, self._pred, row, int(self.clip_sample), _lib.current_stream()))
        return post, x0

    def inversion_timesteps(self, n_steps: Optional[int] = None) -> list:
        """The timesteps the first ``n_steps`` reversed steps start from (default: all): ``reversed(timesteps)[:n_steps]``."""
        ts = [int(t) for t in self.timesteps.tolist()][::-1]
        n = len(ts) if n_steps is None else int(n_steps)
        if not 1 <= n <= len(ts):
            raise ValueError(f"n_steps must be in [1, {len(ts)}], got {n_steps}")
        return ts[:n]

    def inversion_sampler(self, n_steps: Optional[int] = None, eta: float = 0.0) -> "DeviceSampler":
        """The device-resident form of ``reversed_step`` over ``inversion_timesteps(n_steps)``: a DeviceSampler on the ascending rows
        ``_inversion_row(t)``.  Inversion is defined for the deterministic sampler: ``eta`` must be 0."""
        if float(eta) != 0.0:
            raise ValueError(f"DDIM inversion needs the deterministic sampler (eta = 0), got eta = {eta}")
        return DeviceSampler(self, rows=[self._inversion_row(t) for t in self.inversion_timesteps(n_steps)])

    def _prev_alpha_cumprod(self, t: int) -> torch.Tensor:
        """abar of the state ``step`` at timestep t arrives at: abar[t - T // n], ``final_alpha_cumprod`` past the table's start."""
        prev_t = t - self.num_train_timesteps // self.num_inference_steps
        return self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod

    def _row(self, t: int, eta: float = 0.0) -> list:
        """The device sampler's coefficient row of timestep t (see ``_table``), in MONAI's op order on the fp32 tables."""
        a_t = self.alphas_cumprod[t]
        a_prev = self._prev_alpha_cumprod(t)
        var = (1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)
        std = eta * var ** 0.5
        return [float(1.0 / a_t ** 0.5), float((1 - a_t) ** 0.5), float(a_prev ** 0.5), float((1 - a_prev - std ** 2) ** 0.5),
                float(std), float(t), self._sqrt_a[t], self._inv_sqrt_b[t]]

    def step(self, model_output: torch.Tensor, timestep: int, sample: torch.Tensor, eta: float = 0.0,
             generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None
             ) -> Tuple[torch.Tensor, torch.Tensor]:
        return self._step(model_output, timestep, sample, eta, eta > 0, generator, noise)


# bits of a PNDM row's flags (include/ldm3d.h LDM_PNDM_*)
PNDM_ROW, PNDM_PUSH, PNDM_SAVE, PNDM_USE_SAVED, PNDM_ACC_SET, PNDM_ACC_ADD = 16, 1, 2, 4, 8, 16
# e of a PLMS step as weights on the history after the push, latest first (Adams-Bashforth orders 1..4)
_PLMS_WEIGHTS = {1: (1.0,), 2: (3 / 2, -1 / 2), 3: (23 / 12, -16 / 12, 5 / 12), 4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}


class PNDMScheduler(_Scheduler):
    """MONAI's PNDMScheduler (pseudo numerical methods for diffusion models): ``skip_prk_steps=False`` runs the Runge-Kutta warm-up
    (12 UNet calls) before the linear multistep steps, ``True`` is PLMS alone.  No clipping, no noise; prediction_type "epsilon" or
    "v_prediction".  ``step`` is stateful like MONAI's (``ets``, ``cur_sample``, ``cur_model_output``: CUDA tensors; ``counter``: the
    number of calls made, which selects the row) and ``len(timesteps)`` is the number of UNet calls of a chain: call ``set_timesteps``
    (or ``reset_state``) before each chain that ``step`` drives; ``LatentDiffusionInferer`` does."""

    kind = 2
    multistep = True
    pndm_order = 4

    def __init__(self, num_train_timesteps: int = 1000, schedule: str = "linear_beta", skip_prk_steps: bool = False,
                 set_alpha_to_one: bool = False, prediction_type: str = "epsilon", steps_offset: int = 0, **schedule_args):
        if prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"PNDMScheduler: prediction_type given as {prediction_type!r} must be 'epsilon' or 'v_prediction'")
        super().__init__(num_train_timesteps, schedule, clip_sample=False, prediction_type=prediction_type, **schedule_args)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.skip_prk_steps = skip_prk_steps
        self.steps_offset = steps_offset
        self.set_timesteps(num_train_timesteps)

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        if num_inference_steps > self.num_train_timesteps:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                             f"`self.num_train_timesteps`: {self.num_train_timesteps}")
        ratio = self.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round().astype(np.int64) + self.steps_offset
        if self.skip_prk_steps:
            prk = np.array([], dtype=np.int64)
            plms = np.concatenate([ts[:-1], ts[-2:-1], ts[-1:]])[::-1].copy()
        else:
            if num_inference_steps < self.pndm_order:
                raise ValueError(f"PNDMScheduler with the PRK warm-up needs num_inference_steps >= {self.pndm_order}, got "
                                 f"{num_inference_steps}")
            p = np.array(ts[-self.pndm_order:]).repeat(2) + np.tile(np.array([0, ratio // 2]), self.pndm_order)
            prk = (p[:-1].repeat(2)[1:-1])[::-1].copy()
            plms = ts[:-3][::-1].copy()
        self.num_inference_steps = num_inference_steps
        self._ts = ts
        self.prk_timesteps, self.plms_timesteps = prk, plms
        all_ts = np.concatenate([prk, plms]).astype(np.int64)
        self.timesteps = torch.from_numpy(all_ts).to(device) if device is not None else torch.from_numpy(all_ts)
        self.reset_state()

    def reset_state(self) -> None:
        """The multistep state of a chain that has not started (what ``set_timesteps`` leaves)."""
        self.ets: List[torch.Tensor] = []
        self.counter = 0
        self.cur_sample = None
        self.cur_model_output = 0

    def _transfer(self, t: int, prev_t: int):
        """-> (cx, ce, sqrt(a), sqrt(b)) of prev = cx x + ce e in fp64 (MONAI's _get_prev_sample: formula (9) of the PNDM paper)."""
        a = float(self.alphas_cumprod[t])
        a_prev = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else float(self.final_alpha_cumprod)
        b, b_prev = 1.0 - a, 1.0 - a_prev
        return ((a_prev / a) ** 0.5, -(a_prev - a) / (a * b_prev ** 0.5 + (a * b * a_prev) ** 0.5), a ** 0.5, b ** 0.5)

    def _row(self, counter: int, t: int, n_hist: int, head: int = 0) -> list:
        """The PNDM_ROW coefficients of call number ``counter`` at timestep ``t`` with ``n_hist`` model outputs in the history (see
        csrc/norm_elem.h): {cx, ce, sqrt(abar), sqrt(1 - abar), flags, t, wm, w1, w2, w3, wacc, am, head, 0, 0, 0}."""
        ratio = self.num_train_timesteps // self.num_inference_steps
        t_unet = t
        wm, w, wacc, am, flags = 0.0, [0.0, 0.0, 0.0], 0.0, 0.0, 0
        if counter < len(self.prk_timesteps):
            prev_t = t - (0 if counter % 2 else ratio // 2)
            t_eff = int(self.prk_timesteps[counter // 4 * 4])
            phase = counter % 4
            if phase == 0:                    # acc = m / 6 (it was 0); ets.append(m); cur_sample = x; e = m
                wm, am, flags = 1.0, 1 / 6, PNDM_ACC_SET | PNDM_PUSH | PNDM_SAVE
            elif phase < 3:                   # acc += m / 3; e = m
                wm, am, flags = 1.0, 1 / 3, PNDM_ACC_ADD | PNDM_USE_SAVED
            else:                             # e = acc + m / 6; the next phase 0 overwrites acc, which stands for acc = 0
                wm, wacc, flags = 1 / 6, 1.0, PNDM_USE_SAVED
        else:
            prev_t = t - ratio
            push = counter != 1
            if push:
                n_after = min(n_hist, 3) + 1
                flags |= PNDM_PUSH
            else:                             # the repeated timestep of the PLMS-only schedule: the second half of a Heun-like step
                prev_t, t, n_after = t, t + ratio, n_hist
            t_eff = t
            if n_after == 1 and counter == 0:
                wm = 1.0
                flags |= PNDM_SAVE
            elif n_after == 1 and counter == 1:
                wm, w[0] = 0.5, 0.5
                flags |= PNDM_USE_SAVED
            elif n_after >= 2 and push:
                wl = _PLMS_WEIGHTS[n_after]
                wm, w[:len(wl) - 1] = wl[0], wl[1:]
            elif 2 <= n_after <= 3:
                w[:n_after] = _PLMS_WEIGHTS[n_after]
            else:
                raise ValueError(f"PNDMScheduler.step: call {counter} with {n_hist} model outputs in the history is no state of a "
                                 "PNDM chain (set_timesteps starts one)")
        cx, ce, sa, sb = self._transfer(t_eff, prev_t)
        return [cx, ce, sa, sb, float(flags), float(t_unet), wm, w[0], w[1], w[2], wacc, am, float(head), 0.0, 0.0, 0.0]

    def _table(self, eta: float = 0.0) -> list:
        """One PNDM_ROW-float row per UNet call over ``self.timesteps``: the table the device sampler reads (host only, no device work;
        ``eta`` is ignored)."""
        rows, n_hist, head = [], 0, 0
        for k, t in enumerate(self.timesteps.tolist()):
            r = self._row(k, int(t), n_hist, head)
            rows.append(r)
            if int(r[4]) & PNDM_PUSH:
                n_hist, head = (n_hist + 1 if k < len(self.prk_timesteps) else min(n_hist, 3) + 1), head + 1
        return rows

    def _create_sampler(self, coef: int, n_rows: int, seed: int, handle) -> int:
        return _lib.lib().ldm_sampler_create_pndm(coef, n_rows, self._pred, handle)

    def step(self, model_output: torch.Tensor, timestep: int, sample: torch.Tensor, generator=None, noise=None
             ) -> Tuple[torch.Tensor, None]:
        """-> (prev_sample, None): ``step_prk`` while ``counter < len(prk_timesteps)``, then ``step_plms``.  ``generator`` / ``noise``
        are accepted for the other schedulers' call shape and unused: PNDM draws nothing."""
        import ctypes as C
        if not sample.is_cuda:
            raise _lib.LdmError("PNDMScheduler.step: CUDA tensors only (no CPU fallback)")
        m = model_output.detach().to(torch.float32).contiguous()
        x = sample.detach().to(torch.float32).contiguous()
        prk = self.counter < len(self.prk_timesteps)
        row = self._row(self.counter, int(timestep), len(self.ets))
        flags = int(row[4])
        hist = [self.ets[-j].detach().to(device=x.device, dtype=torch.float32).contiguous()
                if len(self.ets) >= j and row[6 + j] != 0.0 else None for j in (1, 2, 3)]
        if any(h is None and row[7 + j] != 0.0 for j, h in enumerate(hist)):
            raise ValueError(f"PNDMScheduler.step: call {self.counter} needs more history than the {len(self.ets)} outputs kept")
        saved = None
        if flags & PNDM_USE_SAVED:
            if self.cur_sample is None:
                raise ValueError(f"PNDMScheduler.step: call {self.counter} continues a step whose first call was never made")
            saved = self.cur_sample.detach().to(device=x.device, dtype=torch.float32).contiguous()
        acc_in = acc_out = None
        if row[10] != 0.0 or flags & PNDM_ACC_ADD:
            if not torch.is_tensor(self.cur_model_output):
                raise ValueError(f"PNDMScheduler.step: call {self.counter} reads a Runge-Kutta accumulator that was never started")
            acc_in = self.cur_model_output.detach().to(device=x.device, dtype=torch.float32).contiguous()
        if flags & (PNDM_ACC_SET | PNDM_ACC_ADD):
            acc_out = torch.empty_like(x)
        prev = torch.empty_like(x)
        crow = (C.c_float * PNDM_ROW)(*row)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().ldm_pndm_step(m.data_ptr(), x.data_ptr(), _lib.ptr(hist[0]), _lib.ptr(hist[1]), _lib.ptr(hist[2]),
                                                _lib.ptr(saved), _lib.ptr(acc_in), _lib.ptr(acc_out), prev.data_ptr(), x.numel(),
                                                self._pred, crow, _lib.current_stream()))
        if flags & PNDM_PUSH:                 # a copy: the model's output buffer may be overwritten by its next forward (graph replay)
            keep = m.clone() if m.data_ptr() == model_output.data_ptr() else m
            self.ets = (self.ets if prk else self.ets[-3:]) + [keep]
        if flags & PNDM_SAVE:
            self.cur_sample = x
        elif not prk and flags & PNDM_USE_SAVED:
            self.cur_sample = None
        if acc_out is not None:
            self.cur_model_output = acc_out
        elif row[10] != 0.0:
            self.cur_model_output = 0
        self.counter += 1
        return prev, None


# floats per row of a DPM-Solver++ table and the bits of its flags (include/ldm3d.h LDM_DPM_*)
DPM_ROW, DPM_HAS_PREV, DPM_DRAWS, DPM_CLIP = 16, 1, 2, 4
DPM_ALGORITHMS = ("dpmsolver++", "sde-dpmsolver++")
DPM_SPACINGS = ("linspace", "leading", "trailing")


class DPMSolverMultistepScheduler(_Scheduler):
    """diffusers' ``DPMSolverMultistepScheduler`` restated from its formulae (not pinned against a diffusers
    install): DPM-Solver++ in the data-prediction form, the 2M multistep solver (``solver_order=2``, midpoint form) or its first-order
    step alone (``solver_order=1``), as an ODE solver (``algorithm_type="dpmsolver++"``) or with fresh noise every step
    (``"sde-dpmsolver++"``).  One UNet call per step; every ``prediction_type``; ``clip_sample`` (default off) clamps x0_hat to
    [``clip_sample_min``, ``clip_sample_max``] before it is used and before it is kept.

      alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = ln alpha - ln sigma;  a step s -> t has h = lambda_t - lambda_s
      first order    x := (sigma_t / sigma_s) x + alpha_t (1 - e^-h) x0_hat                                     (ODE)
                     x := (sigma_t / sigma_s) e^-h x + alpha_t (1 - e^-2h) x0_hat + sigma_t sqrt(1 - e^-2h) z   (SDE)
      second order   x0_hat is replaced by x0_hat + (x0_hat - x0_hat_prev) / (2 r),  r = (lambda_s - lambda_prev) / h
      a step is first order when ``solver_order`` is 1, on the first step (no history) and on the last, which goes to sigma = 0,
      alpha = 1 (``final_sigmas_type="zero"``): x := x0_hat, nothing drawn.

    ``timestep_spacing`` for N steps, T = ``num_train_timesteps``: "linspace" = round(linspace(0, T - 1, N + 1))[::-1][:-1], "trailing" =
    round(arange(T, 0, -T / N)) - 1, and "leading" = THIS PROJECT'S DDIM grid (arange(N) * (T // N))[::-1] + ``steps_offset``, which
    deliberately differs from diffusers' N + 1-point leading grid so that order 1 is DDIMScheduler (eta = 0, unclipped,
    set_alpha_to_one) on identical timesteps.

    All of this is folded on the host, in fp64, into one row per call (``_row``): x := cx x + c0 x0_hat + c1 x0_hat_prev + cz z.  ``step``
    passes the row by value (ldm_dpm_step), the device sampler reads it from a device table (ldm_sampler_create_dpm).  ``step`` is
    stateful (``prev_x0``: the previous x0_hat, a CUDA tensor; ``counter``: the number of calls made, which selects the row): call
    ``set_timesteps`` (or ``reset_state``) before each chain that ``step`` drives; ``LatentDiffusionInferer`` does.

    Not built (each raises, naming itself): ``solver_order=3``, ``algorithm_type`` "dpmsolver" / "sde-dpmsolver", ``solver_type="heun"``,
    Karras / exponential / beta sigmas, dynamic thresholding, ``final_sigmas_type="sigma_min"``, ``lower_order_final=False``.  No image
    quality is measured anywhere here: whether fewer steps suffice is a property of a trained model."""

    kind = 4
    multistep = True

    def __init__(self, num_train_timesteps: int = 1000, schedule: str = "linear_beta", solver_order: int = 2,
                 algorithm_type: str = "dpmsolver++", timestep_spacing: str = "linspace", prediction_type: str = "epsilon",
                 clip_sample: bool = False, clip_sample_min: float = -1.0, clip_sample_max: float = 1.0, steps_offset: int = 0,
                 solver_type: str = "midpoint", final_sigmas_type: str = "zero", thresholding: bool = False,
                 use_karras_sigmas: bool = False, use_exponential_sigmas: bool = False, use_beta_sigmas: bool = False,
                 lower_order_final: bool = True, **schedule_args):
        if solver_order not in (1, 2):
            if solver_order == 3:
                raise NotImplementedError("DPMSolverMultistepScheduler: solver_order=3 is not built (orders 1 and 2 are)")
            raise ValueError(f"DPMSolverMultistepScheduler: solver_order given as {solver_order!r} must be 1 or 2")
        if algorithm_type not in DPM_ALGORITHMS:
            if algorithm_type in ("dpmsolver", "sde-dpmsolver"):
                raise NotImplementedError(f"DPMSolverMultistepScheduler: algorithm_type {algorithm_type!r} (the noise-prediction form) is "
                                          f"not built; {list(DPM_ALGORITHMS)} are")
            raise ValueError(f"DPMSolverMultistepScheduler: algorithm_type given as {algorithm_type!r} must be one of {list(DPM_ALGORITHMS)}")
        if timestep_spacing not in DPM_SPACINGS:
            raise ValueError(f"DPMSolverMultistepScheduler: timestep_spacing given as {timestep_spacing!r} must be one of {list(DPM_SPACINGS)}")
        if solver_type != "midpoint":
            if solver_type == "heun":
                raise NotImplementedError("DPMSolverMultistepScheduler: solver_type='heun' is not built (the midpoint form is)")
            raise ValueError(f"DPMSolverMultistepScheduler: solver_type given as {solver_type!r} must be 'midpoint'")
        if final_sigmas_type != "zero":
            if final_sigmas_type == "sigma_min":
                raise NotImplementedError("DPMSolverMultistepScheduler: final_sigmas_type='sigma_min' is not built (the chain ends at sigma = 0)")
            raise ValueError(f"DPMSolverMultistepScheduler: final_sigmas_type given as {final_sigmas_type!r} must be 'zero'")
        for name, on in (("thresholding (dynamic thresholding)", thresholding), ("use_karras_sigmas", use_karras_sigmas),
                         ("use_exponential_sigmas", use_exponential_sigmas), ("use_beta_sigmas", use_beta_sigmas)):
            if on:
                raise NotImplementedError(f"DPMSolverMultistepScheduler: {name} is not built")
        if not lower_order_final:
            raise NotImplementedError("DPMSolverMultistepScheduler: lower_order_final=False is not built (the last step is first order)")
        if not float(clip_sample_min) <= float(clip_sample_max):
            raise ValueError(f"DPMSolverMultistepScheduler: clip_sample_min {clip_sample_min} above clip_sample_max {clip_sample_max}")
        super().__init__(num_train_timesteps, schedule, clip_sample=bool(clip_sample), prediction_type=prediction_type, **schedule_args)
        self.solver_order, self.algorithm_type, self.timestep_spacing = int(solver_order), algorithm_type, timestep_spacing
        self.clip_sample_min, self.clip_sample_max = float(clip_sample_min), float(clip_sample_max)
        self.steps_offset = int(steps_offset)
        # half the logit of abar, fp64 from the fp32 table: lambda_t = ln(alpha_t / sigma_t)
        ac = self.alphas_cumprod.to(torch.float64)
        self._lambda = (0.5 * (torch.log(ac) - torch.log1p(-ac))).tolist()
        self._ac64 = ac.tolist()
        self.set_timesteps(max(1, min(20, self.num_train_timesteps // 2)))      # a placeholder grid until the caller sets its own

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        T, N = self.num_train_timesteps, int(num_inference_steps)
        if N > T:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than `self.num_train_timesteps`: {T}")
        if N < 1:
            raise ValueError(f"`num_inference_steps` must be at least 1, got {num_inference_steps}")
        if self.timestep_spacing == "linspace":
            ts = np.round(np.linspace(0, T - 1, N + 1))[::-1][:-1]
        elif self.timestep_spacing == "trailing":
            ts = np.round(np.arange(T, 0, -T / N)) - 1
        else:
            ts = (np.arange(0, N) * (T // N))[::-1] + self.steps_offset
        ts = np.ascontiguousarray(ts).astype(np.int64)
        if len(ts) != N or ts.min() < 0 or ts.max() >= T or (N > 1 and not np.all(np.diff(ts) < 0)):
            raise ValueError(f"DPMSolverMultistepScheduler: {N} {self.timestep_spacing} steps of {T} (steps_offset {self.steps_offset}) "
                             f"do not give {N} strictly falling timesteps inside the schedule")
        self.num_inference_steps = N
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)
        self._ts = [int(t) for t in ts]
        self.reset_state()

    def reset_state(self) -> None:
        """The multistep state of a chain that has not started (what ``set_timesteps`` leaves)."""
        self.prev_x0: Optional[torch.Tensor] = None
        self.counter = 0

    def _row(self, k: int) -> list:
        """The DPM_ROW coefficients of call number ``k`` (see csrc/norm_elem.h), Python floats (fp64), rounded to fp32 once where they
        are stored: {cx, c0, sqrt(abar_s), sqrt(1 - abar_s), flags, t, c1, cz, 1/sqrt(abar_s), clip_min, clip_max, 0 ...}.  With g =
        1 (ODE) or 2 (SDE) and E = -expm1(-g h) = 1 - e^(-g h), the update x := cx x + c0 x0_hat + c1 x0_hat_prev + cz z has
          cx = sqrt((1 - abar_t) / (1 - abar_s)) e^(-(g - 1) h)      cz = sqrt((1 - abar_t) E) (SDE), 0 (ODE)
          w  = h / (2 (lambda_s - lambda_prev)) on a second-order step, else 0
          c0 = sqrt(abar_t) E (1 + w)                                 c1 = -sqrt(abar_t) E w
        and the last call (sigma_t = 0) is cx = 0, c0 = 1, c1 = cz = 0.  DRAWS is set exactly where cz is nonzero in fp32."""
        n = len(self._ts)
        if not 0 <= k < n:
            raise ValueError(f"DPMSolverMultistepScheduler: call {k} is outside the chain's {n} calls (set_timesteps starts one)")
        s = self._ts[k]
        a_s, lam_s = self._ac64[s], self._lambda[s]
        sde = self.algorithm_type == "sde-dpmsolver++"
        cx, c0, c1, cz, flags = 0.0, 1.0, 0.0, 0.0, 0
        if k + 1 < n:
            t = self._ts[k + 1]
            a_t, h = self._ac64[t], self._lambda[t] - lam_s
            g = 2.0 if sde else 1.0
            E = -float(np.expm1(-g * h))
            cx = ((1.0 - a_t) / (1.0 - a_s)) ** 0.5 * (float(np.exp(-h)) if sde else 1.0)
            w = 0.0
            if self.solver_order == 2 and k > 0:
                w = h / (2.0 * (lam_s - self._lambda[self._ts[k - 1]]))
                flags |= DPM_HAS_PREV
            c0, c1 = a_t ** 0.5 * E * (1.0 + w), -(a_t ** 0.5) * E * w
            if sde:
                cz = ((1.0 - a_t) * E) ** 0.5
                if float(np.float32(cz)) != 0.0:
                    flags |= DPM_DRAWS
                else:
                    cz = 0.0
        if self.clip_sample:
            flags |= DPM_CLIP
        clip = [self.clip_sample_min, self.clip_sample_max] if self.clip_sample else [0.0, 0.0]
        return [cx, c0, a_s ** 0.5, (1.0 - a_s) ** 0.5, float(flags), float(s), c1, cz, 1.0 / a_s ** 0.5] + clip + [0.0] * (DPM_ROW - 11)

    def _table(self, eta: float = 0.0) -> list:
        """One DPM_ROW-float row per UNet call over ``self.timesteps``: the table the device sampler reads (host only, no device work;
        ``eta`` is ignored)."""
        return [self._row(k) for k in range(len(self._ts))]

    _dpm_rows = _table                        # the name tests/test_dpm_cpu.py and tests/test_gpu_dpm.py call it by

    def _create_sampler(self, coef: int, n_rows: int, seed: int, handle) -> int:
        return _lib.lib().ldm_sampler_create_dpm(coef, n_rows, self._pred, seed, handle)

    def step(self, model_output: torch.Tensor, timestep: int, sample: torch.Tensor,
             generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None
             ) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (prev_sample, x0_hat): call number ``counter`` of the chain, which must be made at ``timesteps[counter]``.  ``noise``
        (extension) supplies z explicitly on a row that draws (the SDE form, every step but the last); otherwise torch.randn."""
        import ctypes as C
        k = self.counter
        if k >= len(self._ts):
            raise ValueError(f"DPMSolverMultistepScheduler.step: the chain's {len(self._ts)} calls are made (set_timesteps or reset_state "
                             "starts another)")
        if int(timestep) != self._ts[k]:
            raise ValueError(f"DPMSolverMultistepScheduler.step: call {k} of the chain is at timestep {self._ts[k]}, got {int(timestep)} "
                             "(the multistep state follows the calls in order)")
        if not sample.is_cuda:
            raise _lib.LdmError("DPMSolverMultistepScheduler.step: CUDA tensors only (no CPU fallback)")
        row = self._row(k)
        flags = int(row[4])
        m = model_output.detach().to(torch.float32).contiguous()
        x = sample.detach().to(torch.float32).contiguous()
        prev_in = None
        if flags & DPM_HAS_PREV:
            if self.prev_x0 is None or self.prev_x0.shape != x.shape:
                raise ValueError(f"DPMSolverMultistepScheduler.step: call {k} needs the previous call's x0_hat of this sample's shape")
            prev_in = self.prev_x0.to(device=x.device)
        z = None
        if flags & DPM_DRAWS:
            z = noise if noise is not None else self._draw(m, generator)
            z = z.to(device=x.device, dtype=torch.float32).contiguous()
        out, x0 = torch.empty_like(x), torch.empty_like(x)
        crow = (C.c_float * DPM_ROW)(*row)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().ldm_dpm_step(m.data_ptr(), x.data_ptr(), _lib.ptr(prev_in), _lib.ptr(z), None, out.data_ptr(),
                                               x0.data_ptr(), x.numel(), self._pred, crow, _lib.current_stream()))
        self.prev_x0 = x0
        self.counter += 1
        return out, x0


# RFlowScheduler's sample_method names -> the method argument of ldm_rflow_timesteps
SAMPLE_METHODS = {"uniform": 0, "logit-normal": 1}


class RFlowScheduler(_NoisingScheduler):
    """MONAI >= 1.4 ``monai.networks.schedulers.RFlowScheduler`` (rectified flow), restated from its formulae (not
    pinned against a MONAI install).  T = ``num_train_timesteps`` and tau = t / T: tau = 1 is pure noise, tau = 0 is data.

      add_noise         noisy = (1 - tau_b) x0 + tau_b noise, tau_b = float(t_b) / T in fp32
      training target   x0 - noise: the model predicts the velocity that carries noise to data (``add_noise_and_target``)
      set_timesteps(N)  t_i = (1 - i / N) T, rounded when ``use_discrete_timesteps``, then ``transform`` when ``use_timestep_transform``,
                        then + ``steps_offset``; kept as fp32 (an integer tensor only when discrete and untransformed); t = T is legal
      transform(t)      T r s / (1 + (r - 1) s), s = t / T, r = (input_img_size_numel / base_img_size_numel)^(1 / spatial_dim) * transform_scale
      step              prev = sample + dt m, x0_hat = sample + tau m, dt = (timestep - next_timestep) / T (1 / num_inference_steps
                        without ``next_timestep``); dt and tau in fp64 on the host, rounded once; no clipping, no noise
      sample_timesteps  t = u T (``"uniform"``) or sigmoid(loc + scale n) T (``"logit-normal"``), floored when discrete, then transformed

    There is no beta schedule, no ``prediction_type`` and no ``get_velocity``.  The element-wise math runs in libldm3d.so
    (ldm_rflow_step, ldm_rflow_noise_target, ldm_rflow_timesteps; the device sampler through ldm_sampler_create_rflow).  CUDA tensors only."""

    kind = 3
    repaint_kind = 2

    def __init__(self, num_train_timesteps: int = 1000, use_discrete_timesteps: bool = True, sample_method: str = "uniform",
                 loc: float = 0.0, scale: float = 1.0, use_timestep_transform: bool = False, transform_scale: float = 1.0,
                 steps_offset: int = 0, base_img_size_numel: int = 32 ** 3, spatial_dim: int = 3):
        if sample_method not in SAMPLE_METHODS:
            raise ValueError(f"sample_method given as {sample_method!r} must be one of {list(SAMPLE_METHODS)}")
        if int(num_train_timesteps) < 1:
            raise ValueError(f"num_train_timesteps must be at least 1, got {num_train_timesteps}")
        if sample_method == "logit-normal" and not float(scale) > 0.0:
            raise ValueError(f"logit-normal sampling needs scale > 0, got {scale}")
        if int(base_img_size_numel) < 1 or int(spatial_dim) < 1 or not float(transform_scale) > 0.0:
            raise ValueError("base_img_size_numel, spatial_dim and transform_scale must be positive")
        self.num_train_timesteps = int(num_train_timesteps)
        self.use_discrete_timesteps = bool(use_discrete_timesteps)
        self.sample_method, self.loc, self.scale = sample_method, float(loc), float(scale)
        self.use_timestep_transform, self.transform_scale = bool(use_timestep_transform), float(transform_scale)
        self.steps_offset = int(steps_offset)
        self.base_img_size_numel, self.spatial_dim = int(base_img_size_numel), int(spatial_dim)
        self._t_dev = {}
        self._drawn = None                    # (t, one_minus_tau, tau) of the last sample_timesteps call
        self.set_timesteps(self.num_train_timesteps, input_img_size_numel=self.base_img_size_numel)

    def transform_ratio(self, input_img_size_numel: int) -> float:
        """r of ``transform`` for a volume of ``input_img_size_numel`` voxels (fp64)."""
        return (float(input_img_size_numel) / self.base_img_size_numel) ** (1.0 / self.spatial_dim) * self.transform_scale

    def transform(self, t, input_img_size_numel: int):
        """The resolution-dependent timestep map, in fp64 (numpy array or float)."""
        r, T = self.transform_ratio(input_img_size_numel), float(self.num_train_timesteps)
        s = np.asarray(t, dtype=np.float64) / T
        return T * (r * s / (1.0 + (r - 1.0) * s))

    def set_timesteps(self, num_inference_steps: int, device=None, input_img_size_numel: Optional[int] = None) -> None:
        if num_inference_steps > self.num_train_timesteps:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                             f"`self.num_train_timesteps`: {self.num_train_timesteps}")
        if num_inference_steps < 1:
            raise ValueError(f"`num_inference_steps` must be at least 1, got {num_inference_steps}")
        if self.use_timestep_transform and input_img_size_numel is None:
            raise ValueError("RFlowScheduler.set_timesteps: use_timestep_transform needs input_img_size_numel")
        self.num_inference_steps = int(num_inference_steps)
        ts = (1.0 - np.arange(num_inference_steps, dtype=np.float64) / num_inference_steps) * self.num_train_timesteps
        if self.use_discrete_timesteps:
            ts = np.round(ts)
        if self.use_timestep_transform:
            ts = self.transform(ts, input_img_size_numel)
        ts = (ts + self.steps_offset).astype(np.float32)
        if self.use_discrete_timesteps and not self.use_timestep_transform:
            ts = ts.astype(np.int64)
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)

    def _row(self, timestep: float, next_timestep: Optional[float]) -> list:
        """The sampler row of one step, {dt, tau, 0, 0, 0, t, 0, 0}: Python floats (fp64), rounded to fp32 once where they are stored."""
        T = float(self.num_train_timesteps)
        dt = 1.0 / self.num_inference_steps if next_timestep is None else (float(timestep) - float(next_timestep)) / T
        return [dt, float(timestep) / T, 0.0, 0.0, 0.0, float(timestep), 0.0, 0.0]

    def _table(self, eta: float = 0.0) -> list:
        """One row per step over ``self.timesteps``, each stepping to the next timestep and the last to 0: the table the device sampler
        reads, and row for row what ``step`` passes by value when the inferer drives it (host only, no device work; ``eta`` is ignored)."""
        ts = [float(t) for t in self.timesteps.tolist()]
        return [self._row(t, ts[k + 1] if k + 1 < len(ts) else 0.0) for k, t in enumerate(ts)]

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, next_timestep=None, generator=None, noise=None
             ) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (prev_sample, x0_hat).  ``generator`` / ``noise`` are accepted for the other schedulers' call shape and unused: a flow step
        draws nothing."""
        import ctypes as C
        if not sample.is_cuda:
            raise _lib.LdmError("RFlowScheduler.step: CUDA tensors only (no CPU fallback)")
        m = model_output.detach().to(torch.float32).contiguous()
        x = sample.detach().to(torch.float32).contiguous()
        row = (C.c_float * 8)(*self._row(float(timestep), None if next_timestep is None else float(next_timestep)))
        prev, x0 = torch.empty_like(x), torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().ldm_rflow_step(m.data_ptr(), x.data_ptr(), prev.data_ptr(), x0.data_ptr(), x.numel(), row,
                                                 _lib.current_stream()))
        return prev, x0

    def _noising_coefs(self, timesteps, dev):
        """The per-sample (1 - tau, tau) [B] on ``dev``: the vectors ldm_rflow_timesteps wrote if ``timesteps`` is the tensor the last
        ``sample_timesteps`` returned, else tau = float(t) / T and 1 - tau in fp32 from the explicit timesteps (no host read)."""
        if self._drawn is not None and timesteps is self._drawn[0]:
            return self._drawn[1], self._drawn[2]
        T = self._t_dev.get(dev)
        if T is None:
            T = self._t_dev[dev] = torch.tensor(float(self.num_train_timesteps), dtype=torch.float32, device=dev)
        tau = (timesteps.to(device=dev, dtype=torch.float32).reshape(-1) / T).contiguous()
        return (1.0 - tau).contiguous(), tau

    def add_noise_and_target(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor
                             ) -> Tuple[torch.Tensor, torch.Tensor]:
        """(add_noise(x0, noise, t), x0 - noise) in one kernel pass (ldm_rflow_noise_target)."""
        x0c, ec, a, b = self._noising_args(original_samples, noise, timesteps, "add_noise_and_target")
        noisy, target = torch.empty_like(x0c), torch.empty_like(x0c)
        B = x0c.shape[0]
        with torch.cuda.device(x0c.device):
            _lib.check(_lib.lib().ldm_rflow_noise_target(x0c.data_ptr(), ec.data_ptr(), a.data_ptr(), b.data_ptr(), noisy.data_ptr(),
                                                         target.data_ptr(), B, x0c.numel() // B, _lib.current_stream()))
        return noisy, target

    def sample_timesteps(self, x_start: torch.Tensor, *, idx=None, seed: int = 0, step: int = 0,
                         draw: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Training timesteps [B] (device fp32, what the UNet's timestep input takes) for the batch ``x_start`` [B, C, ...], in ONE launch
        (ldm_rflow_timesteps) that also writes the two coefficient vectors ``add_noise`` / ``add_noise_and_target`` / ``LatentCache.batch``
        use when they are handed the returned tensor itself.  ``draw`` [B] supplies u (uniform) or n (logit-normal); otherwise the kernel
        draws them as a function of ``(seed, step, idx[b])`` alone (``idx``: dataset indices, default the batch slots).  With
        ``use_timestep_transform`` the volume size is the product of ``x_start.shape[2:]``."""
        import ctypes as C
        if not x_start.is_cuda:
            raise _lib.LdmError("RFlowScheduler.sample_timesteps: CUDA tensors only (no CPU fallback)")
        B, dev = int(x_start.shape[0]), x_start.device
        ids = None
        if idx is not None:
            idx = [int(i) for i in (idx.reshape(-1).tolist() if isinstance(idx, torch.Tensor) else idx)]
            if len(idx) != B:
                raise ValueError(f"sample_timesteps: {B} samples but {len(idx)} indices")
            ids = (C.c_int * B)(*idx)
        if draw is not None:
            draw = draw.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            if draw.numel() != B:
                raise ValueError(f"sample_timesteps: {B} samples but {draw.numel()} draws")
        ratio = 0.0
        if self.use_timestep_transform:
            numel = 1
            for s in x_start.shape[2:]:
                numel *= int(s)
            ratio = self.transform_ratio(numel)
        out = torch.empty((3, B), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ldm_rflow_timesteps(ids, B, self.num_train_timesteps, SAMPLE_METHODS[self.sample_method], self.loc,
                                                      self.scale, int(self.use_discrete_timesteps), ratio, _lib.ptr(draw),
                                                      int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF, out[0].data_ptr(),
                                                      out[1].data_ptr(), out[2].data_ptr(), _lib.current_stream()))
        self._drawn = (out[0], out[1], out[2])
        return self._drawn[0]

    def _step_kwargs(self, ts: list, k: int) -> dict:
        """A flow step goes to the next timestep of the schedule, 0 after the last."""
        return dict(next_timestep=ts[k + 1] if k + 1 < len(ts) else 0)

    def _latent_batch(self, head: tuple, tail: tuple) -> int:
        return _lib.lib().ldm_latent_batch_rflow(*head, *tail)     # (1 - tau, tau) in ``head``, target = z - noise

    def _create_sampler(self, coef: int, n_rows: int, seed: int, handle) -> int:
        return _lib.lib().ldm_sampler_create_rflow(coef, n_rows, handle)       # a flow chain draws nothing: no seed

    def _create_repaint_sampler(self, coef: int, n_rows: int, seed: int, handle) -> int:
        return _lib.lib().ldm_sampler_create_repaint(coef, n_rows, self.repaint_kind, 0, 0, seed, handle)      # no prediction type, no clipping

    def _repaint_marginals(self) -> list:
        """tau of the state at every level 0 .. n: the timesteps' own, and 0 after the last step."""
        T = float(self.num_train_timesteps)
        return [float(t) / T for t in self.timesteps.tolist()] + [0.0]

    @staticmethod
    def _repaint_coefs(m_a: float, m_b: Optional[float] = None) -> tuple:
        ja = 1.0 if m_b is None else (1.0 - m_b) / (1.0 - m_a)
        js = 0.0 if m_b is None else max(m_b ** 2 - ja ** 2 * m_a ** 2, 0.0) ** 0.5
        return 1.0 - m_a, m_a, ja, js


# the keys of a config's NoiseScheduler section that an RFlowScheduler reads, beside num_train_timesteps
RFLOW_CONFIG_KEYS = ("use_discrete_timesteps", "sample_method", "loc", "scale", "use_timestep_transform", "transform_scale",
                     "base_img_size_numel")
NOISE_SCHEDULERS = ("ddpm", "rflow")


def noise_scheduler_name(section: dict) -> str:
    """``"scheduler"`` of a config's NoiseScheduler section: "ddpm" (the default and the reference's) or "rflow"."""
    name = section.get("scheduler", "ddpm")
    if name not in NOISE_SCHEDULERS:
        raise ValueError(f"NoiseScheduler.scheduler given as {name!r} must be one of {list(NOISE_SCHEDULERS)}")
    return name


def rflow_config_args(section: dict) -> dict:
    """Keyword arguments of the RFlowScheduler a config's NoiseScheduler section with ``"scheduler": "rflow"`` describes; the constructor
    refuses an unknown ``sample_method`` or a non-positive ``scale``."""
    kw = dict(num_train_timesteps=section["num_train_timesteps"])
    kw.update({k: section[k] for k in RFLOW_CONFIG_KEYS if k in section})
    return kw


_CHAINS = itertools.count(1)


def start_step_for_strength(n_steps: int, strength: float) -> int:
    """The first row of a warm chain of ``n_steps`` rows that re-noises its start by ``strength`` in (0, 1]: k0 = n - min(int(n *
    strength), n), so the chain makes n - k0 = int(n * strength) UNet calls; 1.0 is the full chain from row 0.  The convention of
    diffusers' image-to-image pipelines (MONAI has none).  A strength that leaves nothing to denoise (k0 == n) raises ValueError."""
    n, s = int(n_steps), float(strength)
    if n < 1:
        raise ValueError(f"n_steps must be at least 1, got {n_steps}")
    if not 0.0 < s <= 1.0:
        raise ValueError(f"strength must be in (0, 1], got {strength}")
    k0 = n - min(int(n * s), n)
    if k0 >= n:
        raise ValueError(f"strength {strength} of {n} steps leaves no step to denoise (int(n * strength) = 0)")
    return k0


def _sampler_rows(scheduler: _NoisingScheduler, eta: float = 0.0):
    """-> (kind, rows): the kind number of the C ABI and the device sampler's coefficient table over ``scheduler.timesteps``."""
    return scheduler.kind, scheduler._table(eta)


class DeviceSampler:
    """The scheduler step as ONE kernel with everything it needs on the device (``ldm_sampler_*``): the per-step coefficients
    (computed here exactly as ``DDPMScheduler.step`` / ``DDIMScheduler.step`` pass them by value) live in a device table, the
    current step index and the UNet's timestep input are device state advanced by the kernel itself, and the noise z is drawn
    inside the kernel (Philox4x32-10, counter = (element, step), key = seed) instead of ``torch.randn``.  One denoising step
    (``DiffusionModelUNet.denoise_step``) is then a fixed launch sequence with fixed arguments and replays as ONE HIP graph:
    no ``fill_`` / ``normal_`` launches and no host work per step (3d_ldm/inference.py:94-99's loop body).

    Not MONAI's RNG stream: a chain sampled this way is a different (equally distributed) draw than the same seed through
    ``torch.randn``; ``noise(step, shape)`` returns the exact z of a step for reproducibility checks.

    A PNDMScheduler steps the same way, one call per entry of its ``timesteps``: its multistep state (four past model outputs, the saved
    sample, the Runge-Kutta accumulator) is one device tensor that this object allocates and hands to the library at the first step,
    when the latent's size is known (``bind_state``); the kernel advances it, ``reset`` rewinds it with the counter.

    A DPMSolverMultistepScheduler steps the same way, one call per timestep: its state is the previous call's x0_hat (``state_numel(n)
    == n``), bound like PNDM's; the SDE form's z of step k is ``noise(k, shape)``, and ``x0_out`` receives x0_hat.

    An RFlowScheduler steps the same way with rows {dt, tau, ..., t} (ldm_sampler_create_rflow): it draws nothing and keeps no state, so
    ``noise`` and ``bind_state`` are refused by the library, and ``x0_out`` receives x + tau m.

    Warm starts: ``seek(k0, tbuf)`` is ``reset`` at row k0 and ``start`` noises a given latent to that row's timestep in one launch
    (DDPM, DDIM, rectified flow; PNDM and DPM-Solver++ chains start at row 0 only).  ``rows=`` builds the sampler on given 8-float rows instead of the
    scheduler's own table: ``DDIMScheduler.inversion_sampler`` passes the ascending rows of DDIM inversion."""

    def __init__(self, scheduler: _NoisingScheduler, seed: int = 0, eta: float = 0.0, rows: Optional[list] = None):
        import ctypes as C
        self.scheduler = scheduler
        if rows is None:
            self.timesteps = scheduler.timesteps.tolist()
            rows = scheduler._table(eta)
        else:                                              # given rows of a DDPM / DDIM scheduler's layout, e.g. DDIM inversion's
            if not isinstance(scheduler, (DDPMScheduler, DDIMScheduler)) or not rows or any(len(r) != 8 for r in rows):
                raise ValueError("DeviceSampler(rows=...) takes 8-float rows of a DDPMScheduler or a DDIMScheduler")
            self.timesteps = [int(r[5]) for r in rows]
        self._h = C.c_void_p()
        self.kind, self._state = scheduler.kind, None
        coef = torch.tensor(rows, dtype=torch.float32).contiguous()
        _lib.check(scheduler._create_sampler(coef.data_ptr(), len(rows), int(seed) & (2 ** 64 - 1), C.byref(self._h)))
        self.chain = next(_CHAINS)
        self.n_steps, self.seed = len(rows), int(seed)

    def reset(self, tbuf: torch.Tensor) -> None:
        """Step counter := 0 and ``tbuf`` (the UNet's fp32 timestep input, one entry per sample) := the first timestep."""
        self.chain = next(_CHAINS)                          # never reused: identifies the chain this reset starts
        with torch.cuda.device(tbuf.device):
            _lib.check(_lib.lib().ldm_sampler_reset(self._h, tbuf.data_ptr(), tbuf.numel(), _lib.current_stream()))

    def seek(self, k0: int, tbuf: torch.Tensor) -> None:
        """``reset`` at row ``k0``: step counter := k0 and ``tbuf`` (every entry) := ``timesteps[k0]``, so that the next step is the
        one a full chain takes as its step k0, noise included (the Philox step index is the row index).  PNDM: k0 = 0 only."""
        self.chain = next(_CHAINS)
        with torch.cuda.device(tbuf.device):
            _lib.check(_lib.lib().ldm_sampler_seek(self._h, int(k0), tbuf.data_ptr(), tbuf.numel(), _lib.current_stream()))

    def start(self, z0: torch.Tensor, k0: int, B: int, seed: Optional[int] = None, first_member: int = 0,
              noise: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The noised start of a warm chain -> x [B, ...]: ``z0`` ([1 or B, ...], the clean scaled latent; one latent is broadcast to the
        B members without a copy) noised to ``timesteps[k0]`` in one launch (ldm_sampler_start), x = sqrt(abar) z0 + sqrt(1 - abar) e
        (rectified flow: (1 - tau) z0 + tau e).  e is ``noise`` [B, ...] or, by default, drawn in the kernel from Philox keyed by ``seed``
        (default: the sampler's) and the member's global index ``first_member + b``: the draw of a member does not depend on the chunk
        it runs in; ``start_noise`` returns it.  ``out`` may be ``z0`` itself when z0 has B entries."""
        if not (z0.is_cuda and z0.dtype == torch.float32 and z0.is_contiguous() and z0.dim() >= 2):
            raise _lib.LdmError("DeviceSampler.start: z0 must be a contiguous fp32 CUDA tensor [1 or B, ...]")
        B = int(B)
        shape = (B,) + tuple(z0.shape[1:])
        per = z0.numel() // z0.shape[0]
        if noise is not None:
            if tuple(noise.shape) != shape:
                raise ValueError(f"DeviceSampler.start: noise must be {shape}, got {tuple(noise.shape)}")
            noise = noise.detach().to(device=z0.device, dtype=torch.float32).contiguous()
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=z0.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape):
            raise _lib.LdmError(f"DeviceSampler.start: out must be a contiguous fp32 CUDA tensor {shape}")
        seed = self.seed if seed is None else int(seed)
        with torch.cuda.device(z0.device):
            _lib.check(_lib.lib().ldm_sampler_start(self._h, int(k0), z0.data_ptr(), int(z0.shape[0]), _lib.ptr(noise), out.data_ptr(), B, per,
                                                    seed & (2 ** 64 - 1), int(first_member) & 0xFFFFFFFF, _lib.current_stream()))
        return out

    def start_noise(self, member: int, shape, device, seed: Optional[int] = None) -> torch.Tensor:
        """The exact draws ``start`` makes for global member ``member`` of one-member ``shape`` (reproducibility checks)."""
        out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
        seed = self.seed if seed is None else int(seed)
        with torch.cuda.device(out.device):
            _lib.check(_lib.lib().ldm_sampler_start_noise(seed & (2 ** 64 - 1), int(member) & 0xFFFFFFFF, out.data_ptr(), out.numel(),
                                                          _lib.current_stream()))
        return out

    def state_numel(self, n: int) -> int:
        """Floats of multistep state a step of ``n`` elements needs (0 for DDPM / DDIM)."""
        return _lib.lib().ldm_sampler_state_bytes(self._h, int(n)) // 4

    def bind_state(self, state: torch.Tensor, n: int) -> None:
        """PNDM, DPM-Solver++: ``state`` (contiguous fp32 CUDA, at least ``state_numel(n)`` entries, any contents) becomes the multistep
        state of steps on ``n``-element latents.  It is kept alive here.  Between chains only: a chain in flight loses its history."""
        if not (state.is_cuda and state.dtype == torch.float32 and state.is_contiguous()):
            raise _lib.LdmError("DeviceSampler.bind_state: a contiguous fp32 CUDA tensor is needed")
        _lib.check(_lib.lib().ldm_sampler_bind_state(self._h, state.data_ptr(), state.numel() * 4, int(n)))
        self._state, self._state_n = state, int(n)

    def ensure_state(self, n: int, device) -> None:
        """Allocate and bind the multistep state (PNDM, DPM-Solver++) for ``n``-element latents on ``device`` unless that is what is bound
        (no-op for a scheduler that is not ``multistep``): called by ``step`` and by the UNet's ``denoise_step`` /
        ``denoise_step_windows`` before they hand over the handle."""
        if not self.scheduler.multistep or (self._state is not None and self._state_n == int(n) and self._state.device == torch.device(device)):
            return
        self.bind_state(torch.empty((self.state_numel(n),), dtype=torch.float32, device=device), n)

    def step(self, eps: torch.Tensor, x: torch.Tensor, tbuf: torch.Tensor, x0_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x := step(x, eps) IN PLACE for the step the device counter points at; advances the counter and ``tbuf``."""
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and eps.is_contiguous() and eps.dtype == torch.float32):
            raise _lib.LdmError("DeviceSampler.step: contiguous fp32 CUDA tensors only")
        self.ensure_state(x.numel(), x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().ldm_sampler_step(self._h, eps.data_ptr(), x.data_ptr(), _lib.ptr(x0_out), x.numel(), tbuf.data_ptr(),
                                                   tbuf.numel(), _lib.current_stream()))
        return x

    def noise(self, step: int, shape, device) -> torch.Tensor:
        out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
        with torch.cuda.device(out.device):
            _lib.check(_lib.lib().ldm_sampler_noise(self._h, int(step), out.data_ptr(), out.numel(), _lib.current_stream()))
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                _lib.lib().ldm_sampler_destroy(self._h)
                self._h = None
        except Exception:
            pass


REPAINT_ROW = 16                              # floats per row of a repaint table (include/ldm3d.h LDM_REPAINT_ROW)
REPAINT_MAX_ROWS = 16384                      # LDM_REPAINT_MAX_ROWS: UNet calls of one chain


def repaint_schedule(n_steps: int, jump_length: int = 1, n_resample: int = 1) -> list:
    """The UNet calls of a RePaint chain (Lugmayr et al. 2022, Alg. 1) over ``n_steps`` timesteps -> [(level, jump)], one per call.
    Level L is the state at ``timesteps[L]`` and level ``n_steps`` the finished sample, so levels count from the NOISE end; a call at
    level L moves the state to level L + 1.  After arriving at a level a with a % jump_length == 0, a < n_steps and fewer than
    n_resample - 1 jumps taken from a so far, the chain jumps back to level a - jump_length (the call that arrived carries jump =
    True) and denoises those levels again.  n_resample = 1 (or jump_length >= n_steps) is the plain chain; the call count is
    n_steps + (n_resample - 1) * jump_length * ((n_steps - 1) // jump_length).  Pure Python, no device work."""
    n, j, r = int(n_steps), int(jump_length), int(n_resample)
    if n < 1 or j < 1 or r < 1:
        raise ValueError(f"n_steps, jump_length and n_resample must be at least 1, got {n_steps}, {jump_length}, {n_resample}")
    calls, taken, level = [], {}, 0
    while level < n:
        a = level + 1
        jump = a % j == 0 and a < n and taken.get(a, 0) < r - 1
        calls.append((level, jump))
        if jump:
            taken[a] = taken.get(a, 0) + 1
            level = a - j
        else:
            level = a
    return calls


def _repaint_marginals(scheduler) -> list:
    """``scheduler._repaint_marginals()``: the name tests/test_repaint_cpu.py imports."""
    return scheduler._repaint_marginals()


def repaint_rows(scheduler, jump_length: int = 1, n_resample: int = 1, eta: float = 0.0):
    """-> (schedule, rows): ``repaint_schedule`` over ``scheduler.timesteps`` and one REPAINT_ROW-float row per call (csrc/repaint.h),
    fp64 here and rounded to fp32 once where the table is stored: the scheduler's own 8-float sampler row of ``timesteps[level]`` (slot
    5 is t), then for the level a = level + 1 the step arrives at
      ka, ks   the known region there, ka known + ks z: sqrt(abar_a), sqrt(1 - abar_a) | flow 1 - tau_a, tau_a | a = n: 1, 0
      ja, js   with ``jump``, the Gaussian jump back to b = a - jump_length: sqrt(abar_b / abar_a), sqrt(1 - abar_b / abar_a) |
               flow (1 - tau_b) / (1 - tau_a), sqrt(tau_b^2 - ja^2 tau_a^2); else 1, 0
      flags    1 = jump
    RePaint's j single forward steps are one Gaussian here: the same distribution in one pass.  Host only, no device work."""
    if not isinstance(scheduler, _NoisingScheduler):
        raise TypeError("inpainting needs a DDPMScheduler, a DDIMScheduler or an RFlowScheduler")
    refuse_multistep(scheduler, inpainting=True)
    n, j = len(scheduler.timesteps), int(jump_length)
    schedule = repaint_schedule(n, j, n_resample)
    if len(schedule) > REPAINT_MAX_ROWS:
        raise ValueError(f"a repaint chain of {len(schedule)} UNet calls: at most {REPAINT_MAX_ROWS} are built")
    lv, base = scheduler._repaint_marginals(), scheduler._table(eta)
    rows = []
    for level, jump in schedule:
        a = level + 1
        ka, ks, ja, js = scheduler._repaint_coefs(lv[a], lv[a - j] if jump else None)
        if a == n:
            ka, ks = 1.0, 0.0
        rows.append([float(v) for v in base[level]] + [ka, ks, ja, js, 1.0 if jump else 0.0, 0.0, 0.0, 0.0])
    return schedule, rows


def check_keep_mask(keep_mask: torch.Tensor, spatial=None) -> torch.Tensor:
    """A keep mask [d, h, w] or [1, 1, d, h, w] with values 0 / 1 -> contiguous fp32 [d, h, w] (1 = keep).  Any other value raises
    ValueError: soft masks are not built."""
    m = keep_mask
    if m.dim() == 5 and m.shape[0] == 1 and m.shape[1] == 1:
        m = m[0, 0]
    if m.dim() != 3 or (spatial is not None and tuple(m.shape) != tuple(spatial)):
        want = "[d, h, w]" if spatial is None else str(tuple(spatial))
        raise ValueError(f"keep_mask must be {want} or [1, 1, d, h, w], got {tuple(keep_mask.shape)}")
    m = m.detach().to(torch.float32)
    if not bool(((m == 0) | (m == 1)).all()):
        raise ValueError("keep_mask must hold only 0 (regenerate) and 1 (keep): soft masks are not implemented")
    return m.contiguous()


def repaint_merge(x: torch.Tensor, known: torch.Tensor, keep: torch.Tensor, coef4, jump: bool, z_known: Optional[torch.Tensor] = None,
                  z_jump: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The merge and the jump of one repaint row on explicit draws (ldm_repaint_merge; the device step's own arithmetic, bit for bit):
    where ``keep`` [d, h, w] is nonzero, x := fma(ka, known, ks z_known); with ``jump``, x := fma(ja, x, js z_jump).  ``x`` [B, C, d, h,
    w], ``known`` [1 or B, C, d, h, w], ``coef4`` = (ka, ks, ja, js): slots 8 .. 11 of the row.  A draw may be None where its coefficient
    is 0.  ``out`` may be ``x``."""
    import ctypes as C
    for name, t in (("x", x), ("known", known), ("keep", keep)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise _lib.LdmError(f"repaint_merge: {name} must be a contiguous fp32 CUDA tensor")
    B, per, dhw = int(x.shape[0]), x.numel() // x.shape[0], keep.numel()
    if known.numel() != int(known.shape[0]) * per:
        raise ValueError(f"repaint_merge: known {tuple(known.shape)} does not match x {tuple(x.shape)}")
    zs = []
    for z in (z_known, z_jump):
        if z is not None:
            if tuple(z.shape) != tuple(x.shape):
                raise ValueError(f"repaint_merge: a draw must have x's shape {tuple(x.shape)}, got {tuple(z.shape)}")
            z = z.detach().to(device=x.device, dtype=torch.float32).contiguous()
        zs.append(z)
    if out is None:
        out = torch.empty_like(x)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == x.shape):
        raise _lib.LdmError("repaint_merge: out must be a contiguous fp32 CUDA tensor of x's shape")
    c4 = (C.c_float * 4)(*[float(v) for v in coef4])
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().ldm_repaint_merge(x.data_ptr(), known.data_ptr(), int(known.shape[0]), keep.data_ptr(), _lib.ptr(zs[0]),
                                                _lib.ptr(zs[1]), out.data_ptr(), B, per, dhw, c4, int(bool(jump)), _lib.current_stream()))
    return out


class RepaintSampler(DeviceSampler):
    """The device sampler of an inpainting chain (``ldm_sampler_create_repaint``; RePaint): every step is the base scheduler's step (DDPM,
    DDIM with its ``eta``, rectified flow), then the known region is put back at the noise level the step arrived at, then, where the
    schedule says so, the whole state jumps back ``jump_length`` levels towards noise - all in the one step kernel, so ``denoise_step``
    / ``denoise_step_windows`` (guided or not, graph replay included) take this sampler as they take any other.

    ``known`` [1 or B, C, d, h, w] (a scaled latent; one latent serves every sample of the batch without a copy) and ``keep_mask`` [d,
    h, w] (1 = keep) are bound to the handle and kept alive here (``bind``).  ``n_calls`` = ``n_steps`` = the UNet calls of the chain,
    ``schedule`` the (level, jump) of each, ``rows`` the 16-float table, ``base_rows`` its first 8 columns (a plain ``DeviceSampler(
    rows=...)`` steps them).  ``noise(row, ...)`` is the step noise of a ROW, ``noise_known`` / ``noise_jump`` the draws of the merge and
    the jump: three Philox streams of one seed.  No warm start (``start`` raises) and no PNDM (NotImplementedError)."""

    def __init__(self, scheduler, known: torch.Tensor, keep_mask: torch.Tensor, jump_length: int = 1, n_resample: int = 1,
                 seed: int = 0, eta: float = 0.0):
        import ctypes as C
        self._h = None
        self.scheduler = scheduler
        self.schedule, self.rows = repaint_rows(scheduler, jump_length, n_resample, eta)
        self.base_rows = [r[:8] for r in self.rows]
        self.kind, self._state = scheduler.kind, None
        ts = scheduler.timesteps.tolist()
        self.timesteps = [ts[level] for level, _ in self.schedule]
        self.jump_length, self.n_resample = int(jump_length), int(n_resample)
        coef = torch.tensor(self.rows, dtype=torch.float32).contiguous()
        h = C.c_void_p()
        _lib.check(scheduler._create_repaint_sampler(coef.data_ptr(), len(self.rows), int(seed) & (2 ** 64 - 1), C.byref(h)))
        self._h = h
        self.chain = next(_CHAINS)
        self.n_steps = self.n_calls = len(self.rows)
        self.seed = int(seed)
        self.known = self.keep = None
        self.bind(known, keep_mask)

    def bind(self, known: torch.Tensor, keep_mask: torch.Tensor) -> None:
        """``known`` and ``keep_mask`` become what the steps keep (ldm_sampler_bind_known); between chains only.  The handle takes a new
        identity in the graph cache, so a graph recorded on the earlier tensors is never replayed."""
        if not (known.is_cuda and known.dim() == 5):
            raise _lib.LdmError("RepaintSampler: the known latent must be a CUDA tensor [1 or B, C, d, h, w] (no CPU fallback)")
        keep = check_keep_mask(keep_mask, known.shape[2:]).to(known.device).contiguous()
        kn = known.detach().to(torch.float32).contiguous()
        _lib.check(_lib.lib().ldm_sampler_bind_known(self._h, kn.data_ptr(), int(kn.shape[0]), keep.data_ptr(), kn.numel() // kn.shape[0],
                                                     keep.numel()))
        self.known, self.keep = kn, keep
        self.chain = next(_CHAINS)

    def start(self, *args, **kwargs):
        raise NotImplementedError("warm-started inpainting is not implemented: a repaint chain starts from noise at its first row")

    def _draws(self, which: int, row: int, shape, device) -> torch.Tensor:
        out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
        with torch.cuda.device(out.device):
            _lib.check(_lib.lib().ldm_sampler_repaint_noise(self._h, which, int(row), out.data_ptr(), out.numel(), _lib.current_stream()))
        return out

    def noise_known(self, row: int, shape, device) -> torch.Tensor:
        """The exact z_known of row ``row`` for a latent of ``shape`` (the whole batch)."""
        return self._draws(0, row, shape, device)

    def noise_jump(self, row: int, shape, device) -> torch.Tensor:
        """The exact z_jump of row ``row`` for a latent of ``shape`` (the whole batch)."""
        return self._draws(1, row, shape, device)


class DeviceLikelihood:
    """``get_likelihood``'s loop state on the device (``ldm_likelihood_*``), next to DeviceSampler: the per-timestep rows
    (``DDPMScheduler.likelihood_rows``) live in a device table indexed by a device step counter, the noise z is Philox4x32-10 keyed by
    ``seed`` (``noise`` returns it as a tensor), and one step (``DiffusionModelUNet.likelihood_step``) is the UNet forward plus two
    small launches: one HIP graph per timestep.  ``noisy`` / ``term`` are the host-driven halves with row k by value: the same
    per-element code and the same reduction, bit for bit.

    Only a DDPMScheduler has the posterior this scores (MONAI raises NotImplementedError for any other scheduler, and so does this)."""

    def __init__(self, scheduler, seed: int = 0, bin_width: float = 1.0 / 255.0):
        import ctypes as C
        if not hasattr(scheduler, "likelihood_rows"):
            raise NotImplementedError("Likelihood computation is only compatible with DDPMScheduler")
        self.scheduler = scheduler
        self.rows = scheduler.likelihood_rows()
        self.timesteps = [int(r[5]) for r in self.rows]
        self.n_steps, self.seed, self.bin_width = len(self.rows), int(seed), float(bin_width)
        self._h = C.c_void_p()
        coef = torch.tensor(self.rows, dtype=torch.float32).contiguous()
        _lib.check(_lib.lib().ldm_likelihood_create(coef.data_ptr(), self.n_steps, scheduler._pred, int(scheduler.clip_sample),
                                                    self.seed & (2 ** 64 - 1), self.bin_width, C.byref(self._h)))
        self._noise = None
        self._scratch = {}

    @staticmethod
    def _shape(x: torch.Tensor):
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() >= 2):
            raise _lib.LdmError("DeviceLikelihood: contiguous fp32 CUDA tensors [B, ...] only")
        return x.shape[0], x.numel() // x.shape[0]

    def scratch(self, x: torch.Tensor) -> torch.Tensor:
        """The persistent partial-sum buffer for tensors shaped like ``x`` (its address is part of a recorded step)."""
        B, per = self._shape(x)
        key = (B, per, str(x.device))
        buf = self._scratch.get(key)
        if buf is None:
            nbytes = _lib.lib().ldm_likelihood_scratch_bytes(B, per)
            if nbytes == 0:
                raise _lib.LdmError((_lib.lib().ldm_last_error() or b"scratch query failed").decode())
            buf = self._scratch[key] = torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=x.device)
        return buf

    def reset(self, x0: torch.Tensor, x_t: torch.Tensor, tbuf: torch.Tensor, total: torch.Tensor, noise: Optional[torch.Tensor] = None) -> None:
        """Step counter := 0, ``total`` := 0, ``x_t`` := the first timestep's noising of ``x0`` (z = ``noise``, default the Philox
        draw), ``tbuf`` := the first timestep.  ``noise`` is kept alive here: the steps re-noise with it."""
        B, per = self._shape(x0)
        self._shape(x_t)
        if noise is not None:
            self._shape(noise)
        self._noise = noise
        with torch.cuda.device(x0.device):
            _lib.check(_lib.lib().ldm_likelihood_reset(self._h, x0.data_ptr(), _lib.ptr(noise), x_t.data_ptr(), tbuf.data_ptr(), B, per,
                                                       total.data_ptr(), _lib.current_stream()))

    def noise(self, shape, device) -> torch.Tensor:
        """The Philox z of a latent of ``shape`` [B, ...]: what ``reset`` and the steps draw when given no noise."""
        out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
        B, per = self._shape(out)
        with torch.cuda.device(out.device):
            _lib.check(_lib.lib().ldm_likelihood_noise(self._h, out.data_ptr(), B, per, _lib.current_stream()))
        return out

    def _row(self, k: int):
        import ctypes as C
        return (C.c_float * LIK_ROW)(*self.rows[k])

    def noisy(self, x0: torch.Tensor, noise: torch.Tensor, k: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Host-driven: x_t of row ``k``, sqrt(abar) x0 + sqrt(1 - abar) noise, rounded as the device loop rounds it."""
        B, per = self._shape(x0)
        self._shape(noise)
        out = torch.empty_like(x0) if out is None else out
        with torch.cuda.device(x0.device):
            _lib.check(_lib.lib().ldm_likelihood_noisy(x0.data_ptr(), noise.data_ptr(), self._row(k), out.data_ptr(), B, per,
                                                       _lib.current_stream()))
        return out

    def term(self, x0: torch.Tensor, x_t: torch.Tensor, m: torch.Tensor, k: int, total: torch.Tensor,
             kl_map: Optional[torch.Tensor] = None, term_out: Optional[torch.Tensor] = None) -> None:
        """Host-driven: row ``k``'s terms of (x0, x_t, model output m): ``total`` [B] += the per-sample mean, ``term_out`` [B] := it,
        ``kl_map`` := the per-element terms."""
        B, per = self._shape(x0)
        self._shape(x_t), self._shape(m)
        ws = self.scratch(x0)
        with torch.cuda.device(x0.device):
            _lib.check(_lib.lib().ldm_likelihood_term(x0.data_ptr(), x_t.data_ptr(), m.data_ptr(), self._row(k), self.scheduler._pred,
                                                      int(self.scheduler.clip_sample), self.bin_width, _lib.ptr(kl_map), _lib.ptr(term_out),
                                                      total.data_ptr(), B, per, ws.data_ptr(), ws.numel() * 8, _lib.current_stream()))

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                _lib.lib().ldm_likelihood_destroy(self._h)
                self._h = None
        except Exception:
            pass
