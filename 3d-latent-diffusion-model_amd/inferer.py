"""LatentDiffusionInferer with MONAI's interface (3d_ldm/train_diffusion.py:152,197-205,260-268,326-333;
3d_ldm/inference.py:85,94-99).  Pure orchestration: every tensor op is a libldm3d.so launch."""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional, Sequence, Union

import torch

from . import _lib
from .guidance import check_measurable
from .schedulers import DeviceLikelihood, check_keep_mask, refuse_multistep, repaint_merge, repaint_rows


def _check_cfg(cfg, conditioning, mode) -> None:
    """Classifier-free guidance (MONAI's ``cfg``) exists for concat conditioning only: it needs the condition it guides towards."""
    if cfg is None:
        return
    if conditioning is None:
        raise ValueError("cfg needs conditioning: classifier-free guidance combines the conditional and the unconditional prediction")
    if mode != "concat":
        raise ValueError(f"cfg is implemented for mode='concat' only, got mode={mode!r}")


def _check_mode(mode, conditioning, cfg=None) -> None:
    """What every sampling entry asks of (mode, conditioning, cfg): a known mode, guidance only where it exists, concat conditioning."""
    if mode not in ("crossattn", "concat"):
        raise NotImplementedError(f"{mode} condition is not supported")
    _check_cfg(cfg, conditioning, mode)
    if conditioning is not None and mode != "concat":
        raise NotImplementedError("cross-attention conditioning is not on the reference's path (mode='concat')")


def _progress(it, verbose):
    """``it`` under a tqdm bar where ``verbose`` asks for one and tqdm is installed."""
    if verbose:
        try:
            from tqdm import tqdm
            return tqdm(it)
        except ImportError:
            pass
    return it


def _check_warm_start(scheduler, n_steps, init_latent, start_step, B=None) -> int:
    """What every sampling entry asks of (init_latent, start_step) -> k0: a warm start needs the latent it starts from, a row of the
    chain, and a scheduler whose rows are independent per timestep (a multistep chain is defined from its first row)."""
    k0 = int(start_step)
    if init_latent is None:
        if k0 != 0:
            raise ValueError(f"start_step = {start_step} needs init_latent: only a warm start begins past the first timestep")
        return 0
    refuse_multistep(scheduler, inpainting=False)
    if not 0 <= k0 < n_steps:
        raise ValueError(f"start_step must be in [0, {n_steps - 1}], got {start_step}")
    if init_latent.dim() != 5 or (B is not None and init_latent.shape[0] not in (1, B)):
        raise ValueError(f"init_latent must be [1 or B, C, d, h, w]{'' if B is None else f' with B = {B}'}, got {tuple(init_latent.shape)}")
    return k0


def _host_start(scheduler, init_latent, input_noise, t, B, init_inverted):
    """The start of a host-driven warm chain: ``init_latent`` itself where it already is the sample at timestep ``t`` (the output of
    ``invert``), else ``scheduler.add_noise(init_latent, input_noise, t)``."""
    z0 = init_latent.detach().to(torch.float32)
    if z0.shape[0] != B:
        z0 = z0.expand(B, -1, -1, -1, -1)
    z0 = z0.contiguous()
    if init_inverted:
        return z0.clone()
    if input_noise is None:
        raise ValueError("the host-driven warm start noises init_latent with input_noise: pass it, or fused_seed for a device draw")
    return scheduler.add_noise(original_samples=z0, noise=input_noise, timesteps=torch.full((B,), t, device=z0.device))


def _fused_start(sampler, tbuf, init_latent, input_noise, k0, B, seed, init_inverted):
    """The start of a warm chain on the device sampler: the counter and ``tbuf`` at row ``k0``, and the persistent image the steps
    update in place: ``init_latent`` itself (``init_inverted``) or its noising by ``sampler.start``."""
    sampler.seek(k0, tbuf)
    z0 = init_latent.detach().to(device=tbuf.device, dtype=torch.float32).contiguous()
    if init_inverted:
        return (z0 if z0.shape[0] == B else z0.expand(B, -1, -1, -1, -1)).contiguous().clone()
    return sampler.start(z0, k0, B, seed, noise=input_noise)


def latent_keep_mask(image_keep: torch.Tensor, factor: int) -> torch.Tensor:
    """The keep mask of a latent from the keep mask of its image ([D, H, W] or [1, 1, D, H, W], 1 = keep) -> [d, h, w]: a latent voxel
    is kept only if EVERY image voxel under it is kept, a min-pool by the autoencoder's ``factor`` (a trailing partial cell pools the
    voxels it has).  Plain torch, run once per scan."""
    m = image_keep
    if m.dim() == 5 and m.shape[0] == 1 and m.shape[1] == 1:
        m = m[0, 0]
    if m.dim() != 3:
        raise ValueError(f"the image keep mask must be [D, H, W] or [1, 1, D, H, W], got {tuple(image_keep.shape)}")
    m = m.detach().to(torch.float32)
    if not bool(((m == 0) | (m == 1)).all()):
        raise ValueError("the keep mask must hold only 0 (regenerate) and 1 (keep): soft masks are not implemented")
    f = int(factor)
    if f < 1:
        raise ValueError(f"factor must be at least 1, got {factor}")
    if f == 1:
        return m.contiguous()
    return (-torch.nn.functional.max_pool3d(-m[None, None], kernel_size=f, stride=f, ceil_mode=True))[0, 0].contiguous()


def _check_inpaint(scheduler, inpaint_latent, keep_mask, init_latent, start_step, shape):
    """What every sampling entry asks of (inpaint_latent, keep_mask) -> None, or (known [1 or B, C, d, h, w] fp32, keep [d, h, w] fp32)
    for a chain on latents of ``shape`` [B, C, d, h, w]: both or neither, a scheduler whose rows are independent per timestep (a
    multistep history is not defined across jumps), no warm start, a binary mask of the latent's spatial shape."""
    if inpaint_latent is None and keep_mask is None:
        return None
    if inpaint_latent is None or keep_mask is None:
        raise ValueError("inpainting needs both inpaint_latent (what to keep) and keep_mask (where to keep it)")
    refuse_multistep(scheduler, inpainting=True)
    if init_latent is not None or int(start_step) != 0:
        raise NotImplementedError("warm-started or inverted inpainting is not implemented: a repaint chain starts from noise")
    shape = tuple(int(s) for s in shape)
    if inpaint_latent.dim() != 5 or inpaint_latent.shape[0] not in (1, shape[0]) or tuple(inpaint_latent.shape[1:]) != shape[1:]:
        raise ValueError(f"inpaint_latent must be [1 or {shape[0]}, {', '.join(map(str, shape[1:]))}], got {tuple(inpaint_latent.shape)}")
    keep = check_keep_mask(keep_mask, shape[2:]).to(inpaint_latent.device)
    return inpaint_latent.detach().to(torch.float32).contiguous(), keep


def _host_step(scheduler, ts, reverse=False):
    """-> step(k, eps, t, image, **kw) -> the next image: the one host-driven scheduler step, number k over the timesteps ``ts``, on a
    stepper with a state of its own per chain (``chain_scheduler``) and with what the scheduler's ``step`` takes beside
    (``_step_kwargs``); ``reverse``: ``reversed_step``, a step of DDIM inversion."""
    if reverse:
        return lambda k, eps, t, image: scheduler.reversed_step(eps, t, image)[0]
    stepper = scheduler.chain_scheduler()
    return lambda k, eps, t, image, **kw: stepper.step(eps, t, image, **scheduler._step_kwargs(ts, k), **kw)[0]


class _Inpaint(NamedTuple):
    """An inpainting chain's arguments, checked: what to keep, where, the schedule's two numbers and the host-driven loop's draws."""
    known: torch.Tensor
    keep: torch.Tensor
    jump_length: int
    n_resample: int
    noise: Optional[Callable[[str, int], torch.Tensor]]


def _inpaint_host_chain(scheduler, image, inpaint: _Inpaint, model_eps):
    """The host-driven repaint chain from ``image``: per UNet call k of ``repaint_rows``, ``model_eps(image, t)`` -> the scheduler's own
    ``step`` -> ``repaint_merge`` (the known region put back at the level arrived at, then the jump back where the row says so).  The
    draws are ``inpaint.noise(stream, k)`` (stream "step" | "known" | "jump"; e.g. a RepaintSampler's accessors) or torch.randn."""
    known, keep, inpaint_noise = inpaint.known, inpaint.keep, inpaint.noise
    schedule, rows = repaint_rows(scheduler, inpaint.jump_length, inpaint.n_resample)
    ts = scheduler.timesteps.tolist()
    step = _host_step(scheduler, ts)
    image = image.detach().to(torch.float32).contiguous()

    def draw(stream, k):
        return torch.randn_like(image) if inpaint_noise is None else inpaint_noise(stream, k)

    for k, ((level, jump), row) in enumerate(zip(schedule, rows)):
        t = ts[level]
        eps = model_eps(image, t)
        kw = dict(noise=draw("step", k)) if row[4] != 0.0 and inpaint_noise is not None else {}
        image = step(level, eps, t, image, **kw)
        image = repaint_merge(image.contiguous(), known, keep, row[8:12], jump, z_known=draw("known", k) if row[9] != 0.0 else None,
                              z_jump=draw("jump", k) if jump and row[11] != 0.0 else None)
    return image


def _model_eps(diffusion_model, image, tbuf, cond=None, cfg=None, cfg_fill_value=-1.0):
    """The host-driven model call of one step: guided (``tbuf`` then has 2 B entries), conditioned or plain."""
    if cfg is not None:
        return _guided_eps(diffusion_model, image, tbuf, cond, cfg, cfg_fill_value)
    if cond is not None:
        return diffusion_model(x=image, timesteps=tbuf, context=None, cond=cond)
    return diffusion_model(x=image, timesteps=tbuf, context=None)


def _guided_eps(diffusion_model, image, tbuf2, conditioning, cfg, cfg_fill_value):
    """MONAI's guided model call, host-driven: one forward at batch 2 B on ``cat([image] * 2)`` with the condition
    ``cat([fill tensor, conditioning])`` (unconditional half first), then ``u + cfg * (c - u)`` (``ldm_guidance_combine``)."""
    B = image.shape[0]
    cond = conditioning.detach().to(device=image.device, dtype=torch.float32)
    both = diffusion_model(x=torch.cat([image] * 2, dim=0), timesteps=tbuf2, context=None,
                           cond=torch.cat([torch.full_like(cond, float(cfg_fill_value)), cond], dim=0))
    both = both.contiguous()
    out = torch.empty_like(both[:B])
    with torch.cuda.device(image.device):
        _lib.check(_lib.lib().ldm_guidance_combine(both[:B].data_ptr(), both[B:].data_ptr(), float(cfg), out.data_ptr(), out.numel(),
                                                   _lib.current_stream()))
    return out


class _Target(NamedTuple):
    """What a chain steps: ``fused_step(image, tbuf, sampler)`` is one device step in place, ``host_eps(image, t)`` the model's
    prediction for a host-driven step, ``tbuf`` the UNet's persistent timestep input (one entry per sample of a call, twice when guided)."""
    fused_step: Callable
    host_eps: Callable
    tbuf: torch.Tensor
    correct: Optional[Callable] = None        # host-driven measurement guidance: image after the scheduler's step -> the guided image
    finish: Optional[Callable] = None         # called once after the chain (measurement guidance: reads the per-step residual norms)


def _latent_target(model, B, device, conditioning, cfg, cfg_fill_value) -> _Target:
    """The full latent [B, C, d, h, w] as a chain's target: ``denoise_step``, or ``_model_eps`` on the whole batch."""
    tbuf = torch.empty((B if cfg is None else 2 * B,), dtype=torch.float32, device=device)
    cond = None if conditioning is None else conditioning.detach().to(torch.float32).contiguous()
    kw = {} if cfg is None else dict(guidance=cfg, guidance_fill=cfg_fill_value)

    def fused_step(image, tbuf, sampler):
        model.denoise_step(image, tbuf, sampler, cond=cond, **kw)

    def host_eps(image, t):
        tbuf.fill_(float(t))
        return _model_eps(model, image, tbuf, conditioning, cfg, cfg_fill_value)

    return _Target(fused_step, host_eps, tbuf)


def _measured_target(model, B, shape, device, conditioning, measurement, scheduler, fused, autoencoder=None, scale_factor=1.0) -> _Target:
    """The full latent as the target of a measurement-guided chain (guidance.py): fused, ``denoise_step_measured`` on the measurement's
    device state; host-driven, the module's forward under torch autograd (its data-only input backward) for zeta grad_x L, which
    ``correct`` subtracts after the scheduler's own ``step``.  Either way the per-step |r_b| stay on the device until ``finish``.
    An image-space measurement (``measurement.space == "image"``) also takes ``autoencoder`` and the inferer's ``scale_factor``: the
    fused step chains the decoder's data-only backward in, the host-driven one differentiates through ``autoencoder.decode`` too."""
    tbuf = torch.empty((B,), dtype=torch.float32, device=device)
    cond = None if conditioning is None else conditioning.detach().to(torch.float32).contiguous()
    n_steps = len(scheduler.timesteps)
    image_space = measurement.space == "image"
    if fused:
        ae = dict(autoencoder=autoencoder) if image_space else {}
        state = measurement.device_state(shape, device, n_steps, **ae, **(dict(scale_factor=scale_factor) if image_space else {}))

        def fused_step(image, tbuf, sampler):
            model.denoise_step_measured(image, tbuf, sampler, state, cond=cond, **ae)

        def finish():
            measurement.norms = state[1]["norm_table"].cpu()

        return _Target(fused_step, None, tbuf, None, finish)
    tgt, wgt = measurement.device_tensors(measurement.measured_shape(shape, autoencoder), device)
    fwd = getattr(model, "forward_data_only", None) or (lambda x, timesteps, cond=None: model(x=x, timesteps=timesteps, cond=cond))
    pending, norms = [], []
    decode = (lambda x0: autoencoder.decode_stage_2_outputs(x0 / scale_factor),) if image_space else ()

    def host_eps(image, t):
        tbuf.fill_(float(t))
        m, corr, norm = measurement.host_correction(lambda xg: fwd(xg, tbuf, cond), *decode, image, t, scheduler, tgt, wgt)
        pending.append(corr)
        norms.append(norm)
        return m

    def correct(image):
        return image - pending.pop()

    def finish():
        measurement.norms = torch.stack(norms).cpu() if norms else torch.zeros((0, B))

    return _Target(None, host_eps, tbuf, correct, finish)


def _window_grid(model, spatial, roi_size, sw_batch_size, device, guided, **grid_args):
    """-> (grid, chunk): the windows of ONE latent of ``spatial`` and how many of them a UNet call takes (default: all, halved until the
    workspace fits in half the free memory)."""
    from .sliding import WindowGrid, default_sw_batch
    grid = WindowGrid(spatial, roi_size, **grid_args)
    grid.check_model(model)
    chunk = default_sw_batch(model, grid, device, guided=guided) if sw_batch_size is None else int(sw_batch_size)
    if not 1 <= chunk <= grid.n_windows:
        raise ValueError(f"sw_batch_size must be in [1, {grid.n_windows}], got {chunk}")
    return grid, chunk


def _window_target(model, grid, chunk, cond_windows, device, cfg, cfg_fill_value) -> _Target:
    """The windows of ``grid`` over one latent as a chain's target: ``denoise_step_windows``, or gather -> ``_model_eps`` on ``chunk``
    windows per call -> blend."""
    nw = grid.n_windows
    kw = {} if cfg is None else dict(guidance=cfg, guidance_fill=cfg_fill_value)

    def fused_step(image, tbuf, sampler):
        model.denoise_step_windows(image, tbuf, sampler, grid, cond_windows=cond_windows, sw_batch_size=chunk, **kw)

    def host_eps(image, t):
        xw = grid.gather(image)
        eps_w = torch.empty((nw, model.out_channels) + grid.roi, dtype=torch.float32, device=image.device)
        for b0 in range(0, nw, chunk):
            nb = min(chunk, nw - b0)
            tb = torch.full((nb if cfg is None else 2 * nb,), float(t), dtype=torch.float32, device=image.device)
            cb = None if cond_windows is None else cond_windows[b0:b0 + nb]
            eps_w[b0:b0 + nb] = _model_eps(model, xw[b0:b0 + nb], tb, cb, cfg, cfg_fill_value)
        return grid.blend(eps_w)

    return _Target(fused_step, host_eps, torch.empty((chunk if cfg is None else 2 * chunk,), dtype=torch.float32, device=device))


def _run_chain(target: _Target, scheduler, image, *, fused, seed=None, k0=0, init_latent=None, init_inverted=False, B=1, inpaint=None,
               invert=None, step_noise=None, keep=None, every=100, verbose=False) -> torch.Tensor:
    """The one chain behind ``sample``, ``sample_sliding_window`` and ``invert`` -> the final latent of ``target``.  The rules they share:

    ``fused``: the loop runs on a device sampler, one ``target.fused_step`` per row, on ONE image updated in place (a copy of ``image``,
    so the caller's tensor stays as it was).  The sampler is the scheduler's ``inversion_sampler`` (``invert``: the timesteps of the
    reversed steps), its ``repaint_sampler`` (``inpaint``: an ``_Inpaint``) or its
    ``device_sampler``, the last two keyed by ``seed``.  A cold chain ``reset``s it; a warm one (``init_latent``: rows ``k0`` onwards)
    ``seek``s to row ``k0`` and starts from ``init_latent`` itself (``init_inverted``) or from ``sampler.start``'s noising of it, on
    ``image`` as the noise or on a device draw where ``image`` is None.

    Otherwise the loop is driven from the host: ``target.host_eps`` then ``_host_step`` per timestep, each chain on a stepper of its
    own; a warm chain starts from ``_host_start``; ``step_noise(t)`` supplies the step's z; an inpainting chain is
    ``_inpaint_host_chain`` (its draws: ``inpaint_noise``, which ``step_noise`` does not replace, and no intermediates).

    ``keep`` collects the image after every step made at a timestep divisible by ``every`` (copies where the loop works in place);
    ``verbose`` shows a tqdm bar over the steps."""
    if fused:
        if invert is not None:
            sampler = scheduler.inversion_sampler(len(invert))
        elif inpaint is not None:
            sampler = scheduler.repaint_sampler(inpaint.known, inpaint.keep, inpaint.jump_length, inpaint.n_resample, seed)
        else:
            sampler = scheduler.device_sampler(seed)
        if init_latent is None:
            image = image.detach().to(torch.float32).contiguous().clone()
            sampler.reset(target.tbuf)
        else:
            image = _fused_start(sampler, target.tbuf, init_latent, image, k0, B, seed, init_inverted)
        for t in _progress(sampler.timesteps[k0:], verbose):
            target.fused_step(image, target.tbuf, sampler)
            if keep is not None and t % every == 0:
                keep.append(image.clone())
        if target.finish is not None:
            target.finish()
        return image
    ts = scheduler.timesteps.tolist() if invert is None else invert
    if init_latent is not None:
        image = _host_start(scheduler, init_latent, image, ts[k0], B, init_inverted)
    elif inpaint is not None:
        if step_noise is not None or keep is not None:
            raise ValueError("the host-driven inpainting loop takes inpaint_noise, not step_noise, and keeps no intermediates")
        return _inpaint_host_chain(scheduler, image, inpaint, target.host_eps)
    step = _host_step(scheduler, ts, reverse=invert is not None)
    for k, t in enumerate(_progress(ts[k0:], verbose), k0):
        eps = target.host_eps(image, t)
        if step_noise is not None:
            image = step(k, eps, t, image, noise=step_noise(t) if t > 0 else None)
        else:
            image = step(k, eps, t, image)
        if target.correct is not None:
            image = target.correct(image)
        if keep is not None and t % every == 0:
            keep.append(image)
    if target.finish is not None:
        target.finish()
    return image


def resize_nearest(x: torch.Tensor, size: Sequence[int]) -> torch.Tensor:
    """``torch.nn.functional.interpolate(x, size=size, mode="nearest")`` of a 5-D fp32 CUDA tensor, on ldm_op_resize_nearest (PyTorch's
    index rule: src = min(floor(dst * float(in) / out), in - 1))."""
    if not (x.is_cuda and x.dim() == 5 and len(size) == 3):
        raise _lib.LdmError("resize_nearest: a CUDA tensor [N, C, d, h, w] and a size (D, H, W) are needed")
    xc = x.detach().to(torch.float32).contiguous()
    N, Cc, d, h, w = xc.shape
    D, H, W = (int(s) for s in size)
    out = torch.empty((N, Cc, D, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().ldm_op_resize_nearest(xc.data_ptr(), out.data_ptr(), N, Cc, d, h, w, D, H, W, _lib.current_stream()))
    return out


class LatentDiffusionInferer:
    def __init__(self, scheduler, scale_factor: float = 1.0, ldm_latent_shape=None, autoencoder_latent_shape=None):
        if ldm_latent_shape is not None or autoencoder_latent_shape is not None:
            raise NotImplementedError("latent resizing is not used by the reference")
        self.scheduler = scheduler
        self.scale_factor = scale_factor

    def _decode(self, autoencoder_model, image):
        """The tail of every chain: latent / scale_factor through the autoencoder (None: the latent itself)."""
        latent = image if self.scale_factor == 1.0 else image / self.scale_factor
        return autoencoder_model.decode_stage_2_outputs(latent) if autoencoder_model is not None else latent

    def __call__(self, inputs: torch.Tensor, autoencoder_model, diffusion_model, noise: torch.Tensor,
                 timesteps: torch.Tensor, condition: Optional[torch.Tensor] = None, mode: str = "crossattn",
                 seg: Optional[torch.Tensor] = None, vae_eps: Optional[torch.Tensor] = None, return_target: bool = False):
        """Training-time forward: z = AE.encode_stage_2_inputs(inputs) * scale -> add_noise -> UNet.  ``return_target`` (extension)
        returns (prediction, target) instead, target = the regression target of the scheduler's prediction_type: ``noise`` itself
        for "epsilon", z for "sample", scheduler.get_velocity(z, noise, t) for "v_prediction", z - noise for an RFlowScheduler
        (written in the same kernel pass as the noisy latent)."""
        if mode not in ("crossattn", "concat"):
            raise NotImplementedError(f"{mode} condition is not supported")
        with torch.no_grad():
            if vae_eps is not None:
                latent = autoencoder_model.encode_stage_2_inputs(inputs, vae_eps)
            else:
                latent = autoencoder_model.encode_stage_2_inputs(inputs)
            if self.scale_factor != 1.0:
                latent = latent * self.scale_factor
        if return_target:
            noisy, target = self.scheduler.add_noise_and_target(original_samples=latent, noise=noise, timesteps=timesteps)
        else:
            noisy = self.scheduler.add_noise(original_samples=latent, noise=noise, timesteps=timesteps)
        if condition is not None and mode != "concat":
            raise NotImplementedError("cross-attention conditioning is not on the reference's path (mode='concat')")
        pred = _model_eps(diffusion_model, noisy, timesteps, condition)
        return (pred, target) if return_target else pred

    @torch.no_grad()
    def sample(self, input_noise: torch.Tensor, autoencoder_model, diffusion_model, scheduler=None,
               save_intermediates: bool = False, intermediate_steps: int = 100,
               conditioning: Optional[torch.Tensor] = None, mode: str = "crossattn", verbose: bool = False,
               seg: Optional[torch.Tensor] = None, step_noise: Optional[Callable[[int], torch.Tensor]] = None,
               fused_seed: Optional[int] = None, cfg: Optional[float] = None,
               cfg_fill_value: float = -1.0, init_latent: Optional[torch.Tensor] = None, start_step: int = 0,
               init_inverted: bool = False, inpaint_latent: Optional[torch.Tensor] = None, keep_mask: Optional[torch.Tensor] = None,
               jump_length: int = 1, n_resample: int = 1, inpaint_noise: Optional[Callable[[str, int], torch.Tensor]] = None,
               measurement=None) -> Union[torch.Tensor, tuple]:
        """Reverse diffusion over scheduler.timesteps then VAE decode of latent / scale_factor: validate, build the target, ``_run_chain``,
        decode.  ``_run_chain`` states the rules this entry shares with ``sample_sliding_window`` and ``invert`` (which sampler, how a
        chain starts, the fused and the host-driven loop); below is what the arguments mean.  ``fused_seed`` (extension) runs
        the loop on the device-resident sampler: noise from Philox(seed) inside the step kernel, one HIP graph per step.  With a
        PNDMScheduler the loop makes ``len(scheduler.timesteps)`` UNet calls, each chain on a multistep state of its own.  With an
        RFlowScheduler ``fused_seed`` only selects the device path (a flow chain draws nothing), and the host-driven loop hands
        ``step`` the next timestep of the schedule.

        ``cfg`` / ``cfg_fill_value`` are MONAI's (>= 1.5) classifier-free guidance: every step runs the UNet once on a doubled batch, the
        unconditional half (its condition filled with ``cfg_fill_value``) first, and steps on ``u + cfg * (c - u)``.  With
        ``fused_seed`` the doubling happens inside the device step (``denoise_step(..., guidance=cfg)``).

        ``init_latent`` / ``start_step`` (extension) warm-start the chain: ``init_latent`` ([1 or B, C, d, h, w], a scaled latent such
        as the low-count scan's own) is noised to ``timesteps[start_step]`` and only ``timesteps[start_step:]`` are denoised, n -
        start_step UNet calls instead of n (SDEdit; ``schedulers.start_step_for_strength`` maps a strength to a start step).  With
        ``fused_seed`` the start is one launch of ``DeviceSampler.start`` on ``input_noise`` or, with ``input_noise=None``, on a
        device draw keyed by the seed; the host-driven loop starts from ``scheduler.add_noise(init_latent, input_noise,
        timesteps[start_step])``.  ``init_inverted=True`` takes ``init_latent`` as already being the sample at
        ``timesteps[start_step]`` (the output of ``invert``) and adds no noise.  A multistep scheduler (PNDM, DPM-Solver++) has no warm
        start (NotImplementedError).

        ``inpaint_latent`` / ``keep_mask`` (extension) inpaint: the chain keeps ``inpaint_latent`` ([1 or B, C, d, h, w], a scaled latent)
        where ``keep_mask`` ([d, h, w] or [1, 1, d, h, w], values 0 / 1) is 1 and regenerates the rest (RePaint): after every scheduler
        step the kept region is replaced by the known latent at the noise level the step arrived at, and with ``n_resample`` > 1 the
        chain jumps back ``jump_length`` levels and denoises them again, ``schedulers.repaint_schedule`` UNet calls in all.  With
        ``fused_seed`` those are ``n_calls`` calls of ``denoise_step`` on ``scheduler.repaint_sampler(...)``; the host-driven loop runs
        ``step`` then ``schedulers.repaint_merge`` on torch draws (or on ``inpaint_noise(stream, row)``).  The final latent equals
        ``inpaint_latent`` bit for bit where the mask is 1.  Refused: a multistep scheduler and a warm start (NotImplementedError), a mask
        with any other value (ValueError).

        ``measurement`` (extension; a ``guidance.ConsistencyGuidance``) steers every step by the gradient of the measurement's loss on the
        model's own unclipped x0_hat (diffusion posterior sampling): x_{t-1} = step(m, t, x_t) - zeta grad_x L.  With ``fused_seed`` a
        step is ``denoise_step_measured`` (training forward, residual kernel, data-only input backward, sampler step, update kernel; the
        host reads nothing); the host-driven loop differentiates the loss through the module's forward with torch autograd.  DDPM and
        DDIM, every prediction type, concat conditioning and warm starts; refused (NotImplementedError, before anything is launched):
        PNDM, DPM-Solver++ and rectified flow, ``cfg`` and inpainting.  ``measurement.norms`` holds |r_b| per step afterwards.
        A ``guidance.ImageConsistencyGuidance`` measures the DECODED prediction ``autoencoder_model.decode(x0_hat / scale_factor)``
        instead: it needs ``autoencoder_model`` (ValueError without it, or when its latent channels are not the latent's); the fused step
        is ``denoise_step_measured(..., autoencoder=autoencoder_model)``, the host-driven loop differentiates through
        ``AutoencoderKL.decode`` as well.  The same refusals."""
        _check_mode(mode, conditioning, cfg)
        scheduler = scheduler or self.scheduler
        if measurement is not None:
            check_measurable(scheduler, cfg=cfg, inpaint=inpaint_latent is not None or keep_mask is not None)
        ref = input_noise if input_noise is not None else conditioning if conditioning is not None else init_latent
        if ref is None:
            raise ValueError("sample needs input_noise (or init_latent for a warm start)")
        B = ref.shape[0]
        inpaint = _check_inpaint(scheduler, inpaint_latent, keep_mask, init_latent, start_step, ref.shape)
        if inpaint is not None and input_noise is None:
            raise ValueError("an inpainting chain starts from input_noise")
        k0 = _check_warm_start(scheduler, len(scheduler.timesteps), init_latent, start_step, B)
        intermediates: Optional[List[torch.Tensor]] = [] if save_intermediates else None
        fused = fused_seed is not None and step_noise is None and hasattr(diffusion_model, "denoise_step")
        if measurement is not None:
            lat = input_noise if input_noise is not None else init_latent
            if lat is None:
                raise ValueError("a measurement-guided chain needs input_noise or init_latent for the latent's shape")
            shape = (B,) + tuple(lat.shape[1:])
            measurement.check(measurement.measured_shape(shape, autoencoder_model))
            target = _measured_target(diffusion_model, B, shape, ref.device, conditioning, measurement, scheduler, fused,
                                      autoencoder_model, self.scale_factor)
        else:
            target = _latent_target(diffusion_model, B, ref.device, conditioning, cfg, cfg_fill_value)
        image = _run_chain(target, scheduler, input_noise, seed=fused_seed, k0=k0, init_latent=init_latent, init_inverted=init_inverted, B=B,
                           fused=fused,
                           inpaint=inpaint and _Inpaint(*inpaint, jump_length, n_resample, inpaint_noise), step_noise=step_noise,
                           keep=intermediates, every=intermediate_steps, verbose=verbose)
        out = self._decode(autoencoder_model, image)
        if save_intermediates:
            return out, [autoencoder_model.decode_stage_2_outputs(x / self.scale_factor) for x in intermediates]
        return out

    @torch.no_grad()
    def invert(self, latent: torch.Tensor, diffusion_model, scheduler=None, conditioning: Optional[torch.Tensor] = None,
               mode: str = "concat", n_steps: Optional[int] = None, cfg: Optional[float] = None, cfg_fill_value: float = -1.0,
               fused: bool = True, eta: float = 0.0, roi_size: Optional[Sequence[int]] = None, overlap: float = 0.25,
               sw_batch_size: Optional[int] = None, sw_mode: str = "gaussian") -> torch.Tensor:
        """DDIM inversion of a scaled ``latent`` [B, C, d, h, w] (extension; MONAI's ``DDIMScheduler.reversed_step`` loop): ``n_steps``
        reversed steps over ``reversed(scheduler.timesteps)``, each the UNet at the current timestep then ``reversed_step`` -> the
        latent at the timestep reached.  The default, all n steps, is MONAI's loop and ends past ``timesteps[0]``.  With n =
        ``len(timesteps)``, ``n - 1 - k0`` steps land exactly on ``timesteps[k0]``: step j leaves ``timesteps[n - 1 - j]`` for
        ``timesteps[n - 1 - j] + T // n = timesteps[n - 2 - j]``, so ``sample(..., init_latent=invert(z, n_steps=n - 1 - k0),
        start_step=k0, init_inverted=True)`` denoises from where the inversion stopped.  Only a DDIMScheduler with ``eta = 0`` inverts
        (a stochastic or multistep sampler has no such map): anything else raises.  ``fused=True`` steps ``denoise_step`` on
        ``scheduler.inversion_sampler(n_steps)``, one HIP graph launch per step in graph mode; ``fused=False`` drives ``reversed_step``
        from the host, bit for bit the same.  ``roi_size`` (fused only): ONE latent larger than the UNet's window, inverted with the
        windowed step of ``sample_sliding_window`` (``overlap`` / ``sw_batch_size`` / ``sw_mode`` are its arguments)."""
        scheduler = scheduler or self.scheduler
        if not hasattr(scheduler, "reversed_step"):
            raise NotImplementedError(f"DDIM inversion needs a DDIMScheduler, you are using {type(scheduler).__name__}")
        if float(eta) != 0.0:
            raise ValueError(f"DDIM inversion needs the deterministic sampler (eta = 0), got eta = {eta}")
        _check_mode(mode, conditioning, cfg)
        if not latent.is_cuda or latent.dim() != 5:
            raise _lib.LdmError("invert: a CUDA latent [B, C, d, h, w] is needed (no CPU fallback)")
        ts = scheduler.inversion_timesteps(n_steps)
        image = latent.detach().to(torch.float32).contiguous()
        B, dev = image.shape[0], image.device
        cond = None if conditioning is None else conditioning.detach().to(device=dev, dtype=torch.float32).contiguous()
        if roi_size is None:
            target = _latent_target(diffusion_model, B, dev, cond, cfg, cfg_fill_value)
        else:
            if not fused or B != 1:
                raise ValueError("invert with roi_size is the fused windowed step on one latent [1, C, D, H, W]")
            grid, chunk = _window_grid(diffusion_model, image.shape[2:], roi_size, sw_batch_size, dev, cfg is not None, overlap=overlap,
                                       mode=sw_mode)
            if cond is not None and tuple(cond.shape[2:]) != grid.shape:
                raise ValueError(f"conditioning must have the latent's spatial shape {grid.shape}, got {tuple(cond.shape)}")
            target = _window_target(diffusion_model, grid, chunk, None if cond is None else grid.gather(cond), dev, cfg, cfg_fill_value)
        return _run_chain(target, scheduler, image if fused else image.clone(), fused=fused, invert=ts)     # never the caller's tensor

    @torch.no_grad()
    def get_likelihood(self, inputs: torch.Tensor, autoencoder_model, diffusion_model, scheduler=None, save_intermediates: bool = False,
                       conditioning: Optional[torch.Tensor] = None, mode: str = "crossattn",
                       original_input_range: Optional[tuple] = (0, 255), scaled_input_range: Optional[tuple] = (0, 1),
                       verbose: bool = True, resample_latent_likelihoods: bool = False, resample_interpolation_mode: str = "nearest",
                       seg: Optional[torch.Tensor] = None, *, noise: Optional[torch.Tensor] = None, fused_seed: Optional[int] = None,
                       return_terms: bool = False):
        """MONAI's ``LatentDiffusionInferer.get_likelihood`` (>= 1.4, restated): the variational bound of ``inputs``' latent under the
        model, in nats per dimension -> ``total_kl`` [B], or ``(total_kl, intermediates)`` with ``save_intermediates``: one per-element
        map per timestep on the CPU, resized to ``inputs.shape[2:]`` with ``resample_latent_likelihoods`` ("nearest" only here).
        latent = ``autoencoder_model.encode_stage_2_inputs(inputs) * scale_factor``; ``autoencoder_model=None``: ``inputs`` is the latent.
        For every t of ``scheduler.timesteps`` (a DDPMScheduler; anything else raises NotImplementedError, as in MONAI): the KL between
        q(x_{t-1} | x_t, x0) and the model's p(x_{t-1} | x_t), at t = 0 the discretised decoder log-likelihood with bins of
        ``(scaled range) / (original range)``; one noise tensor serves every t.  The arithmetic is csrc/likelihood.h's.  With
        ``variance_type="fixed_small"`` the t = 0 variance is 1e-20 and that term is a step function (0 or 27.631 per element): MONAI's
        behaviour, kept.

        Extensions: ``noise`` supplies z (default ``torch.randn_like(latent)``, as MONAI draws it); ``fused_seed`` runs the
        device-resident loop instead (``DiffusionModelUNet.likelihood_step``: z from Philox(seed), one HIP graph launch per timestep,
        bit-identical to the host-driven loop on ``DeviceLikelihood.noise``); ``return_terms`` appends the [n_steps, B] per-timestep
        means to the return."""
        scheduler = scheduler or self.scheduler
        if not hasattr(scheduler, "likelihood_rows"):
            raise NotImplementedError(f"Likelihood computation is only compatible with DDPMScheduler, you are using {type(scheduler).__name__}")
        _check_mode(mode, conditioning)
        if resample_latent_likelihoods and resample_interpolation_mode not in ("nearest", "bilinear", "trilinear"):
            raise ValueError(f"resample_interpolation mode should be either nearest, bilinear, or trilinear, got {resample_interpolation_mode}")
        if resample_latent_likelihoods and resample_interpolation_mode != "nearest":
            raise NotImplementedError(f"resample_interpolation_mode={resample_interpolation_mode!r} is not implemented: only 'nearest' is")
        if noise is not None and fused_seed is not None:
            raise ValueError("noise and fused_seed both choose z: pass one of them")
        latent = inputs if autoencoder_model is None else autoencoder_model.encode_stage_2_inputs(inputs)
        if self.scale_factor != 1.0:
            latent = latent * self.scale_factor
        x0 = latent.detach().to(torch.float32).contiguous()
        if not x0.is_cuda or x0.dim() != 5:
            raise _lib.LdmError("get_likelihood: a CUDA latent [B, C, D, H, W] is needed (no CPU fallback)")
        dev, B = x0.device, x0.shape[0]
        cond = None if conditioning is None else conditioning.detach().to(device=dev, dtype=torch.float32).contiguous()
        bin_width = (scaled_input_range[1] - scaled_input_range[0]) / (original_input_range[1] - original_input_range[0])
        lik = DeviceLikelihood(scheduler, 0 if fused_seed is None else fused_seed, bin_width)
        it = _progress(lik.timesteps, verbose)
        total = torch.zeros((B,), dtype=torch.float32, device=dev)
        terms = torch.zeros((lik.n_steps, B), dtype=torch.float32, device=dev)
        tbuf = torch.empty((B,), dtype=torch.float32, device=dev)
        kl_map = torch.empty_like(x0) if save_intermediates else None
        intermediates: List[torch.Tensor] = []

        def keep():
            m = kl_map if not resample_latent_likelihoods else resize_nearest(kl_map, inputs.shape[2:])
            intermediates.append(m.cpu())

        if fused_seed is not None and hasattr(diffusion_model, "likelihood_step"):
            x_t = torch.empty_like(x0)
            lik.reset(x0, x_t, tbuf, total)
            for _ in it:
                diffusion_model.likelihood_step(x0, x_t, tbuf, lik, total, cond=cond, kl_map=kl_map, terms=terms)
                if save_intermediates:
                    keep()
        else:
            z = torch.randn_like(x0) if noise is None else noise.detach().to(device=dev, dtype=torch.float32).contiguous()
            if z.shape != x0.shape:
                raise ValueError(f"noise must have the latent's shape {tuple(x0.shape)}, got {tuple(z.shape)}")
            x_t = torch.empty_like(x0)
            for k, t in enumerate(it):
                lik.noisy(x0, z, k, out=x_t)
                tbuf.fill_(float(t))
                m = _model_eps(diffusion_model, x_t, tbuf, cond)
                lik.term(x0, x_t, m.contiguous(), k, total, kl_map=kl_map, term_out=terms[k])
                if save_intermediates:
                    keep()
        out = (total, intermediates) if save_intermediates else (total,)
        if return_terms:
            out = out + (terms,)
        return out[0] if len(out) == 1 else out

    @torch.no_grad()
    def sample_sliding_window(self, input_noise: torch.Tensor, autoencoder_model, diffusion_model, roi_size: Sequence[int],
                              overlap: float = 0.25, sw_batch_size: Optional[int] = None, mode: str = "gaussian",
                              sigma_scale: float = 0.125, conditioning: Optional[torch.Tensor] = None, scheduler=None,
                              fused_seed: Optional[int] = None, cfg: Optional[float] = None,
                              cfg_fill_value: float = -1.0, init_latent: Optional[torch.Tensor] = None, start_step: int = 0,
                              init_inverted: bool = False, inpaint_latent: Optional[torch.Tensor] = None, keep_mask: Optional[torch.Tensor] = None,
                              jump_length: int = 1, n_resample: int = 1, inpaint_noise: Optional[Callable[[str, int], torch.Tensor]] = None,
                              measurement=None) -> torch.Tensor:
        """Reverse diffusion of ONE latent larger than the UNet's training window (extension; MONAI's sliding-window inference
        inside every denoising step): each step cuts the latent into overlapping ``roi_size`` windows (``sliding.WindowGrid``),
        runs the UNet on ``sw_batch_size`` windows per call (default: all, halved until the workspace fits in half the free
        memory), blends the eps predictions with the importance map and takes one scheduler step on the whole latent; then the
        autoencoder decodes the whole latent / scale_factor.  ``conditioning`` (mode="concat") has the latent's spatial shape.
        With ``fused_seed`` the step runs on the device sampler (``denoise_step_windows``: one HIP graph launch per step in graph
        mode); without it the loop is driven from the host on the RNG stream ``sample`` uses.  ``cfg`` / ``cfg_fill_value``: classifier-free
        guidance as in ``sample``, window by window (each UNet call then runs twice its windows).  ``init_latent`` / ``start_step`` /
        ``init_inverted``: the warm start of ``sample`` on the whole latent [1, C, D, H, W]; the start is noised once, not per window,
        and ``input_noise`` may be None where ``sample`` allows it.  ``inpaint_latent`` / ``keep_mask`` / ``jump_length`` / ``n_resample``:
        the inpainting of ``sample`` on the whole latent ([1, C, D, H, W] and [D, H, W]); the merge runs on the full latent inside the
        windowed step kernel, never per window.  ``measurement``: refused (NotImplementedError; see ``sample``)."""
        _check_cfg(cfg, conditioning, "concat")
        scheduler = scheduler or self.scheduler
        if measurement is not None:
            check_measurable(scheduler, windows=True)
        ref = input_noise if input_noise is not None else init_latent
        if ref is None or ref.dim() != 5 or ref.shape[0] != 1:
            raise ValueError(f"sample_sliding_window takes one volume [1, C, D, H, W], got {None if ref is None else tuple(ref.shape)}")
        k0 = _check_warm_start(scheduler, len(scheduler.timesteps), init_latent, start_step, 1)
        if init_latent is not None and tuple(init_latent.shape) != tuple(ref.shape):
            raise ValueError(f"init_latent must be {tuple(ref.shape)}, got {tuple(init_latent.shape)}")
        inpaint = _check_inpaint(scheduler, inpaint_latent, keep_mask, init_latent, start_step, ref.shape)
        grid, chunk = _window_grid(diffusion_model, ref.shape[2:], roi_size, sw_batch_size, ref.device, cfg is not None, overlap=overlap,
                                   mode=mode, sigma_scale=sigma_scale)
        cw = None
        if conditioning is not None:
            if conditioning.dim() != 5 or conditioning.shape[0] != 1 or tuple(conditioning.shape[2:]) != grid.shape:
                raise ValueError(f"conditioning must be [1, C, {', '.join(map(str, grid.shape))}], got {tuple(conditioning.shape)}")
            cw = grid.gather(conditioning)
        target = _window_target(diffusion_model, grid, chunk, cw, ref.device, cfg, cfg_fill_value)
        image = _run_chain(target, scheduler, input_noise, fused=fused_seed is not None, seed=fused_seed, k0=k0, init_latent=init_latent,
                           init_inverted=init_inverted,
                           inpaint=inpaint and _Inpaint(*inpaint, jump_length, n_resample, inpaint_noise))
        return self._decode(autoencoder_model, image)

    @torch.no_grad()
    def sample_ensemble(self, n_members: int, latent_shape: Sequence[int], autoencoder_model, diffusion_model, scheduler=None,
                        conditioning: Optional[torch.Tensor] = None, mode: str = "concat", member_batch: Optional[int] = None,
                        seed: int = 0, cfg: Optional[float] = None, cfg_fill_value: float = -1.0,
                        roi_size: Optional[Sequence[int]] = None, overlap: float = 0.25, sw_batch_size: Optional[int] = None,
                        sw_mode: str = "gaussian", output_crop: Optional[Sequence[int]] = None, keep_members: int = 0,
                        target: Optional[torch.Tensor] = None, ddof: int = 1, init_latent: Optional[torch.Tensor] = None,
                        start_step: int = 0, inpaint_latent: Optional[torch.Tensor] = None, keep_mask: Optional[torch.Tensor] = None,
                        jump_length: int = 1, n_resample: int = 1, measurement=None):
        """``n_members`` draws of the same scan's posterior, reduced on the device as they are decoded (extension): returns
        ``EnsembleResult(mean, std, count, stats, members)``, mean / std [1, C, D, H, W] per voxel over the members (``std`` with
        ``ddof``), ``stats`` the Python floats of ``EnsembleAccumulator.stats(target, ddof)``, ``members`` the first ``keep_members``
        volumes or None.  No stack of the decoded volumes is held: each decoded chunk is folded by ``EnsembleAccumulator.update``.

        Member k starts from ``torch.randn(latent_shape, generator=Generator().manual_seed(seed + k))`` ([C, d, h, w], drawn on the host
        and moved), whatever ``member_batch`` is.  Members run ``member_batch`` at a time (default: all, halved until the UNet's
        workspace fits in half the free memory) through ``sample(..., fused_seed=seed + first)`` with the [1, ...] ``conditioning``
        expanded to the chunk.  With ``roi_size`` each member is one ``sample_sliding_window(..., fused_seed=seed + k)`` over the
        whole latent instead (``overlap`` / ``sw_batch_size`` / ``sw_mode`` are its arguments) and ``member_batch`` must be None or 1.
        ``output_crop`` (D, H, W) keeps the leading corner of every decoded volume (a padded whole scan's own shape).

        Limit: a stochastic sampler (DDPM, DDIM with eta > 0) draws its step noise from Philox keyed by the chunk's seed and the
        element's position in the chunk, so such an ensemble reproduces only for the same ``(seed, n_members, member_batch)``; the
        deterministic samplers (DDIM with eta = 0, PNDM, rectified flow) give the same members under any chunking up to the batch
        dependence of the UNet's own summation order.

        ``init_latent`` [1, C, d, h, w] / ``start_step``: every member is a warm chain (see ``sample``) from the same scaled latent.
        Member k then starts from ``DeviceSampler.start``'s device draw keyed by ``(seed, k)`` (no host ``torch.randn``, and the one
        latent is broadcast inside the kernel, never copied per member), whatever ``member_batch`` is; the limit above on the STEP noise
        of a stochastic sampler stays.

        ``inpaint_latent`` [1, C, d, h, w] / ``keep_mask`` / ``jump_length`` / ``n_resample``: every member is an inpainting chain (see
        ``sample``) that keeps the same latent under the same mask: the one known latent is bound with ``known_batch = 1`` and read by
        every member of a chunk, never copied per member (the known-region and jump draws are keyed like the step noise: by the chunk's
        seed and the position in the chunk, so the limit above holds for every base sampler), so the kept region of every member is bitwise the known latent and the
        spread lives in the regenerated region alone.  ``measurement``: refused (NotImplementedError; see ``sample``)."""
        if measurement is not None:
            check_measurable(scheduler or self.scheduler, ensemble=True)
        from .ensemble import EnsembleAccumulator, EnsembleResult, default_member_batch, plan_chunks
        K = int(n_members)
        if K < 2:
            raise ValueError(f"an ensemble needs n_members >= 2, got {n_members}")
        _check_mode(mode, conditioning, cfg)
        if ddof not in (0, 1):
            raise ValueError(f"ddof must be 0 or 1, got {ddof}")
        latent_shape = tuple(int(s) for s in latent_shape)
        if len(latent_shape) != 4:
            raise ValueError(f"latent_shape is one member's [C, d, h, w], got {latent_shape}")
        keep = int(keep_members)
        if not 0 <= keep <= K:
            raise ValueError(f"keep_members must be in [0, {K}], got {keep_members}")
        scheduler = scheduler or self.scheduler
        k0 = _check_warm_start(scheduler, len(scheduler.timesteps), init_latent, start_step, 1)
        if init_latent is not None and tuple(init_latent.shape) != (1,) + latent_shape:
            raise ValueError(f"init_latent must be {(1,) + latent_shape}, got {tuple(init_latent.shape)}")
        inpaint = _check_inpaint(scheduler, inpaint_latent, keep_mask, init_latent, start_step, (1,) + latent_shape)
        dev = next(diffusion_model.parameters()).device
        cond = None
        if conditioning is not None:
            if conditioning.dim() != 5 or conditioning.shape[0] != 1 or tuple(conditioning.shape[2:]) != latent_shape[1:]:
                raise ValueError(f"conditioning must be [1, C, {', '.join(map(str, latent_shape[1:]))}], got {tuple(conditioning.shape)}")
            cond = conditioning.detach().to(device=dev, dtype=torch.float32)
        if roi_size is not None:
            if member_batch not in (None, 1):
                raise ValueError("with roi_size every member is one sliding-window chain: member_batch must be None or 1")
            member_batch = 1
        elif member_batch is None:
            member_batch = default_member_batch(diffusion_model, K, latent_shape[1:], dev, guided=cfg is not None)
        if not 1 <= int(member_batch) <= K:
            raise ValueError(f"member_batch must be in [1, {K}], got {member_batch}")

        def start(k):
            return torch.randn(latent_shape, generator=torch.Generator().manual_seed(int(seed) + k), dtype=torch.float32)

        warm, starter = {}, None
        if init_latent is not None:
            z0 = init_latent.detach().to(device=dev, dtype=torch.float32).contiguous()
            starter = scheduler.device_sampler(int(seed))          # the row table the starts are noised with
            warm = dict(start_step=k0, init_inverted=True)         # the chunk arrives noised: sample only seeks
        if inpaint is not None:
            warm = dict(inpaint_latent=inpaint[0].to(dev), keep_mask=inpaint[1].to(dev), jump_length=jump_length, n_resample=n_resample)

        acc, kept = None, []
        for first, nb in plan_chunks(K, int(member_batch)):
            if starter is not None:
                z = warm["init_latent"] = starter.start(z0, k0, nb, int(seed), first_member=first)
            else:
                z = torch.stack([start(first + j) for j in range(nb)]).to(dev)
            if roi_size is not None:
                vol = self.sample_sliding_window(z, autoencoder_model, diffusion_model, roi_size, overlap=overlap, sw_batch_size=sw_batch_size,
                                                 mode=sw_mode, conditioning=cond, scheduler=scheduler, fused_seed=int(seed) + first,
                                                 cfg=cfg, cfg_fill_value=cfg_fill_value, **warm)
            else:
                kw = {} if cond is None else dict(conditioning=cond.expand(nb, -1, -1, -1, -1).contiguous(), mode="concat")
                vol = self.sample(z, autoencoder_model, diffusion_model, scheduler=scheduler, fused_seed=int(seed) + first, cfg=cfg,
                                  cfg_fill_value=cfg_fill_value, **warm, **kw)
            vol = vol.to(torch.float32)
            if output_crop is not None:
                d, h, w = (int(s) for s in output_crop)
                if not all(1 <= c <= s for c, s in zip((d, h, w), vol.shape[2:])):
                    raise ValueError(f"output_crop {tuple(output_crop)} does not fit the decoded volume {tuple(vol.shape[2:])}")
                vol = vol[:, :, :d, :h, :w]
            vol = vol.contiguous()
            if acc is None:
                acc = EnsembleAccumulator(vol.shape[1:], vol.device)
            acc.update(vol)
            for j in range(nb):
                if first + j < keep:
                    kept.append(vol[j].clone())
        stats = acc.stats(target=target, ddof=ddof)
        return EnsembleResult(acc.mean()[None], acc.std(ddof=ddof)[None], acc.count, stats, torch.stack(kept) if kept else None)

    @torch.no_grad()
    def sample_concurrent(self, input_noises: Sequence[torch.Tensor], autoencoder_model, diffusion_models: Sequence,
                          scheduler=None, conditionings: Optional[Sequence[Optional[torch.Tensor]]] = None,
                          mode: str = "crossattn", measurement=None) -> List[torch.Tensor]:
        """K independent reverse-diffusion chains on one GPU, one stream and one module instance per chain, advanced
        round-robin from this thread so that the launches of different chains overlap (a single B = 1 chain is bound by the
        per-launch floor: DESIGN.md sections 3.5 / 5c).  Same arithmetic per chain as ``sample``; returns the decoded volumes.
        Not in the reference (it samples one volume at a time, 3d_ldm/inference.py:88-102)."""
        if measurement is not None:
            check_measurable(scheduler or self.scheduler, concurrent=True)
        if len(diffusion_models) < len(input_noises):
            raise ValueError("one diffusion model instance per chain is needed (each owns a workspace and a launch graph)")
        scheduler = scheduler or self.scheduler
        conds = list(conditionings) if conditionings is not None else [None] * len(input_noises)
        if any(c is not None for c in conds) and mode != "concat":
            raise NotImplementedError("cross-attention conditioning is not on the reference's path (mode='concat')")
        dev = input_noises[0].device
        main = torch.cuda.current_stream(dev)
        streams = [torch.cuda.Stream(device=dev) for _ in input_noises]
        images = list(input_noises)
        tbufs = []
        for st, img in zip(streams, images):
            st.wait_stream(main)
            tbufs.append(torch.empty((img.shape[0],), dtype=torch.float32, device=dev))
        ts = scheduler.timesteps.tolist()
        steps = [_host_step(scheduler, ts) for _ in images]
        for j, t in enumerate(ts):
            for k, st in enumerate(streams):
                with torch.cuda.stream(st):
                    tbufs[k].fill_(float(t))
                    eps = _model_eps(diffusion_models[k], images[k], tbufs[k], conds[k])
                    images[k] = steps[k](j, eps, t, images[k])
        outs = []
        for k, st in enumerate(streams):                    # the autoencoder (one workspace) decodes the chains one after another
            main.wait_stream(st)
            images[k].record_stream(main)
            outs.append(self._decode(autoencoder_model, images[k]))
        return outs
