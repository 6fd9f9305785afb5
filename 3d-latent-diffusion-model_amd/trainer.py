"""Data-parallel training step of the latent-diffusion UNet.

Reference behaviour being reproduced (3d_ldm/train_diffusion.py):
  :100-124  scale_factor = 1 / std(AE.encode_stage_2_inputs(first label batch)), averaged over ranks
  :147-149  DDP wrap: parameters broadcast from rank 0, gradients averaged over ranks during backward
  :155-156  Adam(lr) + MultiStepLR(milestones=[100, 1000], gamma=0.1), stepped once per epoch (:222-223)
  :172-223  per batch: noise drawn on the HOST then moved (:182), timesteps = randint on the device (:185-187),
            image latents (condition) under no_grad (:194-195), inferer(..., mode="concat") (:197-205), MSE (:207),
            NaN -> skip (:210-212), backward (:214), clip_grad_norm_(1.0) (:217), optimizer step (:219)

MI355X design: one process per GPU; the UNet's gradients live in ONE flat fp32 buffer written in place by the
hand-written backward plan, so the data-parallel exchange is a single (optionally chunked) all-reduce over RCCL/xGMI
issued right after backward, and clip + Adam are two fused launches over the flat buffers (``FlatAdam``).  Two
reference quirks are fixed on purpose: the NaN-skip is agreed across ranks (a single rank skipping
``backward`` dead-locks DDP in the reference) and decided ON THE DEVICE: a NaN loss makes every gradient NaN, the data-parallel
mean carries that to every rank, and the fused clip + Adam launch leaves parameters and moments untouched when the gradient norm is
not finite (``FlatAdam.skipped_steps``) -- no flag all-reduce and no host read inside the step; and the label encode that the
reference runs only to learn the latent shape (:179-181) is not executed (``reference_rng_order=True`` restores it).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.distributed as dist
import torch.nn.functional as F

from .optim import mse_loss


class GradSync:
    """Collectives of the data-parallel trainer over torch.distributed ("nccl" = RCCL on ROCm; "gloo" in CPU tests)."""

    def __init__(self, chunk_elems: int = 1 << 26, grad_dtype: torch.dtype = torch.float32):
        """``grad_dtype=torch.bfloat16`` (opt-in) sends the gradients as bf16: 382 instead of 765 MB per step for the benchmark
        UNet, for rings that are xGMI-link bound; the reference's DDP reduces fp32."""
        self.on = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        self.world = dist.get_world_size() if self.on else 1
        self.chunk = int(chunk_elems)                    # 64 Mi elements = 256 MB per collective
        self._avg = self.on and dist.get_backend() == "nccl"
        if grad_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("grad_dtype must be torch.float32 or torch.bfloat16")
        self.grad_dtype = grad_dtype
        self._modules = []                               # modules whose exchange runs inside backward on the library's communicator

    def _quiescent(self) -> None:
        """Two communicators live in a training process: torch.distributed's group (scalars, barriers, broadcasts, the fallback
        mean) and the library's own RCCL communicator on its comm stream (the buckets).  RCCL requires that two communicators never
        have collectives in flight in an order that differs between ranks; here that is excluded by construction -- every bucket is
        joined into the launch stream at the end of backward, and torch's collectives are ordered behind the launch stream -- and
        this check turns the construction into an assertion: a torch.distributed collective issued while a bucket is still un-joined
        is a programming error, not a race to be debugged on eight GPUs.

        Scope: the assertion guards the collectives issued THROUGH this class (every one the trainers and bench.py's ddp_train leg
        issue); code that calls torch.distributed directly is outside it.  The counter it reads is host bookkeeping: a backward that
        failed between a bucket and its join leaves it non-zero until the next backward begins (which orders itself behind the stray
        buckets and clears it: grad_sync_begin), so after such an error the next collective here raises rather than races."""
        from . import _lib
        L = _lib.lib()
        for m in self._modules:
            n = L.ldm_model_grad_sync_pending(m._h)
            if n:
                raise RuntimeError(f"torch.distributed collective while {n} gradient bucket(s) of the library's communicator are not joined")

    def attach(self, module, force_single: bool = False, transport=None, world: Optional[int] = None, rank: int = 0) -> bool:
        """Route the gradient exchange of ``module`` through the library's own RCCL communicator (``ldm_comm_*``) and overlap it
        with backward: ``loss.backward()`` then all-reduces (mean, fp32) the flat gradient buffer bucket by bucket on a comm
        stream while the backward plan is still running (``ldm_model_set_grad_sync``; DistributedDataParallel's bucketed hooks,
        3d_ldm/train_diffusion.py:147-149), and ``mean_`` becomes a no-op for that module.  The 128-byte RCCL unique id is made
        on rank 0 and broadcast over the existing torch.distributed group.  Only with the "nccl" backend on GPUs;
        ``grad_dtype=torch.bfloat16`` selects the library's bf16 wire format (``ldm_model_set_grad_wire``: cast, all-reduce, cast
        back on the comm stream); ``force_single`` builds a world-size-1 communicator without torch.distributed (tests, traces).

        ``transport(buf_ptr, count, dtype, op, stream_ptr) -> int`` (with ``world`` / ``rank``) replaces RCCL by a caller-supplied
        all-reduce (``ldm_comm_init_custom``): the test seam that lets one GPU play a rank of a world > 1 job.

        Every rank must build the same buckets, so rank 0's ``LDM_GRAD_BUCKET_MB`` is broadcast and written into this process's
        environment before any training plan exists.  If the communicator cannot be created (no librccl, a failing
        ``ncclCommInitRank``) the ranks agree on that and fall back together to ``mean_`` after backward instead of raising."""
        import ctypes as C
        import os
        import warnings
        from . import _lib
        L = _lib.lib()
        comm = C.c_void_p()
        if transport is not None:
            fn = _lib.ALLREDUCE_FN(lambda user, buf, count, dtype, op, stream: int(transport(buf, count, dtype, op, stream) or 0))
            _lib.check(L.ldm_comm_init_custom(int(rank), int(world or 1), C.cast(fn, C.c_void_p), None, C.byref(comm)))
            module._grad_transport = fn                      # the C function pointer must outlive the communicator
        else:
            single = force_single and not self.on
            if not single and not (self.on and dist.get_backend() == "nccl"):
                return False
            rank = 0 if single else dist.get_rank()
            world = 1 if single else self.world
            uid = C.create_string_buffer(128)
            # every rank probes librccl BEFORE any rank enters ncclCommInitRank (which blocks until all `world` ranks have joined):
            # a rank that cannot load it must make all of them fall back, not leave the others waiting inside the rendezvous
            ok = 1 if L.ldm_comm_rccl_version() > 0 else 0
            if ok and rank == 0 and L.ldm_comm_unique_id(uid) != 0:
                ok = 0
            if not single:
                flag = torch.tensor([float(ok)], device="cuda")
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                ok = int(flag.item())
            if ok and not single:
                try:
                    mb = int(os.environ.get("LDM_GRAD_BUCKET_MB", "48") or 48)
                except ValueError:
                    mb = 48
                mb = min(max(mb, 1), 0xFFFF)
                t = torch.tensor(list(uid.raw) + [mb & 0xFF, (mb >> 8) & 0xFF], dtype=torch.uint8, device="cuda")
                dist.broadcast(t, src=0)
                raw = bytes(t.cpu().tolist())
                uid = C.create_string_buffer(raw[:128], 128)
                os.environ["LDM_GRAD_BUCKET_MB"] = str(raw[128] | (raw[129] << 8))
            if ok and L.ldm_comm_init(rank, world, uid, C.byref(comm)) != 0:
                ok = 0
            if not single:                                   # all ranks or none
                flag = torch.tensor([float(ok)], device="cuda")
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                ok = int(flag.item())
            if not ok:
                msg = L.ldm_last_error()
                warnings.warn("in-library RCCL gradient exchange unavailable (%s): falling back to one all-reduce after backward "
                              "over torch.distributed" % (msg.decode() if msg else "?"))
                if comm:
                    L.ldm_comm_destroy(comm)
                return False
        _lib.check(L.ldm_model_set_grad_sync(module._h, comm))
        _lib.check(L.ldm_model_set_grad_wire(module._h, 1 if self.grad_dtype == torch.bfloat16 else 0))
        module._grad_comm = comm                         # keeps the handle alive as long as the module
        self._attached = getattr(self, "_attached", set()) | {id(module)}
        self._modules.append(module)
        return True

    def attached(self, module) -> bool:
        return id(module) in getattr(self, "_attached", set())

    def broadcast(self, flat: torch.Tensor, src: int = 0) -> None:
        """Parameter broadcast at wrap time (what DistributedDataParallel.__init__ does)."""
        if self.on:
            self._quiescent()
            dist.broadcast(flat, src=src)

    def mean_(self, flat: torch.Tensor) -> torch.Tensor:
        """In-place mean over ranks of a flat buffer; chunks are queued asynchronously and waited for together."""
        if not self.on:
            return flat
        self._quiescent()
        works, staged = [], []
        for lo in range(0, flat.numel(), self.chunk):
            part = flat[lo:lo + self.chunk]
            if self.grad_dtype != flat.dtype:              # reduced-precision wire format: cast, reduce, cast back
                if not self._avg:
                    part = part * (1.0 / self.world)       # pre-scale: the SUM of bf16 values then stays in range
                low = part.to(self.grad_dtype)
                staged.append((lo, low))
                part = low
            works.append(dist.all_reduce(part, op=dist.ReduceOp.AVG if self._avg else dist.ReduceOp.SUM, async_op=True))
        for w in works:
            w.wait()
        for lo, low in staged:
            flat[lo:lo + low.numel()].copy_(low)
        if not self._avg and not staged:
            flat.mul_(1.0 / self.world)
        return flat

    def any(self, flag: torch.Tensor) -> torch.Tensor:
        """Logical OR over ranks of a 0/1 device scalar (the agreed NaN-skip)."""
        if self.on:
            self._quiescent()
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        return flag

    def mean_scalar(self, t: torch.Tensor) -> torch.Tensor:
        if not self.on:
            return t
        self._quiescent()
        t = t.clone()
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t / self.world

    def max_scalar(self, t: torch.Tensor) -> torch.Tensor:
        """MAX over ranks (wall clocks of a timed region: bench.py's ddp_train leg)."""
        if not self.on:
            return t
        self._quiescent()
        t = t.clone()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t

    def gather_objects(self, obj) -> list:
        """Every rank's (picklable) record on every rank, in rank order: per-rank timelines of the bench's ddp_train leg."""
        if not self.on:
            return [obj]
        self._quiescent()
        out = [None] * self.world
        dist.all_gather_object(out, obj)
        return out

    def barrier(self) -> None:
        if self.on:
            self._quiescent()
            dist.barrier()


@torch.no_grad()
def compute_scale_factor(autoencoder, labels: torch.Tensor, sync: Optional[GradSync] = None) -> torch.Tensor:
    """1 / std of the label latents of the first batch, averaged over ranks (train_diffusion.py:100-124)."""
    z = autoencoder.encode_stage_2_inputs(labels)
    sf = 1.0 / torch.std(z)
    return (sync or GradSync()).mean_scalar(sf)


class DiffusionTrainer:
    def __init__(self, unet, autoencoder, inferer, lr: float, max_grad_norm: float = 1.0, milestones=(100, 1000),
                 gamma: float = 0.1, reference_rng_order: bool = False, grad_dtype: torch.dtype = torch.float32,
                 ema_decay: Optional[float] = None, ema_warmup: bool = True, cond_drop_prob: float = 0.0,
                 cfg_fill_value: float = -1.0, loss_weighting: str = "none", snr_gamma: float = 5.0,
                 loss_weights: Optional[torch.Tensor] = None, timestep_sampling: str = "uniform", timestep_bins: int = 20,
                 grad_accum_steps: int = 1):
        """``ema_decay`` (opt-in; the reference has no EMA): the optimizer keeps an exponential moving average of the weights inside its
        Adam launch (``FlatAdam.ema_params``).  Every rank computes the same EMA from the same parameters and the same averaged
        gradients: no communication.

        ``cond_drop_prob`` (opt-in; training for classifier-free guidance): each training sample's condition is replaced by a tensor
        filled with ``cfg_fill_value`` with that probability (``ldm_cond_dropout``) before the UNet sees it.  The decisions are keyed by
        ``(cache_seed, cached_steps)`` and the dataset indices on the cached path, by ``(cache_seed, timestep_draws)`` and
        ``rank * B + slot`` on the uncached one (ranks do not drop in lockstep); both counters are in the resume state.  Validation
        never drops.

        ``loss_weighting="min_snr"`` (opt-in; ``snr_gamma``) weights each sample's loss by the Min-SNR-gamma weight of its timestep
        (``loss_weighting.min_snr_weights`` for the scheduler's prediction type); ``loss_weights`` is a user table ``[T]`` in its place
        (the two exclude each other).  ``timestep_sampling="loss_aware"`` (opt-in; ``timestep_bins``) draws the timesteps from
        ``loss_weighting.LossTracker`` and multiplies each sample's loss by its importance weight, keyed as condition dropout keys its
        decisions.  With any of them on, the loss is ``loss_weighting.weighted_mse_loss`` (two launches, like ``mse_loss``), the tracker
        (``self.tracker``) is updated by it, and ``last_unweighted_loss`` holds the plain mean beside the returned loss.  With all at
        their defaults nothing of this is built or called.  Validation stays uniform and unweighted.  Trackers are per rank.  A
        rectified-flow scheduler takes neither option (``NotImplementedError``).

        ``grad_accum_steps=K`` (opt-in; the reference's multi-GPU notes recommend it, its trainer never had it): ``train_step`` /
        ``train_step_cached`` each process ONE micro-batch and every K-th call closes a window with one optimizer step on the mean of the
        window's K gradients, which the backward plan accumulates bucket by bucket (``FlatAdam(grad_accum_steps=K)``).  Calls that do not
        close the window run no exchange (neither the overlapped one nor ``sync.mean_``) and no ``optimizer.step()``, return a device
        ``False`` as ``skipped`` and leave parameters, moments and EMA untouched; the closing call exchanges the accumulated gradient (with
        overlap: inside its backward), applies clip, NaN-skip, Adam, EMA and re-pack from it and reports that step's ``skipped``.
        ``stepped`` (host bool, no device read) says which kind the last call was; ``window_loss`` (device scalar, valid when ``stepped``)
        is the mean of the window's micro losses.  The timestep draw counter, the cached-step counter, condition dropout and the loss
        tracker move on per micro-batch; the skip counter and EMA per optimizer step.  A NaN gradient in any micro-batch makes the
        accumulated norm non-finite: the device-side NaN-skip drops the whole window, and the next window's first micro-batch assigns, so
        nothing has to be cleared.  A window is not tied to an epoch (``end_epoch`` leaves a partial one open).  Every micro-batch of a
        window must have the same batch size (the scale is 1/K).  With K == 1 nothing of this is built."""
        if not 0.0 <= float(cond_drop_prob) <= 1.0:
            raise ValueError(f"cond_drop_prob must lie in [0, 1], got {cond_drop_prob}")
        from .loss_weighting import LOSS_WEIGHTINGS, TIMESTEP_SAMPLINGS
        if loss_weighting not in LOSS_WEIGHTINGS:
            raise ValueError(f"loss_weighting given as {loss_weighting!r} must be one of {list(LOSS_WEIGHTINGS)}")
        if timestep_sampling not in TIMESTEP_SAMPLINGS:
            raise ValueError(f"timestep_sampling given as {timestep_sampling!r} must be one of {list(TIMESTEP_SAMPLINGS)}")
        if loss_weights is not None and loss_weighting != "none":
            raise ValueError("loss_weights (a user table) and loss_weighting='min_snr' exclude each other")
        self.loss_weighting, self.timestep_sampling, self.snr_gamma = loss_weighting, timestep_sampling, float(snr_gamma)
        self.tracker, self.loss_table, self.last_unweighted_loss = None, None, None
        self._iw = None                                  # importance weights of the timesteps _timesteps drew last (loss-aware draw)
        if loss_weighting != "none" or loss_weights is not None or timestep_sampling != "uniform":
            from .loss_weighting import LossTracker, min_snr_weights
            sch = inferer.scheduler
            if not hasattr(sch, "alphas_cumprod"):
                raise NotImplementedError(f"loss weighting / loss-aware timestep sampling are not built for {type(sch).__name__}")
            table = None
            if loss_weighting == "min_snr":
                table = min_snr_weights(sch, snr_gamma)
            elif loss_weights is not None:
                table = loss_weights.detach().to(dtype=torch.float32).reshape(-1)
                if table.numel() != sch.num_train_timesteps:
                    raise ValueError(f"loss_weights has {table.numel()} entries, the scheduler {sch.num_train_timesteps} timesteps")
            tracker = LossTracker(sch.num_train_timesteps, n_bins=timestep_bins)
            dev = unet.flat_params.device if getattr(unet, "flat_params", None) is not None else next(unet.parameters()).device
            self.loss_table = None if table is None else table.to(dev).contiguous()
            self.tracker = tracker.to(dev)
        self.cond_drop_prob, self.cfg_fill_value = float(cond_drop_prob), float(cfg_fill_value)
        from .optim import FlatAdam
        self.unet, self.autoencoder, self.inferer = unet, autoencoder, inferer
        self.sync = GradSync(grad_dtype=grad_dtype)
        self.optimizer = FlatAdam(unet, lr=lr, max_grad_norm=max_grad_norm, ema_decay=ema_decay, ema_warmup=ema_warmup,
                                  grad_accum_steps=grad_accum_steps)   # flattens the parameters
        self.grad_accum_steps = self.optimizer.grad_accum_steps
        self.stepped = True                              # the last train_step* call ended in an optimizer step (host bool)
        self.window_loss = None                          # device scalar: mean of the micro losses of the window that call closed
        self._window_sum = None
        self._false = torch.zeros((), dtype=torch.bool, device=unet.flat_params.device)
        self.sync.broadcast(unet.flat_params, 0)
        unet.mark_weights_dirty()
        # RCCL through the library's C ABI, bucketed and overlapped with backward ("nccl" backend); else one all-reduce after it
        self.overlap = self.sync.attach(unet)
        self.lr_scheduler = torch.optim.lr_scheduler.MultiStepLR(self.optimizer, milestones=list(milestones), gamma=gamma)
        self.reference_rng_order = reference_rng_order
        self.factor = getattr(autoencoder, "factor", 4)
        # latent-cache steps (train_step_cached / validate_cached): the key of the kernel's draws and the two step counts behind it
        self.cache_seed, self.cached_steps, self.cached_val_steps = 0, 0, 0
        self.timestep_draws = 0                          # uncached steps whose timesteps the scheduler drew (the step word of its key)

    def _timesteps(self, like: torch.Tensor, B: int, idx=None, seed: int = 0, step: int = 0) -> torch.Tensor:
        """Training timesteps [B] on ``like``'s device: the scheduler's own draw where it has one (RFlowScheduler.sample_timesteps: one
        launch, keyed by ``(seed, step)`` and the dataset indices ``idx`` or the batch slots), else the reference's device randint."""
        sch = self.inferer.scheduler
        if hasattr(sch, "sample_timesteps"):
            return sch.sample_timesteps(like, idx=idx, seed=seed, step=step)
        if self.timestep_sampling == "loss_aware" and self.unet.training:   # validation stays uniform
            timesteps, self._iw = self.tracker.sample(B, like, idx=idx, seed=seed, step=step)
            return timesteps
        return torch.randint(0, sch.num_train_timesteps, (B,), device=like.device).long()

    def _draw(self, labels: torch.Tensor, want_timesteps: bool = True):
        """-> (noise, timesteps) of one step.  ``want_timesteps=False`` (the caller brought its own): under the loss-aware draw nothing
        is launched, no importance weights are left behind and ``timesteps`` is None; the step word still moves on."""
        B = labels.shape[0]
        lat = [s // self.factor for s in labels.shape[2:]]
        if self.reference_rng_order:
            with torch.no_grad():
                lat = list(self.autoencoder.encode_stage_2_inputs(labels).shape[2:])
        noise = torch.randn((B, self.autoencoder.latent_channels, *lat), dtype=torch.float32).to(labels.device)
        idx = None
        if self.timestep_sampling == "loss_aware":        # ranks do not draw in lockstep: the key of condition dropout
            rank = dist.get_rank() if self.sync.on else 0
            idx = [rank * B + b for b in range(B)]
        if self.timestep_sampling == "loss_aware" and not want_timesteps:
            timesteps = None
        else:
            timesteps = self._timesteps(noise, B, idx=idx, seed=self.cache_seed, step=self.timestep_draws)
        self.timestep_draws += 1
        return noise, timesteps

    def _loss(self, pred: torch.Tensor, target: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        """The training loss of one step: ``mse_loss`` with every option at its default; otherwise the weighted loss with the table, the
        importance weights of the draw (none for explicit timesteps: 1) and the tracker update, all inside its two launches."""
        if self.tracker is None:
            return mse_loss(pred, target)
        from .loss_weighting import weighted_mse_loss
        loss, self.last_unweighted_loss = weighted_mse_loss(pred, target, timesteps, w_table=self.loss_table, sample_w=self._iw,
                                                            tracker=self.tracker)
        return loss

    def _drop(self, cond: torch.Tensor, idx, step: int) -> torch.Tensor:
        """Condition dropout of a training batch, in place on the fresh condition tensor (no launch when nothing drops)."""
        from .latents import cond_dropout
        cond = cond.detach().to(torch.float32).contiguous()
        cond_dropout(cond, self.cond_drop_prob, self.cfg_fill_value, idx=idx, seed=self.cache_seed, step=step)
        return cond

    def _predict(self, images, labels, noise, timesteps, drop_step: Optional[int] = None):
        """-> (prediction, target): the target of the scheduler's prediction_type (``noise`` itself for epsilon).  ``drop_step``
        (training steps with ``cond_drop_prob`` > 0): the step word of the condition-dropout key."""
        with torch.no_grad():
            image_latents = self.autoencoder.encode_stage_2_inputs(images)
            if drop_step is not None and self.cond_drop_prob > 0.0:
                B = image_latents.shape[0]
                rank = dist.get_rank() if self.sync.on else 0
                image_latents = self._drop(image_latents, [rank * B + b for b in range(B)], drop_step)
        return self.inferer(inputs=labels, autoencoder_model=self.autoencoder, diffusion_model=self.unet, noise=noise,
                            timesteps=timesteps, condition=image_latents, mode="concat", return_target=True)

    def train_step(self, images: torch.Tensor, labels: torch.Tensor, noise: Optional[torch.Tensor] = None,
                   timesteps: Optional[torch.Tensor] = None):
        """One optimizer step (one micro-batch of it with ``grad_accum_steps`` > 1: see ``__init__``).  Returns (loss [device scalar],
        skipped [0-dim device bool tensor: truthy if this step was a NaN-skip]).
        Nothing in here reads a device value on the host: ranks never wait for each other's host, only for the gradient exchange."""
        self.unet.train()
        images, labels = images.float(), labels.float()
        self.optimizer.zero_grad(set_to_none=True)
        self._iw = None
        drop_step = self.timestep_draws                   # the step word _draw keys this step's timesteps with
        if noise is None or timesteps is None:
            n2, t2 = self._draw(labels, want_timesteps=timesteps is None)
            noise = n2 if noise is None else noise
            timesteps = t2 if timesteps is None else timesteps
        elif self.cond_drop_prob > 0.0:
            self.timestep_draws += 1                      # explicit draws: the dropout key still moves on with every step
        noise_pred, target = self._predict(images, labels, noise, timesteps, drop_step=drop_step)
        loss = self._loss(noise_pred, target, timesteps)  # F.mse_loss (:207) + its gradient in two HIP launches
        return self._backward_and_step(loss)

    def _backward_and_step(self, loss: torch.Tensor):
        """backward, and on the call that closes the accumulation window (every call with ``grad_accum_steps`` == 1) the exchange and the
        optimizer step.  -> (loss, skipped)."""
        opt = self.optimizer
        before = opt.skipped_steps().clone()
        opt.arm()                                        # K > 1: this backward is micro-batch opt.micro of the window
        loss.backward()                                  # with self.overlap the buckets are reduced inside this call (K > 1: the closing one)
        ld = loss.detach()
        if self.grad_accum_steps > 1:
            self._window_sum = ld if opt.micro == 0 else self._window_sum + ld
        self.stepped = opt.micro_done()
        if not self.stepped:
            return ld, self._false
        self.window_loss = ld if self.grad_accum_steps == 1 else self._window_sum / self.grad_accum_steps
        if not self.overlap:
            self.sync.mean_(opt.grads)
        opt.step()                                       # a NaN / inf gradient norm (on any rank, after the mean) skips the update on the device
        return ld, opt.skipped_steps() > before

    def _predict_cached(self, cache, idx, timesteps, eps_label, eps_image, noise, seed: int, step: int, drop: bool = False):
        """``_predict`` from a ``latents.LatentCache``: one launch (``ldm_latent_batch``) writes the noisy label latents, the image latents
        and the target of the samples ``idx``, then the UNet; no autoencoder call, nothing from the host."""
        sch = self.inferer.scheduler
        if timesteps is None:
            timesteps = self._timesteps(cache.mu_label[0:1].expand(len(idx), *cache.latent_shape), len(idx), idx=idx, seed=seed, step=step)
        noisy, cond, target = cache.batch(idx, sch, timesteps, self.inferer.scale_factor, eps_label=eps_label, eps_image=eps_image,
                                          noise=noise, seed=seed, step=step)
        if drop and self.cond_drop_prob > 0.0:              # after ldm_latent_batch*, same (seed, step) and dataset indices, a stream of its own
            cond = self._drop(cond, cache.check_idx(idx), step)
        return self.unet(x=noisy, timesteps=timesteps, context=None, cond=cond), target

    def train_step_cached(self, cache, idx, noise: Optional[torch.Tensor] = None, timesteps: Optional[torch.Tensor] = None,
                          eps_label: Optional[torch.Tensor] = None, eps_image: Optional[torch.Tensor] = None):
        """``train_step`` for the samples ``idx`` of a ``latents.LatentCache`` instead of a batch of volumes: from the prediction on the
        same step and the same ``(loss, skipped)``.  The autoencoder's draws and the noise are ``eps_label``, ``eps_image`` and ``noise``
        if all three are given; otherwise the kernel draws them from ``(cache_seed, cached_steps)`` and the dataset indices, and
        ``cached_steps`` counts on.  The timesteps come from the same device ``torch.randint`` as in ``train_step``, or from the scheduler's
        own draw under the same key (``_timesteps``)."""
        self.unet.train()
        self.optimizer.zero_grad(set_to_none=True)
        self._iw = None
        if timesteps is None and self.tracker is not None:   # the loss needs them: drawn here as _predict_cached would draw them
            timesteps = self._timesteps(cache.mu_label[0:1].expand(len(idx), *cache.latent_shape), len(idx), idx=idx, seed=self.cache_seed,
                                        step=self.cached_steps)
        noise_pred, target = self._predict_cached(cache, idx, timesteps, eps_label, eps_image, noise, self.cache_seed, self.cached_steps,
                                                  drop=True)
        self.cached_steps += 1
        loss = self._loss(noise_pred, target, timesteps)
        return self._backward_and_step(loss)

    def end_epoch(self):
        """The lr schedule is stepped per epoch, as the reference does; an accumulation window left open here is completed by the next
        epoch's first calls."""
        self.lr_scheduler.step()

    def objective_state_dict(self) -> dict:
        """What a resumed run needs beside the optimizer's and the lr schedule's state to continue the same draws: the step word of the
        uncached key and, with a tracker, its state."""
        sd = {"timestep_draws": int(self.timestep_draws)}
        if self.tracker is not None:
            sd["loss_tracker"] = self.tracker.state_dict()
        return sd

    def load_objective_state_dict(self, sd: dict, default_draws: int = 0) -> None:
        """The inverse; a state without the keys (written before they existed, or by a run without a tracker) leaves the tracker empty
        and starts the counter at ``default_draws``."""
        self.timestep_draws = int(sd.get("timestep_draws", default_draws))
        if self.tracker is not None and sd.get("loss_tracker") is not None:
            self.tracker.load_state_dict(sd["loss_tracker"])

    @torch.no_grad()
    def validate(self, loader, device, use_ema: bool = False) -> float:
        """Mean training-style loss over the loader, NaN batches skipped, averaged over ranks (:231-283).  ``use_ema``: computed
        with the optimizer's EMA weights (``FlatAdam.ema_weights``); the live weights are back afterwards."""
        self.unet.eval()
        if use_ema:
            with self.optimizer.ema_weights():
                return self._validate(loader, device)
        return self._validate(loader, device)

    def _validate(self, loader, device) -> float:
        total, n = torch.zeros((), device=device), 0
        for batch in loader:
            images, labels = batch["image"].to(device).float(), batch["label"].to(device).float()
            noise, timesteps = self._draw(labels)
            pred, target = self._predict(images, labels, noise, timesteps)
            v = F.mse_loss(pred.float(), target.float())
            if not bool(torch.isnan(v)):
                total += v
                n += 1
        val = total / n if n else torch.tensor(float("inf"), device=device)
        return float(self.sync.mean_scalar(val))

    @torch.no_grad()
    def validate_cached(self, cache, batches, use_ema: bool = False) -> float:
        """``validate`` over a ``latents.LatentCache``: ``batches`` yields lists of dataset indices (a loader's ``batch_sampler``).  The
        draws are the kernel's, keyed by ``cache_seed + 1`` and a count of validation batches of its own."""
        self.unet.eval()
        if use_ema:
            with self.optimizer.ema_weights():
                return self._validate_cached(cache, batches)
        return self._validate_cached(cache, batches)

    def _validate_cached(self, cache, batches) -> float:
        device = cache.device
        total, n = torch.zeros((), device=device), 0
        for idx in batches:
            pred, target = self._predict_cached(cache, idx, None, None, None, None, self.cache_seed + 1, self.cached_val_steps)
            self.cached_val_steps += 1
            v = F.mse_loss(pred.float(), target.float())
            if not bool(torch.isnan(v)):
                total += v
                n += 1
        val = total / n if n else torch.tensor(float("inf"), device=device)
        return float(self.sync.mean_scalar(val))


# ------------------------------------------------------------------------------------------------ stage 1: AutoencoderKL
class _GateGrad(torch.autograd.Function):
    """Identity whose backward passes the incoming gradient only where ``ok`` (a 0-dim device bool, filled in AFTER the branch behind
    this node has run forward) is true and zeros otherwise.  Selection, not multiplication: a NaN gradient coming back from a
    non-finite adversarial branch is replaced, not scaled (0 * NaN = NaN), so the branch is really dropped (train_autoencoder.py:417-422)."""

    @staticmethod
    def forward(ctx, x, ok):
        ctx.ok = ok
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return torch.where(ctx.ok, g, torch.zeros_like(g)), None


def kl_loss(z_mu: torch.Tensor, z_sigma: torch.Tensor) -> torch.Tensor:
    """The reference's KL term (3d_ldm/utils.py:249-262): 0.5 * sum(mu^2 + s^2 - log(s^2 + eps) - 1) over all but the batch
    dimension with s = clamp(sigma, min=1e-8), divided by the batch size, clamped to [0, 1000]."""
    eps = 1e-8
    s = torch.clamp(z_sigma, min=eps)
    kl = 0.5 * torch.sum(z_mu.pow(2) + s.pow(2) - torch.log(s.pow(2) + eps) - 1, dim=list(range(1, z_sigma.dim())))
    return torch.clamp(kl / kl.shape[0], 0.0, 1000.0)


class AutoencoderTrainer:
    """The stage-1 (VAE-GAN) training step (3d_ldm/train_autoencoder.py:352-494) on the HIP forward / backward plans:
    clamp the images to [0, 1] (:362), ``reconstruction, z_mu, z_sigma = autoencoder(images)`` (:366), reconstruction L1 / L2
    (:226-233,374), KL (:375,386) * kl_weight, and after ``warm_up_epochs`` (:304,409) the LSGAN generator term
    ``adv_weight * mse(D(reconstruction)[-1], 1)`` (:410-424); NaN-skip agreed over ranks, ``loss_g.backward()``,
    ``clip_grad_norm_(0.5)`` and AdamW(betas (0.5, 0.9), weight_decay 1e-5) (:274-279,440-451), lr scaled by sqrt(world) * 0.5
    under DDP (:246-259); then the discriminator step ``adv_weight * 0.5 * (mse(D(recon.detach())[-1], 0) + mse(D(images)[-1], 1))``
    with its own clip 0.5 + AdamW (:454-494).  The PatchDiscriminator runs on the same HIP kernels (``ldm3d.discriminator``).

    Not reproduced: the perceptual term needs a downloaded SqueezeNet (no network here): a non-zero ``perceptual_weight`` is
    reported once and the term is left out."""

    def __init__(self, autoencoder, lr: float, kl_weight: float, recon_loss: str = "l1", perceptual_weight: float = 0.0,
                 max_grad_norm: float = 0.5, weight_decay: float = 1e-5, warm_up_epochs: int = 5, adv_weight: float = 0.01,
                 discriminator=None, perceptual_weights: Optional[str] = None):
        from .discriminator import PatchAdversarialLoss, PatchDiscriminator
        from .optim import FlatAdam, FlatModuleAdam
        # the perceptual term (:236,386,406) needs LPIPS / SqueezeNet weights: from a user-supplied file, else dropped and recorded
        self.perceptual_weight, self.loss_perceptual = float(perceptual_weight or 0.0), None
        if perceptual_weight and perceptual_weights:
            from .perceptual import PerceptualLoss
            self.loss_perceptual = PerceptualLoss.from_file(perceptual_weights).to(autoencoder.flat_params.device
                                                                                  if getattr(autoencoder, "flat_params", None) is not None
                                                                                  else next(autoencoder.parameters()).device)
        self.perceptual_dropped = bool(perceptual_weight) and self.loss_perceptual is None   # logged by train_autoencoder.py
        if self.perceptual_dropped:
            # the reference's PerceptualLoss downloads a pretrained SqueezeNet (train_autoencoder.py:236): no weights, no network here.
            # Every shipped config sets a (small: 1e-5 .. 1e-3) weight, so warn once and train without the term instead of refusing.
            import warnings
            warnings.warn(f"autoencoder_train.perceptual_weight = {perceptual_weight}: the perceptual term needs pretrained SqueezeNet "
                          "weights that are not available offline; training continues WITHOUT it (reconstruction + KL + adversarial)")
        self.autoencoder = autoencoder
        self.sync = GradSync()
        world = self.sync.world
        lr = lr * (world ** 0.5 * 0.5 if world > 1 else 1.0)
        self.optimizer = FlatAdam(autoencoder, lr=lr, betas=(0.5, 0.9), eps=1e-8, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        self.sync.broadcast(autoencoder.flat_params, 0)
        autoencoder.mark_weights_dirty()
        self.overlap = self.sync.attach(autoencoder)
        self.kl_weight, self.l2 = kl_weight, recon_loss == "l2"
        self.warm_up_epochs, self.adv_weight = warm_up_epochs, adv_weight
        # the reference hard-codes in_channels=1 (:155); the image channel count of the autoencoder keeps 2-channel configs working
        dev = autoencoder.flat_params.device
        self.discriminator = discriminator if discriminator is not None else PatchDiscriminator(
            spatial_dims=3, num_layers_d=3, channels=32, in_channels=autoencoder.out_channels, out_channels=1, norm="INSTANCE")
        self.discriminator = self.discriminator.to(dev)
        self.adv_loss = PatchAdversarialLoss(criterion="least_squares")
        self.optimizer_d = FlatModuleAdam(self.discriminator, lr=lr, betas=(0.5, 0.9), eps=1e-8, weight_decay=weight_decay,
                                          max_grad_norm=max_grad_norm)
        self.sync.broadcast(self.optimizer_d.flat_params, 0)

    def intensity_loss(self, a, b):
        return F.mse_loss(a, b) if self.l2 else F.l1_loss(a, b)

    def train_step(self, images: torch.Tensor, epoch: int = 0, eps: Optional[torch.Tensor] = None):
        """-> (dict of detached scalar losses, skipped)."""
        self.autoencoder.train()
        images = torch.clamp(images.float(), 0.0, 1.0)
        # No host read of a device value in this step: non-finite inputs or losses (:362-365,426-437,470-484 `continue`) make the
        # gradient norm non-finite, the data-parallel mean carries that to every rank, and the fused clip + AdamW launches then leave
        # parameters and moments untouched (optim.FlatAdam.skipped_steps).  A non-finite adversarial term ALONE is dropped and the
        # step continues on reconstruction + KL (:417-422): its value is selected away in the forward and its gradient is selected
        # away where the branch leaves the reconstruction (_GateGrad), so no 0 * NaN reaches the autoencoder.  A skipped generator
        # step also skips the discriminator step of that batch (the reference `continue`s before it).
        adversarial = epoch > self.warm_up_epochs
        reconstruction, z_mu, z_sigma = self.autoencoder(images, eps=eps)
        recons = self.intensity_loss(reconstruction, images)
        kl = kl_loss(z_mu, z_sigma).mean()
        loss_g = recons + self.kl_weight * kl
        out = {"recons": recons.detach(), "kl": kl.detach()}
        if self.loss_perceptual is not None:                                       # :386,406
            p_loss = self.loss_perceptual(reconstruction.float(), images.float())
            loss_g = loss_g + self.perceptual_weight * p_loss
            out["perceptual"] = p_loss.detach()
        if adversarial:
            ok = torch.ones((), dtype=torch.bool, device=reconstruction.device)      # filled in below, read by _GateGrad.backward
            logits_fake = self.discriminator(_GateGrad.apply(reconstruction.contiguous().float(), ok))[-1]
            generator_loss = self.adv_loss(logits_fake, target_is_real=True, for_discriminator=False)
            ok.copy_(torch.isfinite(generator_loss.detach()))
            loss_g = loss_g + self.adv_weight * torch.where(ok, generator_loss, torch.zeros_like(generator_loss))
            out["adv_g"] = generator_loss.detach()
        before = self.optimizer.skipped_steps().clone()
        loss_g.backward()
        if not self.overlap:
            self.sync.mean_(self.autoencoder.flat_grads)
        self.optimizer.step()
        out["loss_g"] = loss_g.detach()
        skipped_g = self.optimizer.skipped_steps() > before
        if adversarial:
            # discriminator step (:454-494): fake = the detached reconstruction, real = the images
            self.optimizer_d.zero_grad()
            logits_fake = self.discriminator(reconstruction.contiguous().detach())[-1]
            loss_d_fake = self.adv_loss(logits_fake, target_is_real=False, for_discriminator=True)
            logits_real = self.discriminator(images.contiguous().detach())[-1]
            loss_d_real = self.adv_loss(logits_real, target_is_real=True, for_discriminator=True)
            discriminator_loss = (loss_d_fake + loss_d_real) * 0.5
            loss_d = self.adv_weight * discriminator_loss
            # a batch whose generator step was skipped gets no discriminator step either: a NaN factor makes every discriminator
            # gradient NaN and FlatModuleAdam skips itself on the device (still no host read)
            loss_d = loss_d * torch.where(skipped_g, torch.full_like(loss_d, float("nan")), torch.ones_like(loss_d))
            loss_d.backward()
            self.sync.mean_(self.optimizer_d.flat_grads)
            self.optimizer_d.step()                          # skips itself on a non-finite gradient norm
            out["adv_d"] = discriminator_loss.detach()
        return out, skipped_g

    @torch.no_grad()
    def validate(self, loader, device) -> float:
        """Mean clamped-reconstruction loss (:565-611), averaged over ranks."""
        self.autoencoder.eval()
        total, n = torch.zeros((), device=device), 0
        for batch in loader:
            images = torch.clamp(batch["image"].to(device).float(), 0.0, 1.0)
            reconstruction, _, _ = self.autoencoder(images)
            v = self.intensity_loss(torch.clamp(reconstruction, 0.0, 1.0), images)
            if bool(torch.isfinite(v)):
                total += v
                n += 1
        val = total / n if n else torch.tensor(float("inf"), device=device)
        return float(self.sync.mean_scalar(val))

    @torch.no_grad()
    def validate_metrics(self, loader, device) -> Dict[str, float]:
        """PSNR / SSIM of the clamped reconstructions against the clamped inputs (ldm3d.metrics, data_range 1), averaged over the
        volumes of the loader and over ranks.  Beside ``validate`` and without touching what it returns; the sums stay on the device
        and are read once."""
        from .metrics import image_metrics
        self.autoencoder.eval()
        sums, n = torch.zeros(2, device=device), 0
        for batch in loader:
            images = torch.clamp(batch["image"].to(device).float(), 0.0, 1.0)
            reconstruction, _, _ = self.autoencoder(images)
            m = image_metrics(torch.clamp(reconstruction.float(), 0.0, 1.0), images, data_range=1.0)
            sums += torch.stack([m["psnr"].sum(), m["ssim"].sum()])
            n += images.shape[0]
        vals = self.sync.mean_scalar(sums / max(n, 1)).cpu().tolist()
        return {"psnr": float(vals[0]), "ssim": float(vals[1])}
