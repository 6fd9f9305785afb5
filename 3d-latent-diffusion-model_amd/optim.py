"""Optimizer tail of the diffusion trainer on flat buffers.

The reference does (3d_ldm/train_diffusion.py:155-156, 214-223)::

    optimizer = torch.optim.Adam(params=unet.parameters(), lr=args.diffusion_train["lr"])
    lr_scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[100, 1000], gamma=0.1)
    loss.backward(); torch.nn.utils.clip_grad_norm_(unet.parameters(), 1.0); optimizer.step()

``FlatAdam`` is a ``torch.optim.Optimizer`` (so ``MultiStepLR`` and ``zero_grad`` keep working) whose single parameter
is the module's flat fp32 buffer (``module.flatten_parameters()``): gradient clipping + Adam are two HIP launches over
191 M elements instead of ~320 per-tensor kernel groups, and the data-parallel mean is one all-reduce of
``module.flat_grads``.  Same arithmetic as ``torch.optim.Adam`` (defaults betas (0.9, 0.999), eps 1e-8, no amsgrad) and,
with ``weight_decay > 0``, as the decoupled ``torch.optim.AdamW`` of the stage-1 trainer
(3d_ldm/train_autoencoder.py:274-279: betas (0.5, 0.9), weight_decay 1e-5), and as ``clip_grad_norm_`` (scale = max_norm /
(norm + 1e-6), clamped to 1).
"""
from __future__ import annotations

import torch

from . import _lib


class _MseLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        p = pred.detach().to(torch.float32).contiguous()
        t = target.detach().to(device=p.device, dtype=torch.float32).contiguous()
        if not p.is_cuda:
            raise _lib.LdmError("mse_loss: CUDA tensors only (no CPU fallback)")
        if p.shape != t.shape:
            raise ValueError(f"mse_loss: shapes differ: {tuple(p.shape)} vs {tuple(t.shape)}")
        loss = torch.empty((1,), dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p)
        with torch.cuda.device(p.device):
            _lib.check(_lib.lib().ldm_op_mse_loss(p.data_ptr(), t.data_ptr(), p.numel(), loss.data_ptr(), grad.data_ptr(), _lib.current_stream()))
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None


def mse_loss(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """``F.mse_loss(pred, target)`` (mean reduction; 3d_ldm/train_diffusion.py:207) in two HIP launches that also leave the gradient
    ``2 (pred - target) / n`` for ``backward`` (instead of ~6 element-wise / reduction kernels of the tensor library between the
    forward and the backward launch plan).  Differentiable w.r.t. ``pred`` only."""
    return _MseLossFn.apply(pred, target)


class FlatAdam(torch.optim.Optimizer):
    """``ema_decay`` (opt-in) keeps an exponential moving average of the parameters in ``ema_params``, updated by the Adam launch
    itself (``ldm_adam_step_ema`` / ``ldm_model_adam_step_ema``): the NaN-skip is decided on the device, so only the kernel knows
    whether a step was applied and how many were applied before it (the warm-up ``min(decay, (1 + a) / (10 + a))`` counts applied
    steps).  ``ema_params`` is ``None`` until the first ``step()``, which starts it as a copy of the parameters as they stand then
    (after a broadcast / checkpoint load that followed construction), unless ``load_state_dict`` supplied one.

    ``grad_accum_steps=K`` (opt-in, K > 1): one ``step()`` per K backwards.  The caller calls ``arm()`` before each backward; the backward
    plan then folds that micro-batch's gradient, scaled by 1/K, into ``grad_accum`` (one more fp32 buffer of the parameter count, allocated
    at the first ``arm()``) bucket by bucket (``module.set_grad_accum``), ``micro_done()`` says whether the window is complete, and
    ``grad_norm()`` / ``step()`` read ``grads`` = ``grad_accum``.  The first micro-batch of a window assigns, so nothing is ever zeroed and a
    window dropped by the NaN-skip leaves nothing behind.  With K == 1 nothing is allocated or armed."""

    def __init__(self, module, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: float | None = None,
                 weight_decay: float = 0.0, ema_decay: float | None = None, ema_warmup: bool = True, grad_accum_steps: int = 1):
        if isinstance(grad_accum_steps, bool) or not isinstance(grad_accum_steps, int) or grad_accum_steps < 1:
            raise ValueError(f"grad_accum_steps must be an integer >= 1, got {grad_accum_steps!r}")
        if getattr(module, "flat_params", None) is None:
            module.flatten_parameters()
        self.module = module
        flat = module.flat_params
        if not flat.is_cuda:
            raise _lib.LdmError("FlatAdam needs the module on the GPU (no CPU fallback)")
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay!r}")
        self._flat = torch.nn.Parameter(flat, requires_grad=False)      # shares storage with module.flat_params
        super().__init__([self._flat], dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.max_grad_norm = max_grad_norm
        self.fuse_repack = True                        # Adam + bf16 re-pack in one kernel (ldm_model_adam_step)
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        # {sum g^2 of the current gradients, optimizer steps skipped on the device because that sum was not finite}: include/ldm3d.h
        self.sq_norm = torch.zeros((2,), dtype=torch.float32, device=flat.device)
        self.steps = 0
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.ema_params = None                         # flat fp32, layout of flat_params; allocated by the first step() (EMA on only)
        self._in_ema = False
        self.grad_accum_steps = grad_accum_steps
        self.grad_accum = None                         # flat fp32, layout of flat_grads; allocated by the first arm() (K > 1 only)
        self.micro = 0                                 # micro-batches of the open window whose backward has been armed: 0 .. K - 1
        self._armed = False

    def zero_grad(self, set_to_none: bool = True):     # every backward overwrites flat_grads and a window's first one assigns grad_accum
        pass

    # -- gradient accumulation (grad_accum_steps > 1) -----------------------------------------------------------------------------
    @property
    def grads(self) -> torch.Tensor:
        """The gradient ``grad_norm()`` and ``step()`` read: the accumulator with ``grad_accum_steps`` > 1, else ``module.flat_grads``."""
        if self.grad_accum_steps > 1:
            if self.grad_accum is None:
                raise RuntimeError("FlatAdam(grad_accum_steps > 1): no backward has been armed yet (call arm() before each backward)")
            return self.grad_accum
        return self.module.flat_grads

    def arm(self) -> None:
        """Before each backward: tells the module which micro-batch of the window this backward is.  K == 1: nothing."""
        if self.grad_accum_steps == 1:
            return
        if self._armed:
            raise RuntimeError("FlatAdam.arm() twice without micro_done() in between")
        if self.grad_accum is None:
            self.grad_accum = torch.empty_like(self.module.flat_grads)
        self.module.set_grad_accum(self.grad_accum, self.micro, self.grad_accum_steps)
        self._armed = True

    def micro_done(self) -> bool:
        """After each backward: counts the micro-batch and disarms the module (validation and sampling never touch the accumulator).
        True when the window is complete: the exchange (if not overlapped) and ``step()`` follow, and the next ``arm()`` opens a new
        window.  K == 1: always True."""
        if self.grad_accum_steps == 1:
            return True
        if not self._armed:
            raise RuntimeError("FlatAdam.micro_done() without arm()")
        self._armed = False
        self.module.set_grad_accum(None)
        self.micro = (self.micro + 1) % self.grad_accum_steps
        return self.micro == 0

    def grad_norm(self) -> torch.Tensor:
        """Global L2 norm of the current gradients (device scalar), as clip_grad_norm_ returns it."""
        L = _lib.lib()
        g = self.grads
        with torch.cuda.device(g.device):
            _lib.check(L.ldm_grad_sq_norm(g.data_ptr(), g.numel(), self.sq_norm.data_ptr(), _lib.current_stream()))
        return self.sq_norm.sqrt()[0]

    def skipped_steps(self) -> torch.Tensor:
        """Device scalar: how many ``step()`` calls left the parameters untouched because the gradient norm was NaN / inf (the agreed
        NaN-skip of the trainers, decided on the device: no host read inside the step)."""
        return self.sq_norm[1]

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("closures are not used by the reference's trainers")
        if self._in_ema:
            raise RuntimeError("FlatAdam.step() inside ema_weights(): the module computes with the EMA weights there")
        if self._armed or self.micro != 0:
            raise RuntimeError(f"FlatAdam.step() inside an accumulation window ({self.micro} of {self.grad_accum_steps} micro-batches done)")
        L = _lib.lib()
        grp = self.param_groups[0]
        p, g = self.module.flat_params, self.grads
        clip = self.max_grad_norm is not None and self.max_grad_norm > 0
        ema = self.ema_decay is not None
        if ema and self.ema_params is None:
            self.ema_params = p.detach().clone()       # the parameters as the first step finds them
        self.steps += 1
        with torch.cuda.device(p.device):
            # the squared norm is taken whether or not clipping is on: the device-side NaN-skip reads it (max_norm <= 0 only disables
            # the clip factor inside the kernel; 3d_ldm/train_diffusion.py:210-212 skips a NaN batch regardless of clipping)
            _lib.check(L.ldm_grad_sq_norm(g.data_ptr(), g.numel(), self.sq_norm.data_ptr(), _lib.current_stream()))
            args = (float(grp["lr"]), float(grp["betas"][0]), float(grp["betas"][1]), float(grp["eps"]),
                    float(grp.get("weight_decay", 0.0)), self.steps) + ((self.ema_decay, int(self.ema_warmup)) if ema else ()) + (
                    self.sq_norm.data_ptr(), float(self.max_grad_norm or 0.0) if clip else 0.0, _lib.current_stream())
            bufs = (p.data_ptr(), g.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()) + ((self.ema_params.data_ptr(),) if ema else ())
            h = getattr(self.module, "_h", None)
            if self.fuse_repack and h is not None and not getattr(self.module, "_dirty", True):
                # one pass: Adam on the flat master weights + the bf16 re-pack of the library's arena from the new values
                _lib.check((L.ldm_model_adam_step_ema if ema else L.ldm_model_adam_step)(h, *bufs, *args))
                return None
            _lib.check((L.ldm_adam_step_ema if ema else L.ldm_adam_step)(*bufs, p.numel(), *args))
        self.module.mark_weights_dirty()               # the bf16 arena is re-packed before the next forward
        return None

    # -- the EMA weights ----------------------------------------------------------------------------------------------------------
    def _need_ema(self) -> torch.Tensor:
        if self.ema_decay is None:
            raise RuntimeError("this FlatAdam was built without ema_decay: there are no EMA weights")
        # before the first step the EMA is the parameters themselves
        return self.ema_params if self.ema_params is not None else self.module.flat_params

    def ema_state_dict(self) -> dict:
        """The EMA weights as an ordinary state dict (the module's own key names and shapes, fresh tensors): any network of the same
        definition loads it with ``load_state_dict``."""
        ema = self._need_ema()
        L, h = _lib.lib(), self.module._h
        out = {}
        for i, (name, q) in enumerate(self._named_params()):
            off = int(L.ldm_model_param_offset(h, i))
            out[name] = ema[off:off + q.numel()].view(q.shape).clone()
        return out

    def _named_params(self):
        """(state-dict key, parameter) in the library's order (the order of the flat buffers)."""
        L, h = _lib.lib(), self.module._h
        d = dict(self.module.named_parameters())
        names = [L.ldm_model_param_name(h, i).decode() for i in range(L.ldm_model_num_params(h))]
        return [(n, d[n]) for n in names]

    def ema_weights(self):
        """``with optimizer.ema_weights():`` the module computes with the EMA weights inside the block and with the live weights
        after it.  The fp32 masters are neither copied nor touched: the library's weight arena is loaded from the EMA buffer on entry
        (``ldm_model_load_params_flat``, which also invalidates everything derived from the weights: phase / im2col weights, the
        fp32 arena, the per-schedule time-embedding table; a replayed HIP graph reads the same addresses with the new contents) and
        re-packed from the live buffer on exit.  The module must be in eval mode; ``train()``, a grad-enabled forward and ``step()``
        raise inside the block, and ``state_dict()`` there still returns the live weights."""
        return _EmaWeights(self)

    # -- checkpointing ------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """Everything a resumed run needs: the moments, the step count, the device skip counter (bias corrections and EMA warm-up
        count step - skipped), the EMA with its decay and warm-up, and ``param_groups``.  ``torch.optim.Optimizer.state_dict``
        sees none of the flat buffers."""
        sd = {"exp_avg": self.exp_avg.detach().clone(), "exp_avg_sq": self.exp_avg_sq.detach().clone(), "steps": int(self.steps),
              "skipped": self.sq_norm[1:2].detach().clone(),
              "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}
        if self.ema_decay is not None:
            sd["ema"] = None if self.ema_params is None else self.ema_params.detach().clone()
            sd["ema_decay"], sd["ema_warmup"] = self.ema_decay, self.ema_warmup
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        has = "ema_decay" in sd
        if has and self.ema_decay is None:
            raise ValueError("the optimizer state carries EMA weights but this FlatAdam was built with EMA off (pass ema_decay)")
        if not has and self.ema_decay is not None:
            raise ValueError("this FlatAdam keeps EMA weights (ema_decay) but the optimizer state has none")
        for name in ("exp_avg", "exp_avg_sq"):
            if sd[name].numel() != getattr(self, name).numel():
                raise ValueError(f"optimizer state '{name}' has {sd[name].numel()} elements, the module {getattr(self, name).numel()}")
            getattr(self, name).copy_(sd[name].reshape(-1))
        self.steps = int(sd["steps"])
        self.sq_norm[1:2].copy_(sd["skipped"].reshape(-1))
        for g, saved in zip(self.param_groups, sd["param_groups"]):
            g.update({k: (tuple(v) if k == "betas" else v) for k, v in saved.items()})
        if has:
            self.ema_decay, self.ema_warmup = float(sd["ema_decay"]), bool(sd["ema_warmup"])
            if sd["ema"] is None:
                self.ema_params = None
            else:
                if sd["ema"].numel() != self.exp_avg.numel():
                    raise ValueError(f"optimizer state 'ema' has {sd['ema'].numel()} elements, the module {self.exp_avg.numel()}")
                if self.ema_params is None:
                    self.ema_params = torch.empty_like(self.exp_avg)
                self.ema_params.copy_(sd["ema"].reshape(-1))


class _EmaWeights:
    def __init__(self, opt: FlatAdam):
        self.opt = opt

    def __enter__(self):
        opt, mod = self.opt, self.opt.module
        ema = opt._need_ema()
        if opt._in_ema:
            raise RuntimeError("ema_weights() does not nest")
        if mod.training:
            raise RuntimeError("ema_weights(): put the module in eval mode first (module.eval())")
        mod._use_weights(ema)
        opt._in_ema = True
        return opt

    def __exit__(self, *exc):
        self.opt._in_ema = False
        self.opt.module._use_weights(None)             # re-packs the arena from the live parameters
        return False


class FlatModuleAdam:
    """clip_grad_norm_ + AdamW for a plain ``nn.Module`` (the PatchDiscriminator of the stage-1 trainer,
    3d_ldm/train_autoencoder.py:277-279,487-494) on the same two HIP launches as ``FlatAdam``: the module's parameters are re-homed
    as views of one flat fp32 buffer, their ``.grad`` as views of a second one that autograd accumulates into."""

    def __init__(self, module: torch.nn.Module, lr: float, betas=(0.5, 0.9), eps: float = 1e-8, weight_decay: float = 1e-5,
                 max_grad_norm: float | None = 0.5):
        params = [p for p in module.parameters() if p.requires_grad]
        if not params or not params[0].is_cuda:
            raise _lib.LdmError("FlatModuleAdam needs the module on the GPU (no CPU fallback)")
        dev = params[0].device
        total = sum(p.numel() for p in params)
        self.flat_params = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat_grads = torch.zeros(total, dtype=torch.float32, device=dev)
        off = 0
        with torch.no_grad():
            for p in params:
                n = p.numel()
                v = self.flat_params[off:off + n].view(p.shape)
                v.copy_(p.detach().float())
                p.data = v
                p.grad = self.flat_grads[off:off + n].view(p.shape)
                off += n
        self.params = params
        self.lr, self.betas, self.eps, self.weight_decay, self.max_grad_norm = lr, tuple(betas), eps, weight_decay, max_grad_norm
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.flat_params), torch.zeros_like(self.flat_params)
        self.sq_norm = torch.zeros((2,), dtype=torch.float32, device=dev)
        self.steps = 0
        self.param_groups = [dict(lr=lr)]

    def zero_grad(self, set_to_none: bool = False):
        self.flat_grads.zero_()
        off = 0
        for p in self.params:                              # a caller may have dropped the views (set_to_none elsewhere): restore them
            n = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.flat_grads.data_ptr() + 4 * off:
                p.grad = self.flat_grads[off:off + n].view(p.shape)
            off += n

    @torch.no_grad()
    def step(self):
        L = _lib.lib()
        p, g = self.flat_params, self.flat_grads
        clip = self.max_grad_norm is not None and self.max_grad_norm > 0
        self.steps += 1
        with torch.cuda.device(p.device):
            _lib.check(L.ldm_grad_sq_norm(g.data_ptr(), g.numel(), self.sq_norm.data_ptr(), _lib.current_stream()))   # NaN-skip needs it, clip or not
            _lib.check(L.ldm_adam_step(p.data_ptr(), g.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), p.numel(),
                                       float(self.param_groups[0]["lr"]), float(self.betas[0]), float(self.betas[1]), float(self.eps),
                                       float(self.weight_decay), self.steps, self.sq_norm.data_ptr(),
                                       float(self.max_grad_norm or 0.0) if clip else 0.0, _lib.current_stream()))
