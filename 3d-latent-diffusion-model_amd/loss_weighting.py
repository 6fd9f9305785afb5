"""The stage-2 objective beyond the reference's plain mean (3d_ldm/train_diffusion.py:185-187 randint, :207 mse_loss): per-timestep
loss weights and a loss-aware draw of the training timesteps, both opt-in (``DiffusionTrainer(loss_weighting=..., timestep_sampling=...)``).

* ``min_snr_weights``: the Min-SNR-gamma table (Hang et al. 2023, "Efficient Diffusion Training via Min-SNR Weighting Strategy"; the
  ``--snr_gamma`` of the diffusers trainers) for the scheduler's ``prediction_type``, with snr_t = abar_t / (1 - abar_t):
  epsilon ``min(snr, g) / snr``, sample ``min(snr, g)``, v_prediction ``min(snr, g) / (snr + 1)``.  Built on the host in fp64 from the
  scheduler's ``alphas_cumprod``, stored fp32; there is no kernel for it.
* ``weighted_mse_loss``: ``(1/B) sum_b w_b mean_i (pred - target)^2`` with ``w_b = w_table[t_b] * sample_w[b]``, its gradient and the
  update of a ``LossTracker`` in two HIP launches (``ldm_op_weighted_mse_loss``).
* ``LossTracker``: an exponential moving average of the squared per-sample loss per bin of timesteps, and the draw of a batch's
  timesteps with probability proportional to (bin size x) the root of it, with the importance weights that keep the objective the
  uniform one (``ldm_timestep_resample``, one launch, no host read).  This is the loss-second-moment resampler of Improved DDPM
  (Nichol & Dhariwal 2021) with three changes that are this project's own: an EMA in place of its 10-entry history, bins of timesteps
  in place of single timesteps, and no collective (each rank keeps its own tracker; each is unbiased on its own).

There is no CPU fallback: the loss and the draw raise without a GPU; only the table is host arithmetic.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch

from . import _lib

MAX_BINS = 64                                            # LW_BINS_MAX of csrc/loss_weight.h
MAX_BATCH = 64                                           # LATENT_BATCH_MAX
LOSS_WEIGHTINGS = ("none", "min_snr")
TIMESTEP_SAMPLINGS = ("uniform", "loss_aware")


def min_snr_weights(scheduler, gamma: float = 5.0) -> torch.Tensor:
    """The ``[num_train_timesteps]`` fp32 Min-SNR-gamma table of ``scheduler`` (a DDPM-family scheduler with ``alphas_cumprod`` and a
    ``prediction_type``), on the CPU.  ``RFlowScheduler`` has no abar table and a timestep draw of its own: ``NotImplementedError``."""
    if not hasattr(scheduler, "alphas_cumprod") or not hasattr(scheduler, "prediction_type"):
        raise NotImplementedError(f"min_snr_weights: {type(scheduler).__name__} has no alphas_cumprod / prediction_type "
                                  "(loss weights for rectified flow are not built)")
    gamma = float(gamma)
    if not gamma > 0.0 or gamma != gamma or gamma == float("inf"):
        raise ValueError(f"min_snr_weights: gamma must be positive and finite, got {gamma}")
    ac = scheduler.alphas_cumprod.detach().to(device="cpu", dtype=torch.float64)
    snr = ac / (1.0 - ac)
    clamped = torch.clamp(snr, max=gamma)
    kind = scheduler.prediction_type
    if kind == "epsilon":
        w = clamped / snr
    elif kind == "sample":
        w = clamped
    elif kind == "v_prediction":
        w = clamped / (snr + 1.0)
    else:
        raise ValueError(f"min_snr_weights: unknown prediction_type {kind!r}")
    return w.to(torch.float32)


def _f32(t: Optional[torch.Tensor], dev, n: int, what: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
    if t.numel() != n:
        raise ValueError(f"weighted_mse_loss: {what} has {t.numel()} elements, expected {n}")
    return t


class _WeightedMseLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, timesteps, w_table, sample_w, tracker):
        p = pred.detach().to(torch.float32).contiguous()
        if not p.is_cuda:
            raise _lib.LdmError("weighted_mse_loss: CUDA tensors only (no CPU fallback)")
        t = target.detach().to(device=p.device, dtype=torch.float32).contiguous()
        if p.shape != t.shape:
            raise ValueError(f"weighted_mse_loss: shapes differ: {tuple(p.shape)} vs {tuple(t.shape)}")
        if p.dim() < 1 or p.numel() == 0:
            raise ValueError("weighted_mse_loss: pred must be [B, ...] with at least one element")
        B = p.shape[0]
        ts = None
        if timesteps is not None:
            ts = timesteps.detach().to(device=p.device, dtype=torch.int64).contiguous()
            if ts.numel() != B:
                raise ValueError(f"weighted_mse_loss: {B} samples but {ts.numel()} timesteps")
        if ts is None and (w_table is not None or tracker is not None):
            raise ValueError("weighted_mse_loss: a weight table or a tracker needs the timesteps")
        T = tracker.num_train_timesteps if tracker is not None else 1
        wt = None
        if w_table is not None:
            wt = w_table.detach().to(device=p.device, dtype=torch.float32).contiguous()
            if tracker is not None and wt.numel() != T:
                raise ValueError(f"weighted_mse_loss: a table of {wt.numel()} weights but a tracker over {T} timesteps")
            T = wt.numel()
        sw = _f32(sample_w, p.device, B, "sample_w")
        state = None
        if tracker is not None:
            state = tracker.state
            if state.device != p.device:
                raise ValueError("weighted_mse_loss: the tracker lives on another device")
        loss = torch.empty((2,), dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p)
        with torch.cuda.device(p.device):
            _lib.check(_lib.lib().ldm_op_weighted_mse_loss(
                p.data_ptr(), t.data_ptr(), B, p.numel() // B, _lib.ptr(ts), _lib.ptr(wt), int(T), _lib.ptr(sw), _lib.ptr(state),
                tracker.n_bins if tracker is not None else 1, float(tracker.beta) if tracker is not None else 0.0,
                loss.data_ptr(), None, grad.data_ptr(), _lib.current_stream()))
        ctx.save_for_backward(grad)
        weighted, unweighted = loss[0].clone(), loss[1].clone()
        ctx.mark_non_differentiable(unweighted)
        return weighted, unweighted

    @staticmethod
    def backward(ctx, g, _g_unweighted):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None, None, None


def weighted_mse_loss(pred: torch.Tensor, target: torch.Tensor, timesteps: Optional[torch.Tensor], w_table: Optional[torch.Tensor] = None,
                      sample_w: Optional[torch.Tensor] = None, tracker: Optional["LossTracker"] = None):
    """-> ``(loss, unweighted)``, two 0-dim device tensors: ``loss = (1/B) sum_b w_table[t_b] sample_w[b] l_b`` with ``l_b`` the mean
    squared error of sample b (differentiable w.r.t. ``pred`` only; the gradient ``2 w_b (pred - target) / numel`` is written by the
    forward launch) and ``unweighted = (1/B) sum_b l_b``, the figure ``optim.mse_loss`` returns.  ``tracker`` is updated with the
    unweighted ``l_b`` in batch order by the same launch.  A timestep outside the table makes that sample's weight, the loss and the
    sample's gradient NaN (the optimizer's NaN-skip then counts the step).  With neither weights nor tracker and one sample both values
    are ``optim.mse_loss``'s bit for bit."""
    return _WeightedMseLossFn.apply(pred, target, timesteps, w_table, sample_w, tracker)


class LossTracker:
    """Second moment of the per-sample loss per bin of timesteps, and the loss-aware timestep draw.  Bin k holds the timesteps t with
    ``(t * n_bins) // num_train_timesteps == k``.  ``state`` is a device fp32 ``[2, n_bins]`` tensor: row 0 the moving second moments
    (``m2 = beta m2 + (1 - beta) l^2``; the first sample of a bin sets it), row 1 the counts.  Until every bin has been seen ``warmup``
    times the draw is uniform and every importance weight is exactly 1."""

    def __init__(self, num_train_timesteps: int, n_bins: int = 20, beta: float = 0.9, warmup: int = 10, uniform_prob: float = 1e-3,
                 device=None):
        T, K = int(num_train_timesteps), int(n_bins)
        if T < 1:
            raise ValueError(f"LossTracker: num_train_timesteps must be positive, got {num_train_timesteps}")
        if not 1 <= K <= min(MAX_BINS, T):
            raise ValueError(f"LossTracker: n_bins must lie in 1 .. min({MAX_BINS}, num_train_timesteps = {T}), got {n_bins}")
        if not 0.0 <= float(beta) < 1.0:
            raise ValueError(f"LossTracker: beta must lie in [0, 1), got {beta}")
        if not 0.0 <= float(uniform_prob) <= 1.0:
            raise ValueError(f"LossTracker: uniform_prob must lie in [0, 1], got {uniform_prob}")
        if int(warmup) < 0:
            raise ValueError(f"LossTracker: warmup must not be negative, got {warmup}")
        self.num_train_timesteps, self.n_bins = T, K
        self.beta, self.warmup, self.uniform_prob = float(beta), int(warmup), float(uniform_prob)
        self.state = torch.zeros((2, K), dtype=torch.float32, device=device)

    def to(self, device) -> "LossTracker":
        self.state = self.state.to(device)
        return self

    def bin_edges(self) -> List[int]:
        """``lo_0 .. lo_K``: bin k is ``range(lo_k, lo_{k+1})``, ``lo_k = ceil(k T / K)``."""
        T, K = self.num_train_timesteps, self.n_bins
        return [(k * T + K - 1) // K for k in range(K + 1)]

    def sample(self, B: int, like: torch.Tensor, idx=None, seed: int = 0, step: int = 0, draw: Optional[torch.Tensor] = None):
        """-> ``(timesteps int64 [B], iw fp32 [B])`` on ``like``'s device in one launch.  The draw of sample b is keyed by ``(seed, step)``
        and the dataset index ``idx[b]`` (default: the batch slot), never by the slot itself; ``draw`` ([B, 2] uniforms in [0, 1))
        replaces the kernel's own."""
        dev = like.device
        if dev.type != "cuda":
            raise _lib.LdmError("LossTracker.sample: CUDA tensors only (no CPU fallback)")
        if self.state.device != dev:
            self.state = self.state.to(dev)
        B = int(B)
        ids = None
        if idx is not None:
            idx = [int(i) for i in (idx.reshape(-1).tolist() if isinstance(idx, torch.Tensor) else idx)]
            if len(idx) != B:
                raise ValueError(f"LossTracker.sample: {B} samples but {len(idx)} indices")
            ids = (C.c_int * B)(*idx)
        d = None
        if draw is not None:
            d = draw.detach().to(device=dev, dtype=torch.float32).contiguous()
            if tuple(d.shape) != (B, 2):
                raise ValueError(f"LossTracker.sample: draw must be [{B}, 2], got {tuple(d.shape)}")
        t = torch.empty((max(B, 0),), dtype=torch.int64, device=dev)
        iw = torch.empty((max(B, 0),), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ldm_timestep_resample(self.state.data_ptr(), self.n_bins, self.num_train_timesteps, self.warmup,
                                                        self.uniform_prob, ids, B, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF,
                                                        _lib.ptr(d), t.data_ptr(), iw.data_ptr(), _lib.current_stream()))
        return t, iw

    def probabilities(self, state: Optional[torch.Tensor] = None) -> List[float]:
        """The bin probabilities the draw uses for ``state`` (default: the tracker's own, one host read), in fp64 on the host."""
        s = (self.state if state is None else state).detach().to(device="cpu", dtype=torch.float64)
        edges, T = self.bin_edges(), float(self.num_train_timesteps)
        n = [float(edges[k + 1] - edges[k]) for k in range(self.n_bins)]
        uniform = [v / T for v in n]
        if bool((s[1] < self.warmup).any()):
            return uniform
        q = [n[k] * float(s[0, k]) ** 0.5 if float(s[0, k]) >= 0.0 else float("nan") for k in range(self.n_bins)]
        sq = sum(q)
        if not (sq > 0.0) or sq != sq or sq == float("inf"):
            return uniform
        return [(1.0 - self.uniform_prob) * q[k] / sq + self.uniform_prob * uniform[k] for k in range(self.n_bins)]

    def report(self) -> List[dict]:
        """Per bin ``lo``, ``hi`` (inclusive), ``rms_loss = sqrt(m2)``, ``count`` and the draw's ``prob``.  The only host read of the
        tracker: call it at validation time, not inside the step."""
        s = self.state.detach().to(device="cpu", dtype=torch.float64)
        edges, prob = self.bin_edges(), self.probabilities(s)
        return [{"lo": edges[k], "hi": edges[k + 1] - 1, "rms_loss": max(float(s[0, k]), 0.0) ** 0.5 if float(s[0, k]) == float(s[0, k]) else float("nan"),
                 "count": int(s[1, k]), "prob": prob[k]} for k in range(self.n_bins)]

    def state_dict(self) -> dict:
        return {"state": self.state.detach().clone(), "num_train_timesteps": self.num_train_timesteps, "n_bins": self.n_bins,
                "beta": self.beta, "warmup": self.warmup, "uniform_prob": self.uniform_prob}

    def load_state_dict(self, sd: dict) -> None:
        if int(sd["num_train_timesteps"]) != self.num_train_timesteps or int(sd["n_bins"]) != self.n_bins:
            raise ValueError(f"LossTracker: the saved tracker has {sd['n_bins']} bins over {sd['num_train_timesteps']} timesteps, this one "
                             f"{self.n_bins} over {self.num_train_timesteps}")
        self.beta, self.warmup, self.uniform_prob = float(sd["beta"]), int(sd["warmup"]), float(sd["uniform_prob"])
        self.state.copy_(sd["state"].to(device=self.state.device, dtype=torch.float32).reshape(2, self.n_bins))
