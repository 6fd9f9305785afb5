"""Per-voxel statistics of an ensemble of sampled volumes (K draws of one scan's posterior): the mean is the denoised estimate, the
standard deviation says where the model is unsure.  ``EnsembleAccumulator`` folds members into a running (mean, m2) state on the
device (``ldm_ensemble_update``, Welford's recurrence, csrc/ensemble.h) as they are decoded, so no stack of K volumes is ever held;
``ldm_ensemble_finalize`` reads the std map and the scalar statistics off it.  The state's bits do not depend on how the members are
split over ``update`` calls.  There is no CPU path: CPU tensors raise ``LdmError``."""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from .sliding import default_batch as default_member_batch  # noqa: F401  (members per UNet call: the one rule)

STAT_NAMES = ("mean_std", "max_std", "mean_var", "bias_sq")


def plan_chunks(n_members: int, member_batch: int) -> List[Tuple[int, int]]:
    """``[(first, size), ...]``: members 0 .. n_members - 1 in order, ``member_batch`` at a time (the last chunk takes what is left)."""
    n, b = int(n_members), int(member_batch)
    if n < 1 or b < 1:
        raise ValueError(f"n_members and member_batch must be positive, got {n_members} and {member_batch}")
    return [(first, min(b, n - first)) for first in range(0, n, b)]


class EnsembleResult(NamedTuple):
    mean: torch.Tensor                       # [1, C, D, H, W]
    std: torch.Tensor                        # [1, C, D, H, W]
    count: int
    stats: Dict[str, float]
    members: Optional[torch.Tensor]          # the first keep_members volumes [keep, C, D, H, W], or None


class EnsembleAccumulator:
    """Running per-voxel mean and sum of squared deviations of the volumes passed to ``update``."""

    def __init__(self, shape: Sequence[int], device):
        self.shape = tuple(int(s) for s in shape)
        self.n = math.prod(self.shape)
        if self.n < 1:
            raise ValueError(f"empty shape {self.shape}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.LdmError("EnsembleAccumulator runs on the GPU only (there is no CPU path)")
        self._mean = torch.empty(self.shape, dtype=torch.float32, device=self.device)      # never zeroed: count == 0 says "ignore"
        self._m2 = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        self._stats = torch.empty((8,), dtype=torch.float32, device=self.device)
        self._scratch = torch.empty((_lib.lib().ldm_ensemble_stats_scratch_bytes(self.n),), dtype=torch.uint8, device=self.device)
        self.count = 0

    def reset(self) -> None:
        self.count = 0

    def update(self, members: torch.Tensor) -> None:
        """Fold ``members`` [B, *shape] (fp32, on the accumulator's device) in order.  Each member must be contiguous; the members may
        be any stride >= a member's size apart (a leading view of a wider buffer is passed as it is)."""
        if not isinstance(members, torch.Tensor) or not members.is_cuda or members.device != self.device:
            raise _lib.LdmError(f"update takes a CUDA tensor on {self.device} (there is no CPU path)")
        if members.dtype != torch.float32:
            raise TypeError(f"update takes fp32 members, got {members.dtype}")
        if members.dim() != len(self.shape) + 1 or tuple(members.shape[1:]) != self.shape or members.shape[0] < 1:
            raise ValueError(f"members must be [B, {', '.join(map(str, self.shape))}] with B >= 1, got {tuple(members.shape)}")
        members = members.detach()
        B = members.shape[0]
        if not members[0].is_contiguous():
            raise ValueError("every member must be contiguous (strides %s)" % (tuple(members.stride()),))
        stride = members.stride(0) if B > 1 else self.n
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ldm_ensemble_update(members.data_ptr(), B, stride, self.n, self._mean.data_ptr(), self._m2.data_ptr(),
                                                      self.count, _lib.current_stream()))
        self.count += B

    def _finalize(self, target: Optional[torch.Tensor], ddof: int, std_out: Optional[torch.Tensor]) -> None:
        if self.count < 1:
            raise ValueError("no member has been folded yet")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ldm_ensemble_finalize(self._mean.data_ptr(), self._m2.data_ptr(), self.count, int(ddof), _lib.ptr(target),
                                                        _lib.ptr(std_out), self._stats.data_ptr(), self._scratch.data_ptr(),
                                                        self._scratch.numel(), self.n, _lib.current_stream()))

    def mean(self) -> torch.Tensor:
        """The members' mean so far (a copy)."""
        if self.count < 1:
            raise ValueError("no member has been folded yet")
        return self._mean.clone()

    def m2(self) -> torch.Tensor:
        """The sum of squared deviations from the mean so far (a copy; exactly 0 after one member)."""
        if self.count < 1:
            raise ValueError("no member has been folded yet")
        return self._m2.clone()

    def std(self, ddof: int = 1) -> torch.Tensor:
        """``sqrt(max(m2, 0) / (count - ddof))`` per voxel; ``ddof`` 1 (sample, needs two members) or 0 (population)."""
        out = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        self._finalize(None, ddof, out)
        return out

    def stats(self, target: Optional[torch.Tensor] = None, ddof: int = 1) -> Dict[str, float]:
        """``mean_std``, ``max_std``, ``mean_var`` over the voxels and, against a ``target`` volume of the accumulator's size,
        ``bias_sq = mean((mean - target)^2)`` (0.0 without one), as Python floats (one read-back).  With ``ddof=0``,
        ``bias_sq + mean_var`` is the mean over the members of their MSE against the target."""
        tgt = None
        if target is not None:
            if not target.is_cuda or target.device != self.device:
                raise _lib.LdmError(f"target must be a CUDA tensor on {self.device}")
            if target.numel() != self.n:
                raise ValueError(f"target has {target.numel()} elements, the ensemble {self.n}")
            tgt = target.detach().to(torch.float32).contiguous()
        self._finalize(tgt, ddof, None)
        vals = self._stats.tolist()
        return {name: float(vals[i]) for i, name in enumerate(STAT_NAMES)}
