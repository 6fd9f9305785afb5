"""Float64 restatements for the inpainting (RePaint) tests, written from the formulae alone (nothing of ldm3d is imported):

  schedule          the (level, jump) list of a chain: levels count from the noise end, a call at level L arrives at L + 1, and after
                    arriving at a multiple of jump_length (below n_steps) the chain goes back jump_length levels, n_resample - 1 times
  n_calls           the closed form of its length
  merge             x -> the known region put back, then the jump back, from given coefficients and draws
  merge_gate        the per-element bound on |fp32 kernel - merge| from the kernel's spelled-out roundings
  known_coefs / jump_coefs   (ka, ks) and (ja, js) from alpha-bars (DDPM / DDIM) or taus (rectified flow)
"""
import torch


def schedule(n_steps: int, jump_length: int = 1, n_resample: int = 1):
    """Walk the chain, one UNet call at a time, written as a recursion over blocks of ``jump_length`` levels rather than as the package's
    counter loop: levels [0, a) are denoised (recursively), and when a = the end of a block is reached below n_steps, the block
    [a - jump_length, a) is denoised n_resample - 1 more times, each time after a jump back."""
    n, j, r = int(n_steps), int(jump_length), int(n_resample)
    calls = []
    level = 0
    while level < n:
        end = min((level // j + 1) * j, n)                   # the block [level, end)
        block = list(range(level, end))
        repeats = r if (end % j == 0 and end < n) else 1
        for rep in range(repeats):
            for L in block:
                calls.append([L, False])
            if rep + 1 < repeats:
                calls[-1][1] = True                          # the call that arrived at `end` carries the jump
        level = end
    return [(L, jmp) for L, jmp in calls]


def n_calls(n_steps: int, jump_length: int = 1, n_resample: int = 1) -> int:
    return n_steps + (n_resample - 1) * jump_length * ((n_steps - 1) // jump_length)


def known_coefs(abar=None, tau=None):
    """(ka, ks) of the known region at a level: sqrt(abar), sqrt(1 - abar) | 1 - tau, tau"""
    if tau is not None:
        return 1.0 - float(tau), float(tau)
    return float(abar) ** 0.5, (1.0 - float(abar)) ** 0.5


def jump_coefs(a=None, b=None, tau_a=None, tau_b=None):
    """(ja, js) of the Gaussian that carries the marginal of level a back to that of the noisier level b"""
    if tau_a is not None:
        ja = (1.0 - float(tau_b)) / (1.0 - float(tau_a))
        return ja, (float(tau_b) ** 2 - ja ** 2 * float(tau_a) ** 2) ** 0.5
    ratio = float(b) / float(a)
    return ratio ** 0.5, (1.0 - ratio) ** 0.5


def _expand(known, keep, x):
    """known [1 or B, C, DHW] and keep [DHW] broadcast to x [B, C, DHW] (float64 CPU)"""
    return known.double().cpu().expand_as(x), (keep.double().cpu() != 0).expand_as(x)


def merge(x, known, keep, coef4, jump, z_known=None, z_jump=None):
    """x [B, C, DHW] -> where keep: ka known + ks z_known; with jump: ja (that) + js z_jump.  float64."""
    ka, ks, ja, js = (float(c) for c in coef4)
    x = x.double().cpu()
    kn, kp = _expand(known, keep, x)
    zk = torch.zeros_like(x) if z_known is None else z_known.double().cpu()
    zj = torch.zeros_like(x) if z_jump is None else z_jump.double().cpu()
    out = torch.where(kp, ka * kn + ks * zk, x)
    if jump:
        out = ja * out + js * zj
    return out


def merge_gate(x, known, keep, coef4, jump, z_known=None, z_jump=None):
    """The per-element bound on |fp32 kernel - merge|, derived as warm_start_ref.start_gate is.  u = 2^-24 is one rounding's relative
    error.  Merge (kept elements only): the product ks z and the fused multiply-add round once each, at most u |ks z| and
    u (|ka known| + |ks z|) (to first order), together under 2 u (|ka known| + |ks z|); with ks = 0 the one product ka known rounds
    once, inside the same bound.  An element that is not kept enters the jump exact.  Jump: the incoming error e arrives scaled by
    |ja|; the product js z and the fused multiply-add round once each, under 2 u (|ja| (|m| + e) + |js z|) with m the exact merged value.
    A factor (1 + 2^-20) covers the second-order terms."""
    ka, ks, ja, js = (abs(float(c)) for c in coef4)
    u = 2.0 ** -24
    xa = x.double().cpu().abs()
    kn, kp = _expand(known, keep, xa)
    zk = torch.zeros_like(xa) if z_known is None else z_known.double().cpu().abs()
    zj = torch.zeros_like(xa) if z_jump is None else z_jump.double().cpu().abs()
    mag = torch.where(kp, ka * kn.abs() + ks * zk, xa)       # a bound on |m|
    err = torch.where(kp, 2.0 * u * mag, torch.zeros_like(xa))
    if jump:
        err = ja * err + 2.0 * u * (ja * (mag + err) + js * zj)
    return err * (1.0 + 2.0 ** -20)
