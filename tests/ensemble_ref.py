"""Independent restatement of the ensemble statistics on torch CPU (no library code): Welford's recurrence in a chosen dtype, a two-pass
mean / sum of squared deviations, the naive sum / sum-of-squares variant in fp32 that the kernels must NOT be, and the scalar statistics.
Members are [K, n] (or [K, ...]) tensors; everything is per element along dim 0."""
import torch


def welford(members: torch.Tensor, dtype=torch.float64, mean=None, m2=None, count=0):
    """The recurrence, one member at a time, every operation rounded in ``dtype``: c += 1; d = x - mean; mean += d / c;
    m2 += d * (x - mean).  Returns (mean, m2, count)."""
    x = members.to(dtype)
    for k in range(x.shape[0]):
        count += 1
        if count == 1:
            mean, m2 = x[k].clone(), torch.zeros_like(x[k])
            continue
        d = x[k] - mean
        mean = mean + d / torch.tensor(float(count), dtype=dtype)
        m2 = m2 + d * (x[k] - mean)
    return mean, m2, count


def two_pass(members: torch.Tensor):
    """fp64 mean, then the sum of squared deviations from it."""
    x = members.double()
    mean = x.sum(dim=0) / x.shape[0]
    return mean, ((x - mean) ** 2).sum(dim=0)


def naive_fp32(members: torch.Tensor):
    """What a sum / sum-of-squares kernel would compute in fp32: m2 = sum x^2 - (sum x)^2 / K."""
    x = members.float()
    s = torch.zeros_like(x[0])
    ss = torch.zeros_like(x[0])
    for k in range(x.shape[0]):
        s = s + x[k]
        ss = ss + x[k] * x[k]
    K = torch.tensor(float(x.shape[0]), dtype=torch.float32)
    return s / K, ss - s * s / K


def stats(mean: torch.Tensor, m2: torch.Tensor, count: int, ddof: int = 1, target=None) -> dict:
    """The scalars in fp64 from a given (mean, m2) state."""
    var = m2.double().clamp_min(0.0) / (count - ddof)
    sd = var.sqrt()
    out = {"mean_std": float(sd.mean()), "max_std": float(sd.max()), "mean_var": float(var.mean()), "bias_sq": 0.0}
    if target is not None:
        out["bias_sq"] = float(((mean.double() - target.double().reshape(mean.shape)) ** 2).mean())
    return out


def family(name: str, K: int, n: int, seed: int) -> torch.Tensor:
    """The two input families of the tests, [K, n] fp32: "unit" = clamp(0.5 + 0.3 randn, 0, 1.2) (a scaled scan), "offset" =
    100 + 0.01 randn (a spread far below the level: where a sum of squares loses everything)."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn((K, n), generator=g, dtype=torch.float32)
    if name == "unit":
        return (0.5 + 0.3 * r).clamp(0.0, 1.2)
    if name == "offset":
        return 100.0 + 0.01 * r
    raise ValueError(name)


def gates(members: torch.Tensor):
    """(mean gate, m2 gate, mean yardstick, m2 yardstick, fp64 mean, fp64 m2): the yardstick is the max-abs error of the fp32 CPU
    recurrence against the fp64 one on the same inputs; gate = 2 x yardstick + 2 * 2^-24 * max|x| (mean) or * max(m2_fp64) (m2)."""
    m64, s64, _ = welford(members, torch.float64)
    m32, s32, _ = welford(members, torch.float32)
    ym = float((m32.double() - m64).abs().max())
    ys = float((s32.double() - s64).abs().max())
    ulp = 2.0 * 2.0 ** -24
    return 2 * ym + ulp * float(members.abs().max()), 2 * ys + ulp * float(s64.max()), ym, ys, m64, s64
