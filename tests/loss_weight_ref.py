"""Independent fp64 restatement of the stage-2 objective options (ldm3d/loss_weighting.py, csrc/loss_weight.h), in numpy alone:
the three Min-SNR-gamma formulae, the weighted loss and its gradient, the tracker update in batch order, and the bins, the bin
probabilities, the CDF, the timestep and the importance weight of the loss-aware draw.  Nothing here imports the package."""
import numpy as np


def betas(T, schedule, beta_start, beta_end):
    """The beta schedule as the schedulers build it: fp32 linspace (of the roots for "scaled_linear_beta"), fp32 cumprod of 1 - beta."""
    if schedule == "scaled_linear_beta":
        return np.linspace(np.float32(beta_start ** 0.5), np.float32(beta_end ** 0.5), T, dtype=np.float32) ** 2
    if schedule == "linear_beta":
        return np.linspace(np.float32(beta_start), np.float32(beta_end), T, dtype=np.float32)
    raise ValueError(schedule)


def snr(alphas_cumprod):
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    return ac / (1.0 - ac)


def min_snr(alphas_cumprod, gamma, prediction_type):
    s = snr(alphas_cumprod)
    m = np.minimum(s, float(gamma))
    if prediction_type == "epsilon":
        return m / s
    if prediction_type == "sample":
        return m
    if prediction_type == "v_prediction":
        return m / (s + 1.0)
    raise ValueError(prediction_type)


def weighted_loss(pred, target, timesteps=None, w_table=None, sample_w=None):
    """-> (loss_w, loss_u, per_sample [B], grad [B, n]) in fp64.  A timestep outside the table gives that sample the weight NaN."""
    p, t = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    B = p.shape[0]
    p, t = p.reshape(B, -1), t.reshape(B, -1)
    n = p.shape[1]
    w = np.ones(B, dtype=np.float64)
    if w_table is not None:
        tab = np.asarray(w_table, dtype=np.float64)
        for b in range(B):
            tb = int(timesteps[b])
            w[b] = tab[tb] if 0 <= tb < tab.shape[0] else np.nan
    if sample_w is not None:
        w = w * np.asarray(sample_w, dtype=np.float64)
    d = p - t
    per = (d * d).mean(axis=1)
    grad = 2.0 * w[:, None] * d / (B * n)
    return float((w * per).sum() / B), float(per.sum() / B), per, grad


def bin_of(t, K, T):
    return (int(t) * int(K)) // int(T)


def bin_edges(K, T):
    """lo_0 .. lo_K by exhaustive membership: bin k is the run of timesteps whose bin_of is k."""
    ks = [bin_of(t, K, T) for t in range(T)]
    assert ks == sorted(ks)
    lo = [ks.index(k) if k in ks else None for k in range(K)]
    assert None not in lo
    return lo + [T]


def tracker_update(state, per_sample, timesteps, K, T, beta, order=None):
    """state: fp64 [2, K] (m2, count), updated in place sample by sample in ``order`` (default: batch order)."""
    B = len(per_sample)
    for b in (range(B) if order is None else order):
        l, t = float(per_sample[b]), int(timesteps[b])
        if not np.isfinite(l) or not 0 <= t < T:
            continue
        k = bin_of(t, K, T)
        state[0, k] = l * l if state[1, k] == 0 else beta * state[0, k] + (1.0 - beta) * l * l
        if state[1, k] < 2.0 ** 24:
            state[1, k] += 1.0
    return state


def bin_probabilities(state, K, T, warmup, uniform_prob):
    """-> (P [K], uniform?)"""
    edges = bin_edges(K, T)
    n = np.array([edges[k + 1] - edges[k] for k in range(K)], dtype=np.float64)
    uni = n / float(T)
    s = np.asarray(state, dtype=np.float64)
    if (s[1] < warmup).any():
        return uni, True
    with np.errstate(invalid="ignore"):
        q = n * np.sqrt(s[0])
    sq = q.sum()
    if not (sq > 0.0) or not np.isfinite(sq):
        return uni, True
    return (1.0 - uniform_prob) * q / sq + uniform_prob * uni, False


def cdf(P):
    return np.cumsum(np.asarray(P, dtype=np.float64))


def draw(state, K, T, warmup, uniform_prob, u0, u1):
    """-> (t, iw, k) of one draw (u0, u1)."""
    edges = bin_edges(K, T)
    P, uniform = bin_probabilities(state, K, T, warmup, uniform_prob)
    Cs = cdf(P)
    k = K - 1
    for j in range(K):
        if float(u0) < Cs[j]:
            k = j
            break
    n = edges[k + 1] - edges[k]
    t = edges[k] + min(n - 1, int(np.floor(float(u1) * n)))
    iw = 1.0 if uniform else n / (T * P[k])
    return t, iw, k


def timestep_probability(P, K, T):
    """p(t) of the draw and iw(t), each [T]: a bin's probability spread evenly over its timesteps."""
    edges = bin_edges(K, T)
    p, iw = np.zeros(T), np.zeros(T)
    for k in range(K):
        n = edges[k + 1] - edges[k]
        p[edges[k]:edges[k + 1]] = P[k] / n
        iw[edges[k]:edges[k + 1]] = n / (T * P[k])
    return p, iw
