"""The arithmetic of measurement-guided sampling, written independently of ldm3d/guidance.py and the kernels,
in float64 torch on the CPU: the pool, the residual, g = dL/dx0_hat, (c_x, c_m), zeta and the update.  Explicit loops over the pooling
cubes instead of avg_pool3d / interpolate, so that it shares no code path with what it checks."""
import math

import torch


def pool_mean(x, p):
    """Mean over non-overlapping p^3 cubes per channel: [B, C, d, h, w] -> [B, C, d/p, h/p, w/p]."""
    x = x.double()
    B, C, d, h, w = x.shape
    out = torch.zeros((B, C, d // p, h // p, w // p), dtype=torch.float64)
    for i in range(p):
        for j in range(p):
            for k in range(p):
                out += x[:, :, i::p, j::p, k::p]
    return out / p ** 3


def upsample(q, p):
    """Nearest upsample by p: every pooled cell onto its p^3 cube."""
    B, C, d, h, w = q.shape
    out = torch.zeros((B, C, d * p, h * p, w * p), dtype=torch.float64)
    for i in range(p):
        for j in range(p):
            for k in range(p):
                out[:, :, i::p, j::p, k::p] = q
    return out


def coefs(prediction_type, abar):
    """(c_x, c_m) = (d x0_hat / d x, d x0_hat / d m)."""
    a, s = math.sqrt(abar), math.sqrt(1.0 - abar)
    return {"epsilon": (1.0 / a, -s / a), "sample": (0.0, 1.0), "v_prediction": (a, -s)}[prediction_type]


def x0_hat(prediction_type, abar, x, m):
    """The UNCLIPPED prediction of the clean latent."""
    a, s = math.sqrt(abar), math.sqrt(1.0 - abar)
    x, m = x.double(), m.double()
    if prediction_type == "epsilon":
        return (x - s * m) / a
    if prediction_type == "sample":
        return m
    return a * x - s * m


def residual(x0, target, weight, p):
    r = pool_mean(x0, p) - target.double()
    return r if weight is None else weight.double() * r


def residual_terms(prediction_type, abar, x, m, target, weight, p):
    """-> (r, g, c_m g, c_x g, |r_b| [B]): what the residual kernel produces (its norm2 is |r_b|^2)."""
    r = residual(x0_hat(prediction_type, abar, x, m), target, weight, p)
    wr = r if weight is None else weight.double() * r
    g = upsample(wr.expand(x.shape[0], *wr.shape[1:]), p) / p ** 3
    cx, cm = coefs(prediction_type, abar)
    return r, g, cm * g, cx * g, r.expand(x.shape[0], *r.shape[1:]).reshape(x.shape[0], -1).norm(dim=1)


def zeta(norm, scale, normalize):
    return scale / norm.clamp_min(1e-12) if normalize else torch.full_like(norm, scale)


def grad_x(prediction_type, abar, x, m, vjp, target, weight, p):
    """grad_x L = c_x g + J^T(c_m g); ``vjp(v)`` = J^T v of m = f(x).  -> (grad, |r_b|)."""
    _, _, go, gx, norm = residual_terms(prediction_type, abar, x, m, target, weight, p)
    return gx + vjp(go), norm


def update(prev, grad, norm, scale, normalize):
    """x_{t-1} = prev - zeta_b grad_b, prev = scheduler.step(m, t, x_t)."""
    z = zeta(norm, scale, normalize).reshape((-1,) + (1,) * (grad.dim() - 1))
    return prev.double() - z * grad
