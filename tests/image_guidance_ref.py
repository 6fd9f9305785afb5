"""The arithmetic of image-space measurement guidance in float64 torch on the CPU, written independently of
ldm3d/guidance.py and the kernels: avg_pool3d for P, a nearest upsample for its adjoint, torch autograd through a ``decode`` and a
``unet`` callable (the tests pass the CPU oracle's) for the two VJPs.

    x0_hat = (x - s m)/a | m | a x - s m;  z0 = x0_hat / sf;  y_hat = decode(z0)
    r = w (P y_hat - y);  L_b = 1/2 |r_b|^2;  g_img = pool^-3 upsample_nearest(w r);  dz = Dec'^T g_img
    grad_x L = c_x dz / sf + J^T(c_m dz / sf);  x_{t-1} = step(m, t, x_t) - zeta_b grad_x L_b
"""
import math

import torch
import torch.nn.functional as F


def pool(y, p):
    """P: mean over non-overlapping p^3 cubes per channel."""
    return y.double() if p == 1 else F.avg_pool3d(y.double(), p)


def pool_t(q, p):
    """P^T: every pooled cell's value / p^3 onto its cube."""
    q = q.double()
    if p == 1:
        return q
    return q.repeat_interleave(p, 2).repeat_interleave(p, 3).repeat_interleave(p, 4) / p ** 3


def coefs(prediction_type, abar):
    a, s = math.sqrt(abar), math.sqrt(1.0 - abar)
    return {"epsilon": (1.0 / a, -s / a), "sample": (0.0, 1.0), "v_prediction": (a, -s)}[prediction_type]


def x0_hat(prediction_type, abar, x, m):
    a, s = math.sqrt(abar), math.sqrt(1.0 - abar)
    x, m = x.double(), m.double()
    return {"epsilon": lambda: (x - s * m) / a, "sample": lambda: m, "v_prediction": lambda: a * x - s * m}[prediction_type]()


def z0(prediction_type, abar, x, m, sf):
    return x0_hat(prediction_type, abar, x, m) / sf


def _full(t, B):
    return None if t is None else t.double().expand(B, *t.shape[1:])


def residual(y_hat, target, weight, p):
    """r = w (P y_hat - y), [B, C, D/p, H/p, W/p]; target / weight with batch 1 or B (weight may be None)."""
    B = y_hat.shape[0]
    r = pool(y_hat, p) - _full(target, B)
    return r if weight is None else _full(weight, B) * r


def loss(y_hat, target, weight, p):
    """L_b = 1/2 |r_b|^2, [B]."""
    return 0.5 * residual(y_hat, target, weight, p).reshape(y_hat.shape[0], -1).pow(2).sum(1)


def image_terms(y_hat, target, weight, p):
    """-> (g_img = dL/dy_hat [B, C, D, H, W], |r_b|^2 [B]): what image_residual_kernel and its fold produce."""
    r = residual(y_hat, target, weight, p)
    wr = r if weight is None else _full(weight, y_hat.shape[0]) * r
    return pool_t(wr, p), r.reshape(r.shape[0], -1).pow(2).sum(1)


def chain(prediction_type, abar, dz, sf):
    """-> (c_m dz / sf, c_x dz / sf): the grad_out of the UNet's input VJP and the direct term."""
    cx, cm = coefs(prediction_type, abar)
    d = dz.double() / sf
    return cm * d, cx * d


def zeta(norm, scale, normalize):
    return scale / norm.clamp_min(1e-12) if normalize else torch.full_like(norm, scale)


def guided_step(prediction_type, abar, x, unet, decode, step, target, weight, p, sf, scale, normalize):
    """One step on x_t = ``x`` (fp32): ``unet(x)`` -> m and ``decode(z)`` -> image are differentiated by autograd, ``step(m)`` is the
    scheduler's x_{t-1}.  -> (x_{t-1} guided [fp64], |r_b| [B], m, grad_x L [fp64])."""
    xg = x.clone().requires_grad_(True)
    m = unet(xg)
    y_hat = decode((z0(prediction_type, abar, xg, m, sf)).to(x.dtype))
    L = loss(y_hat, target, weight, p)
    grad, = torch.autograd.grad(L.sum(), xg)
    norm = (2.0 * L.detach()).sqrt()
    z = zeta(norm, scale, normalize).reshape((-1,) + (1,) * (x.dim() - 1))
    return step(m.detach()).double() - z * grad.double(), norm, m.detach(), grad.double()
