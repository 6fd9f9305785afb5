"""Yardsticks of the stage-1 GAN tail, the optimizer tail and the percentile scaling (tests only, CPU): plain torch / numpy restatements
in float64 of what the ldm_op_* entries compute, on the library's layouts.

    im2col      col[m][tap * C + c] = x[voxel(m, tap)][c], taps ordered (kd, kh, kw), zero in the padding and in columns taps * C .. Kp
    col2im      its adjoint: dx[voxel][c] = sum of dcol[m][tap * C + c] over the (m, tap) pairs that read the voxel; channels C .. Cs zero
    wgrad slabs dw[s] = dy[rows of split s][:cout]^T x[rows of split s], the rows cut in 16-row steps, ceil(steps / ksplit) steps per split
    adam        torch.optim.Adam / AdamW (decoupled decay) with the clip factor of clip_grad_norm_ folded into the gradient and the
                bias corrections taken at an effective step (the library's step - skipped)

Each function takes the defect a gate must be able to see as an argument, so that tests/test_gan_ops_cpu.py (and the GPU files) can
show the gate's negative control on the same code.  tests/test_gan_ops_cpu.py pins these against F.conv3d, autograd and torch.optim."""
import numpy as np
import torch


# k, stride, pad, (D, H, W): the smallest shapes that reach every guard of im2col_generic_kernel / col2im_generic_kernel
GEOMETRIES = [
    (4, 2, 1, (9, 11, 7)),     # odd extents: the last input plane is read by fewer taps, and od >= Do fires in col2im
    (4, 1, 1, (7, 7, 7)),
    (4, 2, 1, (4, 4, 4)),      # Do = 2
    (3, 1, 1, (5, 6, 7)),
    (3, 2, 0, (7, 5, 9)),
    (1, 1, 0, (3, 2, 5)),
    (4, 3, 2, (10, 8, 9)),
    (4, 1, 1, (3, 3, 3)),      # Do = 2; every tap touches padding
]


def out_dims(dims, k, stride, pad):
    return tuple((s + 2 * pad - k) // stride + 1 for s in dims)


def tap_index(kd, kh, kw, k, order="dhw"):
    """(kd, kh, kw) is the library's order; "whd" is the named defect (taps enumerated (kw, kh, kd))."""
    return (kd * k + kh) * k + kw if order == "dhw" else (kw * k + kh) * k + kd


def im2col_ref(x, C, k, stride, pad, Kp, order="dhw", tail=0.0):
    """x [N][D][H][W][Cs] (any dtype; channels C .. Cs are never read) -> col [N * Do * Ho * Wo][Kp] of the same dtype: pure data movement,
    so the result is exact in every dtype.  tail: what the columns k^3 C .. Kp hold (0; NaN = the defect "Kp tail left unwritten")."""
    N, D, H, W = x.shape[:4]
    Do, Ho, Wo = out_dims((D, H, W), k, stride, pad)
    xp = torch.zeros((N, D + 2 * pad, H + 2 * pad, W + 2 * pad, C), dtype=x.dtype)
    xp[:, pad:pad + D, pad:pad + H, pad:pad + W] = x[..., :C]
    col = torch.full((N * Do * Ho * Wo, Kp), tail, dtype=x.dtype)
    for kd in range(k):
        for kh in range(k):
            for kw in range(k):
                t = tap_index(kd, kh, kw, k, order)
                v = xp[:, kd:kd + stride * (Do - 1) + 1:stride, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride]
                col[:, t * C:(t + 1) * C] = v.reshape(-1, C)
    return col


def col2im_ref(dcol, N, dims, Cs, C, k, stride, pad, drop_last_plane=False):
    """dcol [M][Kp] (columns >= k^3 C never read) -> dx [N][D][H][W][Cs] float64, channels C .. Cs zero.  drop_last_plane: the defect of an
    `od >= Do` guard that is off by one (od >= Do - 1): the contributions of the last output plane of every axis are dropped."""
    D, H, W = dims
    Do, Ho, Wo = out_dims(dims, k, stride, pad)
    d = dcol.double().reshape(N, Do, Ho, Wo, -1)
    if drop_last_plane:
        d = d.clone()
        d[:, Do - 1] = 0
        d[:, :, Ho - 1] = 0
        d[:, :, :, Wo - 1] = 0
    dxp = torch.zeros((N, D + 2 * pad, H + 2 * pad, W + 2 * pad, C), dtype=torch.float64)
    for kd in range(k):
        for kh in range(k):
            for kw in range(k):
                t = tap_index(kd, kh, kw, k)
                dxp[:, kd:kd + stride * (Do - 1) + 1:stride, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride] += \
                    d[..., t * C:(t + 1) * C]
    dx = torch.zeros((N, D, H, W, Cs), dtype=torch.float64)
    dx[..., :C] = dxp[:, pad:pad + D, pad:pad + H, pad:pad + W]
    return dx


def weight_matrix(w, Kp):
    """MONAI layout [cout][cin][kd][kh][kw] -> GEMM rows [cout][Kp] with column = tap * cin + c, as ldm3d/discriminator.py reshapes it."""
    cout, cin = w.shape[:2]
    wm = torch.zeros((cout, Kp), dtype=w.dtype)
    wm[:, :w[0].numel()] = w.permute(0, 2, 3, 4, 1).reshape(cout, -1)
    return wm


def wgrad_split_rows(M, ksplit):
    """Row range [r0, r1) of every split of ldm_op_gemm_wgrad_f32 (r0 == r1: an empty split, whose slab must be zero)."""
    steps = (M + 15) // 16
    sps = (steps + ksplit - 1) // ksplit
    return [(min(M, s * sps * 16), min(M, (s + 1) * sps * 16)) for s in range(ksplit)]


def wgrad_slabs_ref(dy, x, cout, ksplit, empty=0.0):
    """dy [M][cdy], x [M][K] -> [ksplit][cout][K] float64; empty: what an empty split holds (0; NaN = the defect "left unwritten")."""
    out = torch.full((ksplit, cout, x.shape[1]), empty, dtype=torch.float64)
    for s, (r0, r1) in enumerate(wgrad_split_rows(dy.shape[0], ksplit)):
        if r1 > r0:
            out[s] = dy[r0:r1, :cout].double().t() @ x[r0:r1].double()
    return out


def leaky_ref(x, slope):
    """v > 0 ? v : slope * v evaluated in fp32 on x (fp32 or bf16), stored in x's dtype (round to nearest even)."""
    v = x.float()
    return torch.where(v > 0, v, torch.tensor(slope, dtype=torch.float32) * v).to(x.dtype)


def leaky_bwd_ref(x, dy, slope, zero_is_positive=False):
    """x > 0 ? dy : slope * dy in fp32; zero_is_positive: the defect x >= 0 (the slope applied on the wrong side at x == 0)."""
    v, g = x.float(), dy.float()
    keep = (v >= 0) if zero_is_positive else (v > 0)
    return torch.where(keep, g, torch.tensor(slope, dtype=torch.float32) * g).to(dy.dtype)


def f32(v):
    """the fp32 value a C float argument carries (the references take the hyper-parameters the kernels read)"""
    return float(np.float32(v))


def clip_factor(sq_norm, max_norm):
    """min(1, max_norm / (sqrt(sum g^2) + 1e-6)) of clip_grad_norm_; no norm or max_norm <= 0: 1"""
    if sq_norm is None or max_norm <= 0:
        return 1.0
    return min(1.0, max_norm / (float(sq_norm) ** 0.5 + 1e-6))


def adam_ref(p, g, m, v, lr, b1, b2, eps, wd, step, sq_norm=None, max_norm=0.0):
    """One Adam (wd == 0) / AdamW step in float64; returns new (p, m, v).  step: the step the bias corrections are taken at."""
    g = g.double() * clip_factor(sq_norm, max_norm)
    m = b1 * m.double() + (1 - b1) * g
    v = b2 * v.double() + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p = p.double() * (1 - lr * wd) - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
    return p, m, v


def percentile_scale_ref(vol, lower, upper, b_min, b_max):
    """ScaleIntensityRangePercentiles on one volume: numpy's "linear" percentile stated exactly in float64 on the sorted values, the two
    percentiles and their difference rounded to fp32 as the kernel holds them, the map evaluated in float64 (tests/test_gpu_harness.py)."""
    s = np.sort(vol.reshape(-1)).astype(np.float64)
    n = s.size

    def pct(q):
        pos = (n - 1) * q / 100.0
        lo = int(np.floor(pos))
        return s[lo] + (s[min(lo + 1, n - 1)] - s[lo]) * (pos - lo)
    a_min, a_max = np.float32(pct(lower)), np.float32(pct(upper))
    d = np.float32(a_max - a_min)
    if d == 0:
        return np.full(vol.shape, b_min, dtype=np.float32)
    return ((vol.astype(np.float64) - float(a_min)) / float(d) * (b_max - b_min) + b_min).astype(np.float32)


def instance_norm_naive_f32(x, eps):
    """The one-pass formula in single precision: fp32 running sums of x and x^2 over DHW (x [N][DHW][C] fp32), var = E[x^2] - mean^2.
    Sequential fp32 accumulation (cumsum), the arithmetic a kernel without the fp64 fold would do."""
    s = torch.cumsum(x, 1)[:, -1]
    q = torch.cumsum(x * x, 1)[:, -1]
    cnt = torch.tensor(float(x.shape[1]), dtype=torch.float32)
    mean = s / cnt
    var = (q / cnt - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    return (x - mean[:, None]) * rstd[:, None]
