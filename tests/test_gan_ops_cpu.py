"""The references of tests/test_gpu_gan_ops.py and tests/test_gpu_optim_ops.py (gan_ops_ref.py) pinned where no GPU is needed: against
F.conv3d, autograd and torch.optim in float64; and the negative control of every gate those files use, on the CPU: each named defect lands
more than 10x outside its gate or breaks bit identity."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gan_ops_ref as R
from util import rup

TOL_EXACT = 1e-5        # the gate of tests/test_gpu_f32_ops.py
BF_FLOOR_X = 1.2        # the bf16 gate of tests/test_gpu_bf16_train_ops.py

GEOMETRIES = R.GEOMETRIES


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _x(N, dims, Cs, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((N, *dims, Cs), generator=g, dtype=dtype)


@pytest.mark.parametrize("k,stride,pad,dims", GEOMETRIES)
@pytest.mark.parametrize("N,C,Cs", [(1, 1, 16), (2, 2, 32), (1, 24, 32), (2, 16, 16)])
def test_im2col_then_matmul_is_conv3d(k, stride, pad, dims, N, C, Cs):
    """float64 im2col followed by a matmul with the MONAI-layout weight reshaped as discriminator.py does it == F.conv3d in float64;
    enumerating the taps (kw, kh, kd) is > 10x outside the 1e-5 gate (k > 1); the Kp tail is exactly zero."""
    g = torch.Generator().manual_seed(k * 100 + stride * 10 + pad + N + C)
    x = _x(N, dims, Cs, 7 + k + C)
    x[..., C:] = float("nan")                                   # channels C .. Cs are never read
    cout = 5
    w = torch.randn((cout, C, k, k, k), generator=g, dtype=torch.float64)
    Kp = rup(k ** 3 * C, 16) + 16
    col = R.im2col_ref(x, C, k, stride, pad, Kp)
    assert torch.equal(col[:, k ** 3 * C:], torch.zeros_like(col[:, k ** 3 * C:]))
    y = col @ R.weight_matrix(w, Kp).t()
    ref = F.conv3d(x[..., :C].permute(0, 4, 1, 2, 3), w, None, stride=stride, padding=pad).permute(0, 2, 3, 4, 1).reshape(-1, cout)
    assert _rel(y, ref) < 1e-13
    if k > 1:
        bad = R.im2col_ref(x, C, k, stride, pad, Kp, order="whd") @ R.weight_matrix(w, Kp).t()
        assert _rel(bad, ref) > 10 * TOL_EXACT
        assert not torch.equal(R.im2col_ref(x, C, k, stride, pad, Kp, order="whd"), col)
    # the Kp tail left unwritten: bit identity with the reference breaks
    assert not torch.equal(R.im2col_ref(x, C, k, stride, pad, Kp, tail=float("nan")), col)


@pytest.mark.parametrize("k,stride,pad,dims", GEOMETRIES)
@pytest.mark.parametrize("N,C,Cs", [(1, 1, 16), (2, 2, 32), (1, 24, 32)])
def test_col2im_is_the_autograd_adjoint(k, stride, pad, dims, N, C, Cs):
    """col2im_ref == d/dx of sum(im2col(x) * dcol) by autograd; dropping the last output plane's contributions is > 10x outside both the
    1e-5 gate and the bf16 gate (1.2 x the bf16 rounding floor of the reference, ~2e-3) and breaks bit identity on integer inputs."""
    g = torch.Generator().manual_seed(k + stride + pad + N + C)
    Kp = rup(k ** 3 * C, 16)
    Do, Ho, Wo = R.out_dims(dims, k, stride, pad)
    dcol = torch.randn((N * Do * Ho * Wo, Kp), generator=g, dtype=torch.float64)
    x = torch.zeros((N, *dims, Cs), dtype=torch.float64, requires_grad=True)
    (R.im2col_ref(x, C, k, stride, pad, Kp) * dcol).sum().backward()
    poisoned = dcol.clone()
    poisoned[:, k ** 3 * C:] = float("nan")                     # the tail of dcol is never read
    got = R.col2im_ref(poisoned, N, dims, Cs, C, k, stride, pad)
    assert torch.equal(got[..., C:], torch.zeros_like(got[..., C:]))
    assert _rel(got, x.grad) < 1e-13
    bad = R.col2im_ref(dcol, N, dims, Cs, C, k, stride, pad, drop_last_plane=True)
    floor = _rel(got.to(torch.bfloat16), got)
    assert _rel(bad, got) > 10 * max(TOL_EXACT, BF_FLOOR_X * floor)
    ints = torch.randint(-3, 4, dcol.shape, generator=g).double()
    exact = R.col2im_ref(ints, N, dims, Cs, C, k, stride, pad)
    assert float(exact.abs().max()) <= 256 and torch.equal(exact.to(torch.bfloat16).double(), exact)   # exact in bf16 and fp32
    assert not torch.equal(R.col2im_ref(ints, N, dims, Cs, C, k, stride, pad, drop_last_plane=True), exact)


@pytest.mark.parametrize("M,ksplit", [(1, 3), (15, 16), (17, 3), (100, 64), (4097, 16), (4097, 64)])
def test_wgrad_slabs_sum_to_the_product_and_empty_splits_are_zero(M, ksplit):
    g = torch.Generator().manual_seed(M + ksplit)
    dy, x = torch.randn((M, 48), generator=g), torch.randn((M, 80), generator=g)
    slabs = R.wgrad_slabs_ref(dy, x, 33, ksplit)
    assert _rel(slabs.sum(0), dy[:, :33].double().t() @ x.double()) < 1e-13
    rows = R.wgrad_split_rows(M, ksplit)
    assert rows[0][0] == 0 and max(r1 for _, r1 in rows) == M and all(a[1] == b[0] or b[0] == M for a, b in zip(rows, rows[1:]))
    empty = [s for s, (r0, r1) in enumerate(rows) if r0 == r1]
    steps = (M + 15) // 16                                       # ceil(steps / ksplit) steps per split: the rounding alone can leave splits empty
    assert len(empty) == ksplit - -(-steps // -(-steps // ksplit)) and (ksplit <= steps or empty)
    for s in empty:
        assert torch.equal(slabs[s], torch.zeros_like(slabs[s]))
    if empty:                                                    # an empty split left unwritten: the finite check and the zero check see it
        bad = R.wgrad_slabs_ref(dy, x, 33, ksplit, empty=float("nan"))
        assert not torch.isfinite(bad).all() and not torch.equal(bad[empty[0]], torch.zeros_like(bad[empty[0]]))


def test_leaky_relu_references_and_the_zero_side_defect():
    x = torch.tensor([0.0, -0.0, 1.5, -1.5, -2.0 ** -133, 3.0, -7.25])
    dy = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, -6.0, 7.0])
    for dt in (torch.float32, torch.bfloat16):
        xx, dd = x.to(dt), dy.to(dt)
        y = R.leaky_ref(xx, 0.2)
        assert torch.equal(y.float(), F.leaky_relu(xx.float(), 0.2).to(dt).float())
        assert torch.equal(y.view(torch.int16 if dt == torch.bfloat16 else torch.int32)[:2] < 0, torch.tensor([False, True]))   # +0 -> +0, -0 -> -0
        xr = xx.float().clone().requires_grad_(True)
        F.leaky_relu(xr, 0.2).backward(dd.float())
        nz = xx.float() != 0                                     # torch's own derivative at 0 is the slope as well; compared away from it
        assert torch.equal(R.leaky_bwd_ref(xx, dd, 0.2).float()[nz], xr.grad.to(dt).float()[nz])
        assert torch.equal(R.leaky_bwd_ref(xx, dd, 0.2).float()[:2], (torch.tensor(0.2) * dd.float()[:2]).to(dt).float())
        assert not torch.equal(R.leaky_bwd_ref(xx, dd, 0.2, zero_is_positive=True), R.leaky_bwd_ref(xx, dd, 0.2))
    assert float(R.leaky_ref(torch.tensor([-2.0 ** -133]).to(torch.bfloat16), 0.2)) == 0.0   # 0.2 of the smallest bf16 subnormal rounds to -0


@pytest.mark.parametrize("decoupled,betas,wd", [(False, (0.9, 0.999), 0.0), (True, (0.5, 0.9), 1e-2)])
@pytest.mark.parametrize("max_norm", [0.0, 0.5, 1e3])
def test_adam_restatement_is_torch_optim(decoupled, betas, wd, max_norm):
    """adam_ref, three steps, against torch.optim.Adam / AdamW + clip_grad_norm_ in float64 (max_norm 0.5 binds, 1e3 does not, 0: no clip)."""
    g = torch.Generator().manual_seed(3)
    n, lr, eps = 257, R.f32(0.05), R.f32(1e-8)
    b1, b2, wd = R.f32(betas[0]), R.f32(betas[1]), R.f32(wd)
    p0 = torch.randn((n,), generator=g, dtype=torch.float64)
    pt = p0.clone().requires_grad_(True)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0, torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in (1, 2, 3):
        gr = torch.randn((n,), generator=g, dtype=torch.float64)
        pt.grad = gr.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([pt], max_norm)
        opt.step()
        p, m, v = R.adam_ref(p, gr, m, v, lr, b1, b2, eps, wd, step, float((gr * gr).sum()), max_norm)
        assert _rel(p, pt.detach()) < 1e-12
        st = opt.state[pt]
        assert _rel(m, st["exp_avg"]) < 1e-12 and _rel(v, st["exp_avg_sq"]) < 1e-12
    assert R.clip_factor(float((gr * gr).sum()), 0.5) < 1 and R.clip_factor(float((gr * gr).sum()), 1e3) == 1.0


def test_bias_correction_at_step_instead_of_step_minus_skipped_is_seen():
    """The skip contract's control: after two skipped calls the sixth call is the optimizer's fourth step; taking the bias corrections at 6
    moves p more than 10x the 1e-5 gate (lr 0.05 on unit-scale parameters, the setting of the GPU test)."""
    g = torch.Generator().manual_seed(5)
    n, lr, eps, b1, b2, wd = 1023, R.f32(0.05), R.f32(1e-8), R.f32(0.5), R.f32(0.9), R.f32(1e-2)
    p, m, v = torch.randn((n,), generator=g, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in (1, 2, 3):
        p, m, v = R.adam_ref(p, torch.randn((n,), generator=g, dtype=torch.float64), m, v, lr, b1, b2, eps, wd, step)
    gr = torch.randn((n,), generator=g, dtype=torch.float64)
    good = R.adam_ref(p, gr, m, v, lr, b1, b2, eps, wd, 4)
    bad = R.adam_ref(p, gr, m, v, lr, b1, b2, eps, wd, 6)
    assert _rel(bad[0], good[0]) > 10 * TOL_EXACT
    assert torch.equal(bad[1], good[1]) and torch.equal(bad[2], good[2])      # the moments do not depend on it: p carries the control


def test_percentile_reference_is_numpy_percentile():
    rng = np.random.RandomState(0)
    for vol in (rng.gamma(2.0, 1.0, size=(7, 9, 5)).astype(np.float32), (rng.poisson(0.7, size=(6, 5, 4)) / 8).astype(np.float32),
                -1 - rng.gamma(2.0, 1.0, size=(5, 5, 5)).astype(np.float32), np.array([-1.5, 2.25], dtype=np.float32)):
        for lo, hi, b0, b1 in ((0.0, 99.5, 0.0, 1.0), (5.0, 50.0, -1.0, 1.0)):
            a_min, a_max = np.percentile(vol.astype(np.float64), lo), np.percentile(vol.astype(np.float64), hi)
            if a_max - a_min == 0:
                continue
            ref = (vol.astype(np.float64) - a_min) / (a_max - a_min) * (b1 - b0) + b0
            got = R.percentile_scale_ref(vol, lo, hi, b0, b1)
            assert np.abs(got - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max())
    one = np.array([3.0], dtype=np.float32)
    assert R.percentile_scale_ref(one, 0.0, 99.5, 0.25, 1.0)[0] == 0.25          # constant volume -> b_min
    assert (R.percentile_scale_ref(vol, 40.0, 40.0, -2.0, 1.0) == -2.0).all()   # lower == upper -> b_min everywhere


def test_naive_instance_norm_loses_the_variance_as_the_mean_grows():
    """The yardstick of the cancellation test: the one-pass fp32 formula is fine at mean / std = 0 and loses digits as the ratio grows."""
    g = torch.Generator().manual_seed(1)
    z = torch.randn((2, 210, 64), generator=g, dtype=torch.float64)
    errs = []
    for ratio in (0.0, 32.0, 256.0):
        x = (ratio + z).float()
        ref = F.group_norm(x.double().permute(0, 2, 1), 64, None, None, 1e-5).permute(0, 2, 1)
        errs.append(_rel(R.instance_norm_naive_f32(x, 1e-5), ref))
    assert errs[0] < 1e-6 and errs[0] < errs[1] < errs[2] and errs[2] > 1e-4
