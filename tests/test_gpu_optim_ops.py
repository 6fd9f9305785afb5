"""Per-kernel parity of the optimizer tail and the data path (-m gpu): ldm_grad_sq_norm, ldm_adam_step, ldm_op_mse_loss and
ldm_op_scale_intensity_percentiles called directly, against float64 restatements (tests/gan_ops_ref.py) on exactly the values the kernels
read, at the sizes where their launch geometry changes: the float4 body and the scalar remainder of sq_norm_part_kernel, the grid caps
(2048 x 256 x 4, 8192 x 256, 1024 x 1024 elements) behind which the grid-stride loops run, and the skip counter the last block bumps.

Why direct calls: these entries were reached only through FlatAdam on a whole UNet, at whatever parameter count the tiny test network has.

Gates: sums (sq_norm, loss) rel 1e-6 against float64; Adam's p, m, v rel-L2 <= 1e-5 (TOL_EXACT of test_gpu_f32_ops.py) after each of three
consecutive steps; the MSE gradient and a skipped step bit-identical; the scaled volumes within 2e-6 of the exact float64 statement (the gate
of test_gpu_harness.py).  Outputs are NaN-filled before the launch, a repeat launch is bit-identical (no float atomics: the percentile
histograms are integer), and refusals are only checked for arguments the launchers reject before any launch.  Measured values are printed
(-s), quoted in the docstrings and kept in profiles/gan_ops_errors_vs_fp64.txt.
"""
import numpy as np
import pytest
import torch

import gan_ops_ref as R
from test_gpu_f32_ops import TOL_EXACT, _call, _p, _rel, _stream

pytestmark = pytest.mark.gpu
ERR_BAD_ARG = -1


def _L():
    from ldm3d import _lib
    return _lib.lib()


def _nan(shape, cuda):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=cuda)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ ldm_grad_sq_norm
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, (1 << 21) + 3])
def test_grad_sq_norm(cuda, n):
    """sq_norm_part_kernel / sq_norm_fold_kernel: n = 0 (exactly 0), below / at / past one float4, 1023 (255 float4 + 3), 2^21 + 3 (past the
    2048 x 256 x 4 elements of one grid pass, remainder 3 in block 0).  out[1] (the skip counter) is not touched.
    Measured rel error <= 9.2e-8."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn((n + 4,), generator=g)                      # the buffer is longer than n: elements behind n (large) must not be read
    x[n:] = 1e18
    ref = float((x[:n].double() ** 2).sum())
    xd = x.to(cuda)
    outs = []
    for _ in range(2):
        out = _nan((2,), cuda)
        _call("ldm_grad_sq_norm", _p(xd), n, _p(out), _stream())
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert _bits_equal(outs[0][:1], outs[1][:1]) and torch.isnan(outs[0][1]), "out[1] belongs to the caller"
    got = float(outs[0][0])
    err = abs(got - ref) / ref if n else abs(got)
    print(f"grad_sq_norm n={n}: {got:.9g} vs float64 {ref:.9g}, rel error {err:.1e} (gate 1e-6)")
    assert (got == 0.0) if n == 0 else (err <= 1e-6)


def test_grad_sq_norm_refuses_a_misaligned_buffer(cuda):
    """The float4 body needs 16-byte alignment: a pointer offset by 4 bytes is refused with LDM_ERR_BAD_ARG before any launch."""
    x = torch.zeros((64,), device=cuda)
    out = _nan((2,), cuda)
    assert x.data_ptr() % 16 == 0
    assert _L().ldm_grad_sq_norm(x.data_ptr() + 4, 8, _p(out), _stream()) == ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------ ldm_adam_step
LR, EPS = R.f32(0.05), R.f32(1e-8)      # lr 0.05 on unit-scale parameters: an update wrong by 1e-3 of itself moves p by 5e-5, outside the 1e-5 gate
ADAM = dict(b1=R.f32(0.9), b2=R.f32(0.999), wd=0.0)
ADAMW = dict(b1=R.f32(0.5), b2=R.f32(0.9), wd=R.f32(1e-2))


def _adam_launch(cuda, p, g, m, v, n, hp, step, sq, max_norm):
    _call("ldm_adam_step", _p(p), _p(g), _p(m), _p(v), n, LR, hp["b1"], hp["b2"], EPS, hp["wd"], step, _p(sq), max_norm, _stream())


@pytest.mark.parametrize("n", [1, 255, 257, (1 << 21) + 5])
@pytest.mark.parametrize("mode", ["adam_clip_binds", "adam_clip_loose", "adamw_max_norm_0", "adamw_no_norm"])
def test_adam_step_three_steps(cuda, n, mode):
    """adam_step_kernel, three consecutive steps from zero moments, against the float64 restatement of torch.optim.Adam (betas 0.9, 0.999) /
    AdamW (weight_decay 1e-2, betas 0.5, 0.9) with the hyper-parameters as the fp32 values the kernel receives: a clip that binds (max_norm =
    0.3 x the norm), one that does not (3 x), max_norm = 0 (no clip, norm still read), sq_norm = NULL.  n = 2^21 + 5 is past the 8192 x 256
    grid.  Three elements behind n stay untouched.  Measured rel-L2: p <= 4.4e-7, m <= 1.6e-7, v <= 3.0e-7."""
    hp = ADAM if mode.startswith("adam_") else ADAMW
    g = torch.Generator().manual_seed(n % 1000 + len(mode))
    p0 = torch.randn((n + 3,), generator=g)
    pd, md, vd = p0.to(cuda), torch.zeros((n + 3,), device=cuda), torch.zeros((n + 3,), device=cuda)
    md[n:], vd[n:] = 7.0, 9.0
    p, m, v = p0[:n].double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    worst = [0.0, 0.0, 0.0]
    for step in (1, 2, 3):
        gr = torch.randn((n + 3,), generator=g)
        gr[n:] = float("nan")
        sq32 = np.float32(float((gr[:n].double() ** 2).sum()))                  # the fp32 norm the kernel reads
        norm = float(sq32) ** 0.5
        max_norm = {"adam_clip_binds": R.f32(0.3 * norm), "adam_clip_loose": R.f32(3 * norm), "adamw_max_norm_0": 0.0, "adamw_no_norm": 0.0}[mode]
        sq = None if mode == "adamw_no_norm" else torch.tensor([float(sq32), 0.0], device=cuda)
        if mode == "adam_clip_binds":
            assert R.clip_factor(float(sq32), max_norm) < 0.31
        if mode == "adam_clip_loose":
            assert R.clip_factor(float(sq32), max_norm) == 1.0
        _adam_launch(cuda, pd, gr.to(cuda), md, vd, n, hp, step, sq, max_norm)
        torch.cuda.synchronize()
        p, m, v = R.adam_ref(p, gr[:n], m, v, LR, hp["b1"], hp["b2"], EPS, hp["wd"], step, None if sq is None else float(sq32), max_norm)
        for j, (got, ref, name) in enumerate(((pd, p, "p"), (md, m, "m"), (vd, v, "v"))):
            got = got.cpu()
            assert torch.isfinite(got).all()
            e = _rel(got[:n], ref)
            worst[j] = max(worst[j], e)
            assert e <= TOL_EXACT, (mode, n, step, name, e)
        if sq is not None:
            assert float(sq.cpu()[1]) == 0.0, "the skip counter moved on a good step"
    assert torch.equal(pd[n:].cpu(), p0[n:]) and float(md[n]) == 7.0 and float(vd[n + 2]) == 9.0, "wrote past n"
    print(f"adam_step {mode} n={n}: worst rel-L2 over three steps p {worst[0]:.2e}, m {worst[1]:.2e}, v {worst[2]:.2e} (gate {TOL_EXACT:.0e})")


@pytest.mark.parametrize("n", [1, 257, (1 << 21) + 5])
def test_adam_step_skip_contract(cuda, n):
    """The NaN-skip without a host read: three good AdamW steps, then a NaN and a +inf sq_norm[0]: p, m, v stay bit-identical and each call
    raises sq_norm[1] by exactly one (the last block bumps it; n = 2^21 + 5 has 8192 blocks); the sixth call is the optimizer's fourth
    step: its bias corrections are those of step - skipped = 4, gated against float64.  Control: the corrections of step 6 move p > 10x the
    gate (here and in tests/test_gan_ops_cpu.py).  Measured rel-L2 after the resumed step: p <= 2.4e-7, m <= 4.4e-8, v <= 7.5e-8;
    control 3.4e-3 ... 7.0e-3."""
    hp = ADAMW
    g = torch.Generator().manual_seed(n % 1000)
    p0 = torch.randn((n,), generator=g)
    pd, md, vd = p0.to(cuda), torch.zeros((n,), device=cuda), torch.zeros((n,), device=cuda)
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    sq = torch.zeros((2,), device=cuda)

    def good(step, eff):
        nonlocal p, m, v
        gr = torch.randn((n,), generator=g)
        sq32 = np.float32(float((gr.double() ** 2).sum()))
        max_norm = R.f32(0.5 * float(sq32) ** 0.5)
        sq[0] = float(sq32)
        _adam_launch(cuda, pd, gr.to(cuda), md, vd, n, hp, step, sq, max_norm)
        torch.cuda.synchronize()
        before = (p, m, v)
        p, m, v = R.adam_ref(p, gr, m, v, LR, hp["b1"], hp["b2"], EPS, hp["wd"], eff, float(sq32), max_norm)
        return before, gr, float(sq32), max_norm
    for step in (1, 2, 3):
        good(step, step)
    assert float(sq.cpu()[1]) == 0.0
    kept = [t.clone() for t in (pd, md, vd)]
    for k, (bad, step) in enumerate(((float("nan"), 4), (float("inf"), 5))):
        sq[0] = bad
        _adam_launch(cuda, pd, torch.randn((n,), generator=g).to(cuda), md, vd, n, hp, step, sq, 1.0)
        torch.cuda.synchronize()
        for a, b in zip((pd, md, vd), kept):
            assert _bits_equal(a, b), "a skipped step changed the state"
        assert float(sq.cpu()[1]) == k + 1.0, "each skipped step adds exactly one"
    before, gr, sq32, max_norm = good(6, 4)
    wrong = R.adam_ref(*before[:1], gr, *before[1:], LR, hp["b1"], hp["b2"], EPS, hp["wd"], 6, sq32, max_norm)[0]
    errs = [_rel(a.cpu(), b) for a, b in ((pd, p), (md, m), (vd, v))]
    ctl = _rel(wrong, p)
    print(f"adam_step skip contract n={n}: resumed step rel-L2 p {errs[0]:.2e}, m {errs[1]:.2e}, v {errs[2]:.2e} (gate {TOL_EXACT:.0e}); "
          f"bias corrections at step instead of step - skipped: {ctl:.1e}")
    assert float(sq.cpu()[1]) == 2.0
    assert max(errs) <= TOL_EXACT, errs
    assert ctl > 10 * TOL_EXACT


# ------------------------------------------------------------------------------------------------ ldm_op_mse_loss
@pytest.mark.parametrize("n", [1, 1023, (1 << 20) + 1])
def test_mse_loss(cuda, n):
    """mse_part_kernel / mse_fold_kernel: n = 2^20 + 1 is past the 1024 x 1024 elements of one grid pass.  Loss rel 1e-6 against float64;
    the gradient bit-identical to (2 / n) (p - t) evaluated in fp32; a NULL grad_out gives the same loss.  Measured rel error <= 2.5e-8."""
    g = torch.Generator().manual_seed(n)
    pr, tg = torch.randn((n + 2,), generator=g), torch.randn((n + 2,), generator=g)
    pr[n:] = 1e18                                               # behind n: must not be read
    ref = float(((pr[:n].double() - tg[:n].double()) ** 2).mean())
    gref = (torch.tensor(2.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)) * (pr[:n] - tg[:n])
    pd, td = pr.to(cuda), tg.to(cuda)
    res = []
    for with_grad in (True, True, False):
        loss, grad = _nan((1,), cuda), (_nan((n + 2,), cuda) if with_grad else None)
        _call("ldm_op_mse_loss", _p(pd), _p(td), n, _p(loss), _p(grad), _stream())
        torch.cuda.synchronize()
        res.append((loss.cpu(), None if grad is None else grad.cpu()))
    assert _bits_equal(res[0][0], res[1][0]) and _bits_equal(res[0][0], res[2][0]) and _bits_equal(res[0][1], res[1][1])
    loss, grad = res[0]
    err = abs(float(loss) - ref) / ref
    print(f"mse_loss n={n}: {float(loss):.9g} vs float64 {ref:.9g}, rel error {err:.1e} (gate 1e-6); gradient bit-identical")
    assert err <= 1e-6
    assert torch.isnan(grad[n:]).all(), "wrote past n"
    assert _bits_equal(grad[:n], gref)


# ------------------------------------------------------------------------------------------------ ldm_op_scale_intensity_percentiles
def _scale(cuda, vols, lower, upper, b_min, b_max):
    B, n = vols.shape[0], vols[0].size
    L = _L()
    xd = torch.from_numpy(np.ascontiguousarray(vols)).to(cuda)
    sb = L.ldm_op_scale_intensity_percentiles_scratch_bytes(B)
    outs = []
    for _ in range(2):
        out = _nan(tuple(vols.shape), cuda)
        scratch = torch.full((sb,), 0xFF, dtype=torch.uint8, device=cuda)       # poisoned: the entry clears what it needs
        _call("ldm_op_scale_intensity_percentiles", _p(xd), _p(out), B, n, lower, upper, b_min, b_max, _p(scratch), sb, _stream())
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.isfinite(outs[0]).all() and _bits_equal(outs[0], outs[1])
    return outs[0].numpy()


def _check_scaled(got, vols, lower, upper, b_min, b_max, what):
    worst = 0.0
    for i in range(vols.shape[0]):
        exact = R.percentile_scale_ref(vols[i], lower, upper, b_min, b_max)
        e = float(np.abs(got[i] - exact).max() / max(1.0, np.abs(exact).max()))
        worst = max(worst, e)
        assert e <= 2e-6, (what, i, e)
    print(f"scale_intensity_percentiles {what}: worst |error| / max(1, |exact|) {worst:.1e} (gate 2e-6)")


def _poisson_volume(rng, shape):
    """the low-count volume of ldm3d.data.write_synthetic_pairs: Poisson counts of a smooth field / 8 -- a few dozen distinct values, mostly 0"""
    zz, yy, xx = np.meshgrid(*[np.linspace(-1, 1, s, dtype=np.float32) for s in shape], indexing="ij")
    high = np.zeros(shape, dtype=np.float32)
    for _ in range(6):
        c, w, a = rng.uniform(-0.6, 0.6, 3), rng.uniform(0.15, 0.5), rng.uniform(0.3, 1.0)
        high += a * np.exp(-((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2) / (2 * w * w))
    return (rng.poisson(np.clip(high, 0, None) * 8.0).astype(np.float32) / 8.0).astype(np.float32)


def test_percentiles_on_heavily_tied_data(cuda):
    """Poisson counts / 8 at 37 x 41 x 29 (every radix bin of the select holds thousands of equal keys, both ranks of a percentile usually the
    same value), 0 ... 99.5 -> 0 ... 1 and 10 ... 99 -> -1 ... 1.  Measured <= 4.9e-8."""
    rng = np.random.RandomState(3)
    vols = np.stack([_poisson_volume(rng, (37, 41, 29)) for _ in range(2)])
    assert len(np.unique(vols[0])) < 64
    for args in ((0.0, 99.5, 0.0, 1.0), (10.0, 99.0, -1.0, 1.0)):
        _check_scaled(_scale(cuda, vols, *args), vols, *args, f"Poisson / 8 {args}")


def test_percentiles_of_one_and_two_values(cuda):
    """n = 1: every rank is element 0, the range is empty -> b_min.  n = 2: ranks 0 and 1, the upper percentile interpolates at 0.995."""
    one = np.array([[3.0], [-2.0]], dtype=np.float32)
    assert (_scale(cuda, one, 0.0, 99.5, 0.25, 1.0) == 0.25).all()
    two = np.array([[-1.5, 2.25], [4.0, 0.5]], dtype=np.float32)
    _check_scaled(_scale(cuda, two, 0.0, 99.5, 0.0, 1.0), two, 0.0, 99.5, 0.0, 1.0, "n = 2")


def test_percentiles_of_three_distributions_in_one_call(cuda):
    """B = 3: gamma noise, an all-negative volume (the order-preserving key inverts negative floats) and Poisson / 8 in one call, each
    scaled by its own percentiles; then lower == upper, which gives b_min everywhere.  Measured <= 1.2e-7."""
    rng = np.random.RandomState(5)
    shape = (19, 23, 17)
    vols = np.stack([rng.gamma(2.0, 1.0, size=shape).astype(np.float32), (-1.0 - rng.gamma(2.0, 1.0, size=shape)).astype(np.float32),
                     _poisson_volume(rng, shape)])
    assert vols[1].max() < 0
    for args in ((0.0, 99.5, 0.0, 1.0), (2.0, 98.0, -1.0, 3.0)):
        _check_scaled(_scale(cuda, vols, *args), vols, *args, f"B = 3 {args}")
    assert (_scale(cuda, vols, 40.0, 40.0, -2.0, 1.0) == -2.0).all()
