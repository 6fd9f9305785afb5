"""Per-kernel parity of the stage-1 GAN tail (-m gpu): every building block of ldm3d/discriminator.py, bf16 and fp32 form, called through its
ldm_op_* entry, against plain torch on the CPU in float64 (tests/gan_ops_ref.py) on exactly the values the kernel reads.

Why operator level: tests/test_gpu_gan.py gates whole layers at 2e-3 ... 6e-3 (bf16) and the whole fp32 network at 1e-3, at k = 4, pad = 1 and
even extents only; a kernel wrong by 1e-4 of one tensor, or wrong only where stride 2 meets an odd extent, passes there.

Gates (those of test_gpu_f32_ops.py and test_gpu_bf16_train_ops.py, imported, not restated):
  data movement (im2col, pack, unpack, leaky_relu(_bwd), col2im on exactly summable inputs): bit-identical to the reference, signed zeros and
  round-to-nearest-even included;
  fp32 arithmetic (gemm_f32, gemm_wgrad_f32, group_norm_f32, group_norm_bwd_f32, col2im_f32 on random inputs): rel-L2 <= 1e-5, worst row <= 1e-4;
  bf16 outputs (col2im, group_norm, group_norm_bwd dx): rel-L2 <= 1.2 x the bf16 rounding floor of the reference and no element more than
  one bf16 ulp off.
Every case NaN-fills outputs and scratch (and the parts of the inputs the kernel must not read: channels C .. Cs, the Kp tail of dcol),
requires finite outputs with the documented padding exactly zero and a bit-identical second launch, and carries a negative control: the
same operation on bf16-rounded operands, or one named defect, more than 10x outside the gate.  Measured values are printed (-s), quoted in
the docstrings and kept in profiles/gan_ops_errors_vs_fp64.txt.
"""
import pytest
import torch
import torch.nn.functional as F

import gan_ops_ref as R
from test_gpu_bf16_train_ops import _gate32, _gate_bf
from test_gpu_f32_ops import TOL_EXACT, _bf, _call, _gate, _p, _rel, _stream
from util import rup

pytestmark = pytest.mark.gpu

# form -> (dtype, entry suffix, multiple of Kp / stored channels, (C, Cs) cases)
FORMS = {
    "bf16": (torch.bfloat16, "", 32, [(1, 32), (2, 32), (32, 32), (40, 64)]),
    "f32": (torch.float32, "_f32", 16, [(1, 16), (2, 16), (16, 16), (24, 32)]),
}


def _L():
    from ldm3d import _lib
    return _lib.lib()


def _nan(shape, cuda, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=cuda)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _twice(launch):
    """launch() -> tuple of NaN-filled-then-written device tensors; two launches, bit-identical and finite; returns the first on the CPU."""
    a, b = launch(), launch()
    torch.cuda.synchronize()
    a, b = [t.cpu() for t in a], [t.cpu() for t in b]
    for u, v in zip(a, b):
        assert torch.isfinite(u.float()).all(), "an output element was left unwritten or is not finite"
        assert _same_bits(u, v), "second launch differs"
    return a


def _randn(shape, g, dtype):
    x = torch.randn(shape, generator=g).to(dtype)
    x.view(-1)[::5] = -0.0                                      # signed zeros travel as bits
    x.view(-1)[1::11] = 0.0
    return x


# ------------------------------------------------------------------------------------------------ im2col / col2im
@pytest.mark.parametrize("form", ["bf16", "f32"])
@pytest.mark.parametrize("k,stride,pad,dims", R.GEOMETRIES)
def test_im2col_is_bit_identical(cuda, form, k, stride, pad, dims):
    """im2col_generic_kernel<bf16_t | float> at every geometry, N in {1, 2}, C < Cs and C == Cs, Kp = the next multiple of 32 | 16 above k^3 C:
    bit-identical to plain indexing; the zero tail and the padding taps are +0; channels C .. Cs of x (NaN here) are never read."""
    dt, sfx, mul, chans = FORMS[form]
    for N in (1, 2):
        for C, Cs in chans:
            g = torch.Generator().manual_seed(k * 1000 + stride * 100 + pad * 10 + N + C)
            x = _randn((N, *dims, Cs), g, dt)
            x[..., C:] = float("nan")
            Kp = rup(k ** 3 * C, mul)
            ref = R.im2col_ref(x, C, k, stride, pad, Kp)
            xd = x.to(cuda)

            def launch():
                col = _nan(ref.shape, cuda, dt)
                _call("ldm_op_im2col" + sfx, _p(xd), _p(col), N, *dims, Cs, C, k, stride, pad, Kp, _stream())
                return (col,)
            (col,) = _twice(launch)
            assert _same_bits(col, ref), (form, N, C, Cs)
    print(f"im2col{sfx} k{k} s{stride} p{pad} {dims}: bit-identical (N 1, 2; {chans})")


@pytest.mark.parametrize("form", ["bf16", "f32"])
def test_im2col_wide_zero_tail(cuda, form):
    """Kp three further multiples above k^3 C (C = 2, k = 3: 54 real columns of 160 | 112): a zero tail wider than one vector, exactly +0."""
    dt, sfx, mul, _ = FORMS[form]
    g = torch.Generator().manual_seed(11)
    N, dims, C, Cs, k, stride, pad = 2, (5, 6, 7), 2, mul, 3, 2, 1
    x = _randn((N, *dims, Cs), g, dt)
    x[..., C:] = float("nan")
    Kp = rup(k ** 3 * C, mul) + 3 * mul
    ref = R.im2col_ref(x, C, k, stride, pad, Kp)
    xd = x.to(cuda)

    def launch():
        col = _nan(ref.shape, cuda, dt)
        _call("ldm_op_im2col" + sfx, _p(xd), _p(col), N, *dims, Cs, C, k, stride, pad, Kp, _stream())
        return (col,)
    (col,) = _twice(launch)
    assert _same_bits(col, ref)
    assert int((_bits(col[:, k ** 3 * C:]) != 0).sum()) == 0
    # its adjoint reads none of the tail
    dcol = _randn(ref.shape, g, dt)
    dcol[:, k ** 3 * C:] = float("nan")
    dref = R.col2im_ref(dcol, N, dims, Cs, C, k, stride, pad)
    dd = dcol.to(cuda)

    def launch2():
        dx = _nan((N, *dims, Cs), cuda, dt)
        _call("ldm_op_col2im" + sfx, _p(dd), _p(dx), N, *dims, Cs, C, k, stride, pad, Kp, _stream())
        return (dx,)
    (dx,) = _twice(launch2)
    assert int((_bits(dx[..., C:]) != 0).sum()) == 0
    (_gate_bf if form == "bf16" else _gate32)(dx.reshape(N, *dims[:2], -1), dref.reshape(N, *dims[:2], -1), f"col2im{sfx} wide tail Kp={Kp}")


@pytest.mark.parametrize("form", ["bf16", "f32"])
@pytest.mark.parametrize("k,stride,pad,dims", R.GEOMETRIES)
def test_col2im_against_the_fp64_adjoint(cuda, form, k, stride, pad, dims):
    """col2im_generic_kernel<bf16_t | float>: on small integers (|sum| <= 192: exact in bf16 and fp32) bit-identical to the float64 adjoint; on
    random inputs the bf16 form within 1.2 x the bf16 floor and one ulp, the fp32 form within 1e-5.  Control: the contributions of the last
    output plane dropped (an od >= Do guard off by one).  Channels C .. Cs exactly zero; the Kp tail of dcol (NaN) is never read.
    Measured: bf16 1.000 x floor, worst 0.50 ulp (control 0.55 ... 0.98); fp32 rel-L2 <= 1.2e-7, worst W line <= 3.3e-7."""
    dt, sfx, mul, chans = FORMS[form]
    worst = 0.0
    for N in (1, 2):
        for C, Cs in chans:
            g = torch.Generator().manual_seed(k * 1000 + stride * 100 + pad * 10 + N + C + 1)
            Kp = rup(k ** 3 * C, mul)
            Do, Ho, Wo = R.out_dims(dims, k, stride, pad)
            M = N * Do * Ho * Wo
            ints = torch.randint(-3, 4, (M, Kp), generator=g).to(dt)
            rnd = torch.randn((M, Kp), generator=g).to(dt)
            for name, dcol in (("integers", ints), ("random", rnd)):
                dcol[:, k ** 3 * C:] = float("nan")
                ref = R.col2im_ref(dcol, N, dims, Cs, C, k, stride, pad)
                bad = R.col2im_ref(dcol, N, dims, Cs, C, k, stride, pad, drop_last_plane=True)
                dd = dcol.to(cuda)

                def launch():
                    dx = _nan((N, *dims, Cs), cuda, dt)
                    _call("ldm_op_col2im" + sfx, _p(dd), _p(dx), N, *dims, Cs, C, k, stride, pad, Kp, _stream())
                    return (dx,)
                (dx,) = _twice(launch)
                assert int((_bits(dx[..., C:]) != 0).sum()) == 0, "channels C .. Cs must be exactly zero"
                what = f"col2im{sfx} k{k} s{stride} p{pad} {dims} N={N} C={C}/{Cs} {name}"
                # a row of the worst-row gate = one W line of voxels: a single element (C = 1) that sums 64 terms of either sign to ~0
                # has no relative accuracy in any fp32 summation order
                line = lambda t: t[..., :C].reshape(N, *dims[:2], dims[2] * C)
                if name == "integers" or _rel(ref.to(dt), ref) == 0.0:          # k = 1: one term per voxel, the reference is exact in dt
                    assert torch.equal(dx.double(), ref), what
                    assert not torch.equal(bad, ref)
                elif form == "bf16":
                    e = _gate_bf(line(dx), line(ref), what, line(bad), "last output plane dropped")
                    worst = max(worst, e / _rel(ref[..., :C].to(dt), ref[..., :C]))
                else:
                    worst = max(worst, _gate32(line(dx), line(ref), what, line(bad), "last output plane dropped"))
    print(f"col2im{sfx} k{k} s{stride} p{pad} {dims}: integers bit-identical; random worst {'x floor' if form == 'bf16' else 'rel-L2'} {worst:.3e}")


# ------------------------------------------------------------------------------------------------ pack / unpack / LeakyReLU
@pytest.mark.parametrize("form", ["bf16", "f32"])
def test_pack_and_unpack_are_bit_identical(cuda, form):
    """pack2_ncdhw(_f32)_kernel (fp32 NCDHW -> NDHWC with channels zero-padded to Cs; the bf16 form rounds to nearest even) and
    unpack_ndhwc_kernel<bf16_t | float> (first C channels back to fp32 NCDHW; channels C .. Cs, NaN here, never read), N in {1, 2},
    DHW in {1, 210, 4097}: bit-identical."""
    dt, sfx, mul, chans = FORMS[form]
    for N in (1, 2):
        for C, Cs in chans:
            for DHW in (1, 210, 4097):
                g = torch.Generator().manual_seed(N * 10000 + C * 100 + DHW)
                x = _randn((N, C, DHW), g, torch.float32)
                x.view(-1)[2::13] = 1.00390625                  # 1 + 2^-8: a bf16 tie, rounds to even (1.0)
                ref = torch.zeros((N, DHW, Cs), dtype=dt)
                ref[..., :C] = x.permute(0, 2, 1).to(dt)
                xd = x.to(cuda)

                def launch():
                    out = _nan((N, DHW, Cs), cuda, dt)
                    _call("ldm_op_pack_ncdhw" + sfx, _p(xd), _p(out), N, C, Cs, DHW, _stream())
                    return (out,)
                (out,) = _twice(launch)
                assert _same_bits(out, ref), ("pack", form, N, C, Cs, DHW)
                a = _randn((N, DHW, Cs), g, dt)
                a[..., C:] = float("nan")
                uref = a[..., :C].float().permute(0, 2, 1).contiguous()
                ad = a.to(cuda)

                def launch2():
                    out = _nan((N, C, DHW), cuda)
                    _call("ldm_op_unpack_ndhwc" + sfx, _p(ad), _p(out), N, C, Cs, DHW, _stream())
                    return (out,)
                (out,) = _twice(launch2)
                assert _same_bits(out, uref), ("unpack", form, N, C, Cs, DHW)
    print(f"pack_ncdhw{sfx} / unpack_ndhwc{sfx}: bit-identical")


@pytest.mark.parametrize("form", ["bf16", "f32"])
@pytest.mark.parametrize("n", [0, 1, 255, 257, (1 << 21) + 5])
def test_leaky_relu_and_its_backward_are_bit_identical(cuda, form, n):
    """leaky_relu_kernel / leaky_relu_bwd_kernel<bf16_t | float>: the fp32 expression v > 0 ? v : slope * v (x > 0 ? dy : slope * dy), stored
    round-to-nearest-even, bit for bit; inputs hold +0, -0 (-0 -> -0; the backward takes the slope side at both zeros) and the smallest bf16
    subnormal (0.2 of it rounds to zero in bf16).  n = 2^21 + 5 is past the 8192 x 256 grid, so the grid-stride loop runs; three elements
    behind n stay NaN.  Control (CPU): x >= 0 in the backward breaks bit identity."""
    dt, sfx, _, _ = FORMS[form]
    g = torch.Generator().manual_seed(n + 1)
    x = torch.randn((n + 3,), generator=g).to(dt)
    dy = torch.randn((n + 3,), generator=g).to(dt)
    special = torch.tensor([0.0, -0.0, -2.0 ** -133, 2.0 ** -133, -1.0], dtype=torch.float32).to(dt)
    for off in (0, 250, n - 5):
        if 0 <= off and off + 5 <= n:
            x[off:off + 5] = special
    slope = 0.2
    yref, dref = R.leaky_ref(x[:n], slope), R.leaky_bwd_ref(x[:n], dy[:n], slope)
    xd, dyd = x.to(cuda), dy.to(cuda)
    y, dx = _nan((n + 3,), cuda, dt), _nan((n + 3,), cuda, dt)
    y2, dx2 = _nan((n + 3,), cuda, dt), _nan((n + 3,), cuda, dt)
    for a, b in ((y, dx), (y2, dx2)):
        _call("ldm_op_leaky_relu" + sfx, _p(xd), _p(a), n, slope, _stream())
        _call("ldm_op_leaky_relu_bwd" + sfx, _p(xd), _p(dyd), _p(b), n, slope, _stream())
    torch.cuda.synchronize()
    assert _same_bits(y, y2) and _same_bits(dx, dx2)
    assert torch.isnan(y[n:].float()).all() and torch.isnan(dx[n:].float()).all(), "wrote past n"
    assert _same_bits(y[:n], yref) and _same_bits(dx[:n], dref)
    if n >= 5:
        assert not _same_bits(R.leaky_bwd_ref(x[:n], dy[:n], slope, zero_is_positive=True), dref)
    print(f"leaky_relu{sfx} / leaky_relu_bwd{sfx} n={n}: bit-identical")


# ------------------------------------------------------------------------------------------------ exact-fp32 GEMMs
def _well_conditioned_rows(x, w, bias, g):
    """Redraw the rows of x whose float64 output row is short (< 1/4 of the median row norm): the worst-row gate divides by the row's own
    norm, and a row of one or a few columns that cancels to ~0 has no relative accuracy in ANY fp32 summation.  Asserted before the launch."""
    for _ in range(50):
        ref = x.double() @ w.double().t() + (bias.double() if bias is not None else 0)
        rn = ref.norm(dim=1)
        short = rn < 0.25 * rn.median()
        if not short.any():
            return ref
        x[short] = torch.randn((int(short.sum()), x.shape[1]), generator=g)
    raise AssertionError("could not condition the rows")


def _gemm_case(cuda, M, K, cout, cout_pad, couts, bias, seed, what):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((M, K), generator=g)
    w = torch.zeros((cout_pad, K))
    w[:cout] = torch.randn((cout, K), generator=g) / K ** 0.5
    b = None
    if bias:
        b = torch.zeros((cout_pad,))
        b[:cout] = 0.1 * torch.randn((cout,), generator=g)
    ref = _well_conditioned_rows(x, w[:cout], b[:cout] if bias else None, g)
    ref_bf = _bf(x) @ _bf(w[:cout]).t() + (b[:cout].double() if bias else 0)
    xd, wd, bd = x.to(cuda), w.to(cuda), (b.to(cuda) if bias else None)

    def launch():
        out = _nan((M, couts), cuda)
        _call("ldm_op_gemm_f32", _p(xd), K, _p(wd), _p(bd), _p(out), M, cout, cout_pad, couts, _stream())
        return (out,)
    (out,) = _twice(launch)
    assert int((_bits(out[:, cout:]) != 0).sum()) == 0, "columns cout .. couts must be exactly zero"
    return _gate(out[:, :cout], ref, TOL_EXACT, what, ref_bf)


@pytest.mark.parametrize("cout,cout_pad,couts", [(1, 64, 16), (33, 64, 48), (64, 64, 64), (130, 192, 132), (256, 256, 256)])
@pytest.mark.parametrize("bias", [True, False])
def test_gemm_f32(cuda, cout, cout_pad, couts, bias):
    """ldm_op_gemm_f32 (conv_f32_kernel<64 | 128> as a 1x1 GEMM): M in {1, 127, 129, 300} (one row; one short of, one past a 128-row tile;
    three tiles, the last ragged) x K in {16, 80, 1024}; the one-channel final conv (1, 64, 16), ragged stored columns, 64- and 128-wide
    tiles; bias and NULL.  Columns cout .. couts exactly zero.  Rows of x whose float64 output row is short are redrawn first
    (_well_conditioned_rows).  Measured rel-L2 <= 6.2e-7, worst row <= 5.6e-6; bf16 operands >= 4e-4 (M = 1), typically 2e-3."""
    worst = 0.0
    for M in (1, 127, 129, 300):
        for K in (16, 80, 1024):
            worst = max(worst, _gemm_case(cuda, M, K, cout, cout_pad, couts, bias, M * 7 + K + cout + bias,
                                          f"gemm_f32 M={M} K={K} cout={cout}/{couts}/{cout_pad}{' bias' if bias else ''}"))
    print(f"gemm_f32 ({cout}, {cout_pad}, {couts}){' bias' if bias else ''}: worst rel-L2 {worst:.2e}")


@pytest.mark.parametrize("M,K,Kp", [(129, 48, 80), (300, 16, 1040), (127, 64, 2048)])
def test_gemm_f32_as_the_data_gradient(cuda, M, K, Kp):
    """The dgrad use of discriminator.py: dcol[M][Kp] = dy[M][couts] wt[rup64(Kp)][couts]^T, cout = couts = Kp, cout_pad = rup(Kp, 64), no bias
    (Kp = 1040: 17 tiles of 64, the last holding 16 real rows; 2048: 128-wide tiles).  Measured rel-L2 <= 1.5e-7, worst row <= 2.0e-7."""
    _gemm_case(cuda, M, K, Kp, rup(Kp, 64), Kp, False, M + K + Kp, f"gemm_f32 dgrad M={M} couts={K} Kp={Kp}")


@pytest.mark.parametrize("cout,cdy", [(1, 16), (32, 32), (130, 144)])
@pytest.mark.parametrize("K", [16, 144, 272])
def test_gemm_wgrad_f32(cuda, cout, cdy, K):
    """ldm_op_gemm_wgrad_f32 (wgrad_f32_kernel with ksize 1): M in {1, 15, 17, 100, 4097} (no multiple of the 16-row step but 4096 + 1) x
    ksplit in {1, 3, 16, 64}; the sum of the slabs against float64, every slab against the float64 product of its own row range, and the
    slabs of empty splits (more splits than 16-row steps, or left over by the rounding of steps per split) exactly zero.  cdy >= cout:
    the columns cout .. cdy of dy are never part of dW.  Measured: sums and single slabs rel-L2 <= 1.5e-6, worst row <= 2.3e-6; bf16 operands >= 1.3e-3."""
    worst = worst_slab = 0.0
    for M in (1, 15, 17, 100, 4097):
        g = torch.Generator().manual_seed(M + cout + K)
        dy, x = torch.randn((M, cdy), generator=g), torch.randn((M, K), generator=g)
        dyd, xd = dy.to(cuda), x.to(cuda)
        total = dy[:, :cout].double().t() @ x.double()
        total_bf = _bf(dy[:, :cout]).t() @ _bf(x)
        for ksplit in (1, 3, 16, 64):
            ref = R.wgrad_slabs_ref(dy, x, cout, ksplit)

            def launch():
                dw = _nan((ksplit, cout, K), cuda)
                _call("ldm_op_gemm_wgrad_f32", _p(dyd), cdy, _p(xd), K, _p(dw), cout, M, ksplit, _stream())
                return (dw,)
            (dw,) = _twice(launch)
            what = f"gemm_wgrad_f32 M={M} K={K} cout={cout}/{cdy} ksplit={ksplit}"
            n_empty = 0
            for s, (r0, r1) in enumerate(R.wgrad_split_rows(M, ksplit)):
                if r0 == r1:
                    n_empty += 1
                    assert int((_bits(dw[s]) != 0).sum()) == 0, (what, "an empty split must leave a zero slab", s)
                else:
                    e = _rel(dw[s], ref[s])
                    worst_slab = max(worst_slab, e)
                    assert e <= TOL_EXACT, (what, "slab", s, e)
            assert (n_empty > 0) or ksplit <= (M + 15) // 16
            worst = max(worst, _gate(dw.double().sum(0), total, TOL_EXACT, what + f" ({n_empty} empty)", total_bf))
    print(f"gemm_wgrad_f32 cout={cout}/{cdy} K={K}: worst rel-L2 of the sums {worst:.2e}, of single slabs {worst_slab:.2e}")


# ------------------------------------------------------------------------------------------------ GroupNorm / InstanceNorm (+ act)
def _act(u, act):
    return F.silu(u) if act == 1 else (F.leaky_relu(u, 0.2) if act == 2 else u)


def _gn_inputs(N, C, groups, DHW, act, eps, dt, seed, affine=True, dy_corr=0.0):
    """x [N][C][DHW] of dtype dt (as float64), built per (sample, group) as mean + std * (exactly standardised noise) with std in [0.5, 2]
    and |mean| <= std: the one-pass variance E[x^2] - mean^2 has condition number 1 + (mean / std)^2 <= 2 here, the growth with
    mean / std is test_instance_norm_cancellation's subject.  act 2: no normalised value within 1e-3 of the kink (offenders moved, re-checked,
    asserted), so that no element needs an exemption.  dy_corr: dy = noise + dy_corr * x, so that the group-mean terms of dx matter."""
    g = torch.Generator().manual_seed(seed)
    cpg = C // groups
    z = torch.randn((N, groups, cpg * DHW), generator=g, dtype=torch.float64)
    z = (z - z.mean(2, keepdim=True)) / z.var(2, unbiased=False, keepdim=True).sqrt()
    std = 0.5 + 1.5 * torch.rand((N, groups, 1), generator=g, dtype=torch.float64)
    mean = (2 * torch.rand((N, groups, 1), generator=g, dtype=torch.float64) - 1) * std
    x = (mean + std * z).reshape(N, C, DHW).to(dt).double()
    if affine:
        gamma = (1 + 0.2 * torch.randn((C,), generator=g)).float()
        beta = (0.2 * torch.randn((C,), generator=g)).float()
    else:
        gamma, beta = torch.ones((C,)), torch.zeros((C,))
    noise = torch.randn((N, C, DHW), generator=g)
    if act == 2:
        for _ in range(40):
            u = F.group_norm(x, groups, gamma.double(), beta.double(), eps)
            near = u.abs() < 2e-3
            if not near.any():
                break
            x = torch.where(near, x + 0.05, x).to(dt).double()
        u = F.group_norm(x, groups, gamma.double(), beta.double(), eps)
        assert float(u.abs().min()) >= 1e-3, "a normalised value sits on the LeakyReLU kink"
    dy = (noise.double() + dy_corr * x).to(dt).double()
    return x, gamma, beta, dy


def _gn_refs(x, gamma, beta, dy, groups, eps, act):
    xx, gm, bt = x.clone().requires_grad_(True), gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    y = _act(F.group_norm(xx, groups, gm, bt, eps), act)
    y.backward(dy)
    return y.detach(), xx.grad, gm.grad, bt.grad


def _cl(t):
    """[N][C][DHW] -> [N * DHW][C]"""
    return t.permute(0, 2, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("C,groups", [(4, 4), (32, 32), (64, 64), (260, 260), (64, 8), (1024, 32)])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("DHW", [2, 27, 210])
def test_group_norm_f32_and_backward(cuda, C, groups, act, DHW):
    """ldm_op_group_norm_f32 (gn_stats_f32 / gn_finalize / gn_apply_f32) and ldm_op_group_norm_bwd_f32 (+ gnb32_stats / gn_bwd_finalize /
    gnb32_apply / rowsum_n), N in {1, 3}: y, dx, dgamma, dbeta against float64 autograd.  InstanceNorm (groups == C: one channel per group;
    C = 4: one float4 column; 260: 65 columns, no divisor of 256), GroupNorm with 8 and 32 channels per group; DHW 2 (fewer rows than row
    lanes), 27, 210 (several slabs).  eps = 1e-5, except where a group holds two values (groups == C, DHW = 2): the normalised pair is +-1
    whatever the input, dx vanishes to O(eps / var) and has no relative accuracy in fp32, so those cases pass eps = 0.25 (var = O(1)),
    where dx is a well-conditioned function again.
    Measured rel-L2: y <= 4.4e-7, dx <= 1.8e-6, dgamma <= 3.2e-6 (C = 4, DHW = 210, N = 1: within 4x of the gate), dbeta <= 6.1e-7; worst row
    <= 2.3e-6; bf16 operands >= 3.4e-4."""
    eps = 0.25 if (groups == C and DHW == 2) else 1e-5
    L = _L()
    for N in (1, 3):
        x, gamma, beta, dy = _gn_inputs(N, C, groups, DHW, act, eps, torch.float32, C + groups + act * 7 + DHW + N)
        y_ref, dx_ref, dg_ref, db_ref = _gn_refs(x, gamma, beta, dy, groups, eps, act)
        y_bf, dx_bf, dg_bf, db_bf = _gn_refs(_bf(x), _bf(gamma), beta, _bf(dy), groups, eps, act)
        xd, dyd = _cl(x).float().contiguous().to(cuda), _cl(dy).float().contiguous().to(cuda)
        gd, bd = gamma.to(cuda), beta.to(cuda)
        sb = L.ldm_op_group_norm_f32_scratch_bytes(N, C, DHW, groups)

        def launch():
            s1, s2 = _nan(((sb + 3) // 4,), cuda), _nan(((sb + 3) // 4,), cuda)
            y, dx, dg, db = _nan((N * DHW, C), cuda), _nan((N * DHW, C), cuda), _nan((C,), cuda), _nan((C,), cuda)
            _call("ldm_op_group_norm_f32", _p(xd), C, _p(gd), _p(bd), groups, eps, act, _p(y), N, DHW, _p(s1), s1.numel() * 4, _stream())
            _call("ldm_op_group_norm_bwd_f32", _p(dyd), _p(xd), C, _p(gd), _p(bd), groups, eps, act, _p(dx), _p(dg), _p(db), N, DHW,
                  _p(s2), s2.numel() * 4, _stream())
            return y, dx, dg, db
        y, dx, dg, db = _twice(launch)
        what = f"group_norm_f32 N={N} C={C} G={groups} DHW={DHW} act={act}"
        _gate(y, _cl(y_ref), TOL_EXACT, what + " y", _cl(y_bf))
        _gate(dx, _cl(dx_ref), TOL_EXACT, what + " dx", _cl(dx_bf))
        _gate(dg[None], dg_ref[None], TOL_EXACT, what + " dgamma", dg_bf[None])
        _gate(db[None], db_ref[None], TOL_EXACT, what + " dbeta", db_bf[None])


@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("DHW", [27, 210])
def test_instance_norm_leaky_bf16_and_backward(cuda, C, DHW):
    """The bf16 entries as the discriminator calls them: ldm_op_group_norm / ldm_op_group_norm_bwd with groups == C, act 2, gamma = 1,
    beta = 0, eps 1e-5, N = 2, on bf16 x / dy.  y and dx (bf16) under the bf16 gate, dgamma / dbeta (fp32) at 1e-5.  Controls: the activation
    left out (y); the xhat mean(g xhat) term of dx dropped.
    Measured: y and dx 1.000 x floor, worst 0.50 ulp (controls 0.78 ... 0.80 and 0.42 ... 0.52); dgamma <= 8.2e-8, dbeta <= 6.7e-8."""
    N, groups, act, eps = 2, C, 2, 1e-5
    L = _L()
    x, gamma, beta, dy = _gn_inputs(N, C, groups, DHW, act, eps, torch.bfloat16, C + DHW, affine=False, dy_corr=0.5)
    y_ref, dx_ref, dg_ref, db_ref = _gn_refs(x, gamma, beta, dy, groups, eps, act)
    u = F.group_norm(x, groups, None, None, eps)                                   # gamma = 1, beta = 0: u = xhat
    gg = torch.where(u > 0, dy, 0.2 * dy)
    rstd = 1.0 / (x.var(2, unbiased=False, keepdim=True) + eps).sqrt()
    dx_def = rstd * (gg - gg.mean(2, keepdim=True))
    xd, dyd = _cl(x).to(torch.bfloat16).contiguous().to(cuda), _cl(dy).to(torch.bfloat16).contiguous().to(cuda)
    gd, bd = gamma.to(cuda), beta.to(cuda)
    sf, sbw = L.ldm_op_group_norm_scratch_bytes(N, C, DHW), L.ldm_op_group_norm_bwd_scratch_bytes(N, C, DHW, groups)

    def launch():
        s1, s2 = _nan(((sf + 3) // 4,), cuda), _nan(((sbw + 3) // 4,), cuda)
        y, dx = _nan((N * DHW, C), cuda, torch.bfloat16), _nan((N * DHW, C), cuda, torch.bfloat16)
        dg, db = _nan((C,), cuda), _nan((C,), cuda)
        _call("ldm_op_group_norm", _p(xd), C, None, 0, _p(gd), _p(bd), groups, eps, act, _p(y), N, DHW, _p(s1), s1.numel() * 4, _stream())
        _call("ldm_op_group_norm_bwd", _p(dyd), _p(xd), C, None, 0, _p(gd), _p(bd), groups, eps, act, None, None, _p(dx), None, _p(dg), _p(db),
              N, DHW, _p(s2), s2.numel() * 4, _stream())
        return y, dx, dg, db
    y, dx, dg, db = _twice(launch)
    what = f"instance_norm_leaky bf16 C={C} DHW={DHW}"
    _gate_bf(y, _cl(y_ref), what + " y", _cl(u), "activation left out")
    _gate_bf(dx, _cl(dx_ref), what + " dx", _cl(dx_def), "xhat mean(g xhat) term dropped")
    _gate32(dg[None], dg_ref[None], what + " dgamma")
    _gate32(db[None], db_ref[None], what + " dbeta")


def test_instance_norm_cancellation(cuda):
    """How the InstanceNorm result (groups == C, act 0, fp32 entry, C = 64, N = 2, DHW = 210, eps 1e-5) degrades as mean / std grows: inputs
    m + N(0, 1); the variance is E[x^2] - mean^2 from fp32 per-slab sums of squares folded in fp64 (gn_finalize_kernel).  Yardstick: the
    one-pass formula with sequential fp32 sums of x and x^2 on the same data (gan_ops_ref.instance_norm_naive_f32, CPU).  The kernel's rel-L2
    error against float64 must not exceed the naive formula's by more than 2x at m / std in {0, 4, 32, 256}; the ratios in between are
    printed for the record.  No absolute figure is gated.
    Measured (kernel / naive): 0: 4.0e-8 / 5.7e-8; 4: 3.3e-7 / 7.6e-7; 32: 1.9e-5 / 4.5e-5; 256: 1.1e-3 / 2.8e-3 -- the kernel is outside the
    1e-5 gate of this file from m / std = 32 on (16: 4.4e-6 is the largest measured ratio inside it)."""
    N, C, DHW, eps = 2, 64, 210, 1e-5
    L = _L()
    g = torch.Generator().manual_seed(210)
    z = torch.randn((N, DHW, C), generator=g, dtype=torch.float64)
    ones, zeros = torch.ones((C,), device=cuda), torch.zeros((C,), device=cuda)
    sb = L.ldm_op_group_norm_f32_scratch_bytes(N, C, DHW, C)
    gated, lines = (0.0, 4.0, 32.0, 256.0), []
    for ratio in (0.0, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0):
        x = (ratio + z).float()
        ref = F.group_norm(x.double().permute(0, 2, 1), C, None, None, eps).permute(0, 2, 1)
        naive = _rel(R.instance_norm_naive_f32(x, eps), ref)
        xd = x.reshape(N * DHW, C).contiguous().to(cuda)

        def launch():
            s1, y = _nan(((sb + 3) // 4,), cuda), _nan((N * DHW, C), cuda)
            _call("ldm_op_group_norm_f32", _p(xd), C, _p(ones), _p(zeros), C, eps, 0, _p(y), N, DHW, _p(s1), s1.numel() * 4, _stream())
            return (y,)
        (y,) = _twice(launch)
        e = _rel(y, ref.reshape(N * DHW, C))
        lines.append((ratio, e, naive))
        print(f"instance_norm_f32 cancellation mean/std {ratio:5.0f}: kernel rel-L2 {e:.2e}, naive one-pass fp32 {naive:.2e}"
              f"{'' if ratio in gated else ' (not gated)'}{'  [outside the 1e-5 gate]' if e > TOL_EXACT else ''}")
    for ratio, e, naive in lines:
        if ratio in gated:
            assert e <= 2 * naive, (ratio, e, naive)
