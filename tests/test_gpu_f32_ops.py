"""Per-kernel parity of the fp32 precision mode (-m gpu): every kernel of the fp32 plans, called through its ldm_op_*_f32 entry (the
same launch helpers the plan executor uses), against plain torch on the CPU in float64 on the same fp32 inputs (no rounding);
gradients from fp64 autograd.

Why operator level: the fp32 backward is gated only as whole-network gradients at 1e-3 (test_gpu_train.py), and at unit weight
gain those networks amplify a 1e-5 perturbation to 1e-3 of the gradient, so a kernel wrong by 1e-4 of a tensor would pass there.

Gates: rel-L2 <= 1e-5 for the exact fp32-MFMA forms, <= 3e-5 for the 3 x bf16 forms (conv form 1, x3 attention); the worst output row
relative to its own norm <= 10x the tensor gate.  Every case also shows, on the CPU, that the same operation on bf16-rounded operands
is more than 10x the gate away from the fp64 result, i.e. the gate would catch a kernel that lost its lo terms.  Outputs, slabs and
lse are NaN-filled before the launch and must come back finite, padding columns exactly zero, and a second launch bit-identical
(the fp32 plans have no atomics).  Measured values are printed (-s) and quoted in each test's docstring.
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from util import rup

pytestmark = pytest.mark.gpu
TOL_EXACT = 1e-5
TOL_X3 = 3e-5


def _lib():
    from ldm3d import _lib
    return _lib


def _call(name, *args):
    _lib().check(getattr(_lib().lib(), name)(*args))


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def C_int():
    import ctypes
    return ctypes.c_int()


def _nan(shape, cuda):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=cuda)


def _bf(t):
    return t.to(torch.bfloat16).double()


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _gate(got, ref, tol, what, bf16_ref=None):
    """rel-L2 <= tol, worst row (last dim = the row) <= 10 tol; bf16_ref (the op on bf16-rounded operands, fp64) > 10 tol away."""
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    e = _rel(got, ref)
    g2, r2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    rn = r2.norm(dim=1)
    keep = rn > 1e-6 * rn.max()
    worst = float(((g2 - r2).norm(dim=1)[keep] / rn[keep]).max())
    disc = _rel(bf16_ref, ref) if bf16_ref is not None else float("nan")
    print(f"{what}: rel-L2 {e:.2e} (gate {tol:.0e}), worst row {worst:.2e} (gate {10 * tol:.0e}), bf16 operands {disc:.1e}")
    assert e <= tol, (what, e)
    assert worst <= 10 * tol, (what, worst)
    if bf16_ref is not None:
        assert disc > 10 * tol, (what, "the gate cannot tell fp32 from bf16 operands", disc)
    return e


def _ndhwc(x, cs=None):
    """[N][C][D][H][W] -> fp32 NDHWC with cs (>= C) stored channels, padding zero."""
    n, c = x.shape[:2]
    cs = cs or c
    out = torch.zeros((n, *x.shape[2:], cs), dtype=torch.float32)
    out[..., :c] = x.permute(0, 2, 3, 4, 1)
    return out.contiguous()


def _wpack(w, cout_pad):
    """[cout][cin][k][k][k] -> [k^3][cout_pad][cin] fp32 (the fp32 arena layout), rows >= cout zero."""
    cout, cin = w.shape[:2]
    out = torch.zeros((w[0, 0].numel(), cout_pad, cin), dtype=torch.float32)
    out[:, :cout] = w.reshape(cout, cin, -1).permute(2, 0, 1)
    return out.contiguous()


def _conv_ref(x, w, b, stride, pad, ups):
    """fp64 torch reference of the kernels' addressing modes (ups 1: nearest x2; ups 2: zero insertion; stride 2 pad 0: F.pad(0, 1))."""
    if ups == 1:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    elif ups == 2:
        z = torch.zeros((*x.shape[:2], *(2 * s for s in x.shape[2:])), dtype=x.dtype)
        z[:, :, ::2, ::2, ::2] = x
        x = z
    if stride == 2 and pad == 0 and w.shape[-1] == 3:
        x = F.pad(x, (0, 1, 0, 1, 0, 1))
    return F.conv3d(x, w, b, stride=stride, padding=pad)


def _launch_conv(cuda, xa, ca, xb, cb, wp, bias, temb, temb_stride, res, couts, ncdhw, stats, n, dims, k, stride, pad, ups, cout, cout_pad,
                 form, bn, splitk, out_shape, st_shape):
    """NaN-filled outputs, one launch; returns (out, stats or None)."""
    out = _nan(out_shape, cuda)
    st = _nan(st_shape, cuda) if stats else None
    sk_max = splitk if splitk else 64
    M = out.numel() // (couts if not ncdhw else cout)
    scratch = _nan((sk_max * M * cout_pad,), cuda) if sk_max > 1 else None
    _call("ldm_op_conv3d_f32", _p(xa), ca, _p(xb), cb, _p(wp), _p(bias), _p(temb), temb_stride, _p(res),
          None if ncdhw else _p(out), couts, _p(out) if ncdhw else None, _p(st), n, *dims, k, stride, pad, ups, cout, cout_pad,
          form, bn, splitk, _p(scratch), 0 if scratch is None else scratch.numel() * 4, _stream())
    torch.cuda.synchronize()
    return out, st


def _conv_case(cuda, *, n=1, cin=(64, 0), cout=128, dims=(6, 5, 7), k=3, stride=1, pad=1, ups=0, form=0, bn=0, splitk=0,
               temb=False, residual=False, ncdhw=False, stats=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    ca, cb = cin
    c = ca + cb
    x = torch.randn((n, c, *dims), generator=g)
    w = torch.randn((cout, c, k, k, k), generator=g) / (c * k ** 3) ** 0.5
    b = 0.1 * torch.randn((cout,), generator=g)
    cout_pad = rup(cout, 64)
    couts = rup(cout, 32)
    ref = _conv_ref(x.double(), w.double(), b.double(), stride, pad, ups)
    ref_bf = _conv_ref(_bf(x), _bf(w), b.double(), stride, pad, ups)
    Do, Ho, Wo = ref.shape[2:]
    te = rs = None
    if temb:
        te = torch.zeros((n, cout_pad + 16))
        te[:, :cout] = torch.randn((n, cout), generator=g)
        ref = ref + te[:, :cout, None, None, None].double()
        ref_bf = ref_bf + te[:, :cout, None, None, None].double()
    if residual:
        r = torch.randn((n, cout, Do, Ho, Wo), generator=g)
        rs = _ndhwc(r, couts)
        ref, ref_bf = ref + r.double(), ref_bf + r.double()
    xn = _ndhwc(x)
    xa = xn[..., :ca].contiguous().to(cuda)
    xb = xn[..., ca:].contiguous().to(cuda) if cb else None
    wp = _wpack(w, cout_pad).to(cuda)
    bp = torch.zeros(cout_pad)
    bp[:cout] = b
    bp = bp.to(cuda)
    te_d = te.to(cuda) if te is not None else None
    rs_d = rs.to(cuda) if rs is not None else None
    out_shape = (n, cout, Do, Ho, Wo) if ncdhw else (n * Do * Ho * Wo, couts)
    rows = C_int()
    nrb = _lib().lib().ldm_op_conv3d_f32_stats_blocks(n, Do * Ho * Wo, couts, rows) if stats else 0
    st_shape = (n * nrb, couts, 2)
    args = (cuda, xa, ca, xb, cb, wp, bp, te_d, cout_pad + 16 if temb else 0, rs_d, couts, ncdhw, stats, n, dims, k, stride, pad, ups,
            cout, cout_pad, form, bn, splitk, out_shape, st_shape)
    out, st = _launch_conv(*args)
    out2, st2 = _launch_conv(*args)
    assert torch.equal(out, out2), "second launch differs"
    if stats:
        assert torch.equal(st, st2)
    tol = TOL_X3 if form else TOL_EXACT
    what = (f"conv3d_f32 form {form} bn {bn} splitk {splitk} n={n} cin={cin} cout={cout} {dims} k{k} s{stride} p{pad} ups{ups}"
            f"{' temb' if temb else ''}{' res' if residual else ''}{' ncdhw' if ncdhw else ''}")
    if ncdhw:
        e = _gate(out.permute(0, 2, 3, 4, 1), ref.permute(0, 2, 3, 4, 1), tol, what, ref_bf.permute(0, 2, 3, 4, 1))
    else:
        o = out.cpu()
        assert torch.equal(o[:, cout:], torch.zeros_like(o[:, cout:])), "padding columns must be exactly zero"
        e = _gate(o[:, :cout], ref.permute(0, 2, 3, 4, 1).reshape(-1, cout), tol, what, ref_bf.permute(0, 2, 3, 4, 1).reshape(-1, cout))
        if stats:
            o64 = o.double().view(n, Do * Ho * Wo, couts)
            s64 = st.cpu().double().view(n, nrb, couts, 2)
            for blk in range(nrb):
                seg = o64[:, blk * rows.value:(blk + 1) * rows.value]
                assert torch.allclose(s64[:, blk, :, 0], seg.sum(1), rtol=1e-5, atol=1e-4)
                assert torch.allclose(s64[:, blk, :, 1], (seg * seg).sum(1), rtol=1e-5, atol=1e-4)
    return e


# form x bn x splitk at 64 -> 128 channels, 6x5x7 (M = 210: two voxel tiles, the second ragged).  Form 0: 27 taps x 4 K steps = 108
# steps (5 splits: 22 + 22 + 22 + 22 + 20); form 1: 27 x 2 = 54 (5 splits: 11 x 4 + 10).
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("bn", [64, 128])
@pytest.mark.parametrize("splitk", [1, 3, 5])
def test_conv3d_f32_forms_tiles_splits(cuda, form, bn, splitk):
    """conv_f32_kernel<64|128> / conv_x3_kernel<64|128>, finalize_stats_f32_kernel (split cases).
    Measured rel-L2: form 0 3.1e-7 ... 6.5e-7, form 1 4.4e-6 ... 4.5e-6 (worst row <= 1.1e-6 / 6.1e-6)."""
    _conv_case(cuda, form=form, bn=bn, splitk=splitk, stats=splitk > 1, seed=form * 10 + bn + splitk)


@pytest.mark.parametrize("kw", [
    dict(cin=(16, 0), cout=64, dims=(8, 8, 8)),                                        # conv_in: 16 input channels (form 0 only)
    dict(cin=(64, 0), cout=4, ncdhw=True, splitk=3),                                   # conv_out: NCDHW output, finalize_f32_kernel
    dict(cin=(64, 0), cout=4, ncdhw=True, splitk=1, form=1),                           # NCDHW from the MFMA epilogue
    dict(cin=(96, 0), cout=32, dims=(5, 6, 4)),                                        # 96 -> 32: one 64-wide tile, half of it padding
    dict(cin=(96, 0), cout=32, dims=(5, 6, 4), form=1),
    dict(cin=(64, 0), cout=40, splitk=2, stats=True),                                  # padded stored columns (40 of 64)
    dict(cin=(128, 64), cout=128, dims=(4, 4, 4), form=1),                             # dual source (decoder concatenation)
    dict(cin=(128, 64), cout=128, dims=(4, 4, 4), form=0, splitk=4),
    dict(n=3, cin=(32, 0), cout=64, dims=(3, 5, 7), form=1),                           # ragged M over three samples
    dict(n=3, cin=(32, 0), cout=64, dims=(3, 5, 7), form=0, splitk=3),
    dict(cin=(32, 0), cout=64, dims=(8, 8, 8), stride=2, pad=1),                       # stride 2 pad 1
    dict(cin=(32, 0), cout=64, dims=(8, 6, 10), stride=2, pad=0, form=1),              # AEKLDownsample: F.pad(0, 1) then stride 2
    dict(cin=(64, 0), cout=64, dims=(4, 5, 3), ups=1, form=1),                         # fused nearest x2 upsample
    dict(cin=(64, 0), cout=64, dims=(4, 5, 3), ups=1, form=0, splitk=2),
    dict(n=2, cin=(64, 0), cout=128, dims=(4, 4, 4), temb=True, residual=True),        # ResBlock conv2: + temb[n] + residual
    dict(n=2, cin=(64, 0), cout=128, dims=(4, 4, 4), temb=True, residual=True, form=1, splitk=3),
    dict(cin=(32, 0), cout=64, k=1, pad=0, dims=(5, 5, 5)),                            # 1x1x1
    dict(cin=(256, 0), cout=256, dims=(12, 12, 12)),                                   # the training plan's 256 -> 256 at 12^3 (planner split)
])
def test_conv3d_f32_shapes(cuda, kw):
    """Ragged tiles, strides, upsampling, dual sources, epilogue terms.  Measured rel-L2: form 0 1.1e-7 ... 5.5e-7, form 1 2.2e-6 ... 4.5e-6
    (worst row <= 1.8e-6 / 2.1e-5, the latter a 4-channel NCDHW row)."""
    _conv_case(cuda, **kw)


def _flip_transpose(cuda, wp, k, cout, cout_pad, cin, ci_off, ci_cnt):
    L = _lib().lib()
    ws_bytes = L.ldm_op_weight_flip_transpose_f32_ws_bytes(k, cout, ci_cnt)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=cuda)
    wt = _nan((k ** 3, rup(ci_cnt, 64), rup(cout, 32)), cuda)
    _call("ldm_op_weight_flip_transpose_f32", _p(wp), _p(wt), k, cout, cout_pad, cin, ci_off, ci_cnt, _p(ws), ws.numel() * 4, _stream())
    torch.cuda.synchronize()
    return wt


@pytest.mark.parametrize("cin,cout,stride,pad,dims,src,take_grad", [
    ((64, 0), 64, 1, 1, (5, 6, 4), 0, False),
    ((64, 0), 96, 1, 1, (4, 4, 4), 0, True),            # += the gradient already staged for the input (take_grad)
    ((32, 0), 64, 2, 1, (8, 6, 4), 0, False),           # stride 2: zero-insertion upsample of dY (ups = 2)
    ((32, 0), 64, 2, 0, (8, 6, 10), 0, False),          # stride 2 pad 0 (F.pad form): pad' = 2, the extra output planes dropped
    ((64, 32), 64, 1, 1, (4, 5, 3), 1, False),          # dual-source conv: dX of the second source via ci_off
    ((64, 32), 64, 1, 1, (4, 5, 3), 0, True),
])
def test_conv3d_dgrad_f32(cuda, cin, cout, stride, pad, dims, src, take_grad):
    """Data gradient as the training plan runs it: weight_flip_transpose_batched_f32_kernel (one descriptor, ci_off / ci_cnt slice), then
    conv_f32_kernel on dY (pad' = 2 - pad, stride 2 -> ups = 2), against fp64 autograd dX.  Measured rel-L2 2.5e-7 ... 6.3e-7."""
    g = torch.Generator().manual_seed(cout + dims[0] + 7 * src)
    ca, cb = cin
    c, k = ca + cb, 3
    x = torch.randn((1, c, *dims), generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn((cout, c, k, k, k), generator=g) / (c * 27) ** 0.5)
    y = _conv_ref(x, w.double(), None, stride, pad, 0)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.double())
    ci_off, ci_cnt = (0, ca) if src == 0 else (ca, cb)
    ref = x.grad[:, ci_off:ci_off + ci_cnt]
    xb_ = x.detach().clone().requires_grad_(True)
    _conv_ref(xb_, _bf(w), None, stride, pad, 0).backward(_bf(dy))
    ref_bf = xb_.grad[:, ci_off:ci_off + ci_cnt]
    acc = None
    if take_grad:
        acc = torch.randn((1, ci_cnt, *dims), generator=g)
        ref, ref_bf = ref + acc.double(), ref_bf + acc.double()
    cout_pad = rup(cout, 64)
    wp = _wpack(w, cout_pad).to(cuda)
    wt = _flip_transpose(cuda, wp, k, cout, cout_pad, c, ci_off, ci_cnt)
    wt2 = _flip_transpose(cuda, wp, k, cout, cout_pad, c, ci_off, ci_cnt)
    assert torch.equal(wt, wt2) and torch.isfinite(wt).all()
    # the flip-transpose itself is a permutation: exact
    exp = torch.zeros_like(wt.cpu())
    exp[:, :ci_cnt, :cout] = w.reshape(cout, c, 27).permute(2, 1, 0).flip(0)[:, ci_off:ci_off + ci_cnt]
    assert torch.equal(wt.cpu(), exp)
    cdy = rup(cout, 32)
    dyn = _ndhwc(dy, cdy).to(cuda)
    dd = dy.shape[2:]
    pad_d = k - 1 - pad
    ups = 2 if stride == 2 else 0
    Do = (dd[0] << (ups > 0)) + 2 * pad_d - 2
    Ho = (dd[1] << (ups > 0)) + 2 * pad_d - 2
    Wo = (dd[2] << (ups > 0)) + 2 * pad_d - 2
    couts = rup(ci_cnt, 32)
    cpad = rup(ci_cnt, 64)
    res = None
    if take_grad:
        res = _ndhwc(acc, couts).to(cuda)
    outs = []
    for _ in range(2):
        out = _nan((Do * Ho * Wo, couts), cuda)
        _call("ldm_op_conv3d_f32", _p(dyn), cdy, None, 0, _p(wt), None, None, 0, _p(res), _p(out), couts, None, None,
              1, *dd, k, 1, pad_d, ups, ci_cnt, cpad, 0, 0, 1, None, 0, _stream())
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    o = outs[0].view(Do, Ho, Wo, couts)[:dims[0], :dims[1], :dims[2]]
    assert torch.equal(o[..., ci_cnt:], torch.zeros_like(o[..., ci_cnt:]))
    _gate(o[..., :ci_cnt].reshape(-1, ci_cnt), ref[0].permute(1, 2, 3, 0).reshape(-1, ci_cnt), TOL_EXACT,
          f"dgrad_f32 cin={cin} src={src} cout={cout} s{stride} p{pad} {dims}{' +acc' if take_grad else ''}",
          ref_bf[0].permute(1, 2, 3, 0).reshape(-1, ci_cnt))


@pytest.mark.parametrize("n,cin,cout,dims,k,stride,pad,ups,ksplit", [
    (1, (64, 0), 64, (6, 5, 4), 3, 1, 1, 0, 1),
    (1, (64, 0), 64, (6, 5, 4), 3, 1, 1, 0, 3),
    (1, (32, 0), 64, (8, 6, 4), 3, 2, 1, 0, 2),          # stride 2
    (1, (32, 0), 64, (8, 6, 10), 3, 2, 0, 0, 1),         # stride 2 pad 0 (F.pad form)
    (1, (64, 0), 32, (4, 5, 3), 3, 1, 1, 1, 2),          # fused nearest x2 upsample
    (2, (64, 0), 64, (5, 3, 2), 1, 1, 0, 0, 1),          # 1x1, batch 2
    (1, (96, 0), 160, (4, 4, 4), 3, 1, 1, 0, 1),         # part tiles on both sides
    (1, (160, 0), 96, (4, 4, 4), 3, 1, 1, 0, 3),
    (2, (64, 32), 64, (5, 3, 2), 3, 1, 1, 0, 1),         # dual source: the second source's columns at dw_ci_off
    (1, (32, 0), 64, (2, 2, 2), 3, 1, 1, 0, 3),          # 8 voxels = one K step: splits 1 and 2 are empty (zero slabs)
    (2, (32, 0), 32, (2, 2, 2), 3, 1, 1, 0, 1),
])
def test_conv3d_wgrad_f32(cuda, n, cin, cout, dims, k, stride, pad, ups, ksplit):
    """wgrad_f32_kernel with taps, dw_ld / dw_ci_off, ksplit slabs, against fp64 autograd dW.  Measured rel-L2 3.7e-8 ... 2.4e-7."""
    g = torch.Generator().manual_seed(n * 100 + cout + k + ksplit)
    ca, cb = cin
    c = ca + cb
    x = torch.randn((n, c, *dims), generator=g)
    w = torch.randn((cout, c, k, k, k), generator=g, dtype=torch.float64, requires_grad=True)
    y = _conv_ref(x.double(), w, None, stride, pad, ups)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.double())
    taps = k ** 3
    ref = w.grad.reshape(cout, c, taps).permute(2, 0, 1)            # [tap][co][ci]
    wb = w.detach().clone().requires_grad_(True)
    _conv_ref(_bf(x), wb, None, stride, pad, ups).backward(_bf(dy))
    ref_bf = wb.grad.reshape(cout, c, taps).permute(2, 0, 1)
    cdy = rup(cout, 32)
    dyn = _ndhwc(dy, cdy).to(cuda)
    xn = _ndhwc(x)
    srcs = [(xn[..., :ca].contiguous().to(cuda), ca, 0)] + ([(xn[..., ca:].contiguous().to(cuda), cb, ca)] if cb else [])
    outs = []
    for _ in range(2):
        dw = _nan((ksplit, taps, cout, c), cuda)
        for xs, cs, off in srcs:
            _call("ldm_op_conv3d_wgrad_f32", _p(dyn), cdy, _p(xs), cs, _p(dw), cout, cs, c, off, n, *dims, k, stride, pad, ups, ksplit, _stream())
        torch.cuda.synchronize()
        outs.append(dw.cpu())
    assert torch.equal(outs[0], outs[1])
    dw = outs[0]
    assert torch.isfinite(dw).all(), "a slab was left unwritten"
    Mtot = y[0, 0].numel() * n
    steps = (Mtot + 15) // 16
    sps = (steps + ksplit - 1) // ksplit
    for s in range(ksplit):
        if s * sps >= steps:
            assert torch.equal(dw[s], torch.zeros_like(dw[s])), "empty split must leave a zero slab"
    _gate(dw.double().sum(0), ref, TOL_EXACT, f"wgrad_f32 n={n} cin={cin} cout={cout} {dims} k{k} s{stride} p{pad} ups{ups} ksplit {ksplit}",
          ref_bf)


def _attn_ref(qkv, B, N, C, d):
    q, k, v = qkv.view(B, N, 3, C // d, d).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / d ** 0.5
    o = torch.softmax(s, -1) @ v
    return o.permute(0, 2, 1, 3).reshape(B * N, C), torch.logsumexp(s, -1)


@pytest.mark.parametrize("B,N,C,d,x3", [
    (1, 216, 64, 32, 0),       # attn_f32_split_kernel<1>
    (2, 130, 64, 32, 0),
    (1, 343, 128, 64, 0),      # attn_f32_split_kernel<2>
    (1, 343, 128, 64, 1),      # attn_f32_split_kernel<2, true>
    (1, 1728, 512, 64, 0),     # 8 heads, the 12^3 level
    (1, 1728, 512, 64, 1),
    (2, 100, 128, 64, 0),      # attn_f32_kernel<2> (N < 128)
    (1, 127, 64, 32, 1),       # attn_f32_kernel<1>, one below the split boundary (x3 has no effect there)
    (1, 128, 64, 32, 0),       # the boundary: split kernel
    (1, 512, 256, 128, 0),     # attn_f32_kernel<4>
    (2, 216, 256, 256, 0),     # attn_f32_kernel<8>
])
def test_attention_f32(cuda, B, N, C, d, x3):
    """Flash-style fp32 attention and its lse rows against fp64 softmax / logsumexp (lse to 1e-5 absolute).
    Measured rel-L2: exact 2.5e-7 ... 5.8e-7, x3 6.2e-6 ... 6.3e-6 (worst row 1.4e-5); lse error <= 1.1e-6 exact, 4.5e-6 x3."""
    g = torch.Generator().manual_seed(N + C + d + x3)
    qkv = torch.randn((B * N, 3 * C), generator=g)
    ref, lse_ref = _attn_ref(qkv.double(), B, N, C, d)
    ref_bf, _ = _attn_ref(_bf(qkv), B, N, C, d)
    qd = qkv.to(cuda)
    outs = []
    for _ in range(2):
        out = _nan((B * N, C), cuda)
        lse = _nan((B, C // d, N), cuda)
        _call("ldm_op_attention_f32", _p(qd), _p(out), _p(lse), B, N, C, d, x3, _stream())
        torch.cuda.synchronize()
        outs.append((out.cpu(), lse.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    out, lse = outs[0]
    tol = TOL_X3 if (x3 and d == 64 and N >= 128) else TOL_EXACT
    _gate(out.view(B * N, C // d, d), ref.view(B * N, C // d, d), tol, f"attention_f32 B={B} N={N} C={C} d={d} x3={x3}",
          ref_bf.view(B * N, C // d, d))
    assert torch.isfinite(lse).all()
    le = float((lse.double() - lse_ref).abs().max())
    print(f"  lse max abs error {le:.1e}")
    assert le <= 1e-5


@pytest.mark.parametrize("B,N,C,d", [
    (2, 77, 64, 32),
    (2, 130, 128, 64),
    (1, 343, 256, 64),
    (2, 100, 256, 128),
    (2, 45, 512, 256),
])
def test_attention_bwd_f32(cuda, B, N, C, d):
    """attn32_delta / attn32_bwd_dq / attn32_bwd_dkv against fp64 autograd; fed the forward op's own o and lse; dq, dk, dv gated
    separately.  Measured rel-L2 3.4e-7 ... 5.5e-7."""
    g = torch.Generator().manual_seed(B * N + C + d)
    qkv = torch.randn((B * N, 3 * C), generator=g)
    do = torch.randn((B * N, C), generator=g)
    q64 = qkv.double().requires_grad_(True)
    _attn_ref(q64, B, N, C, d)[0].backward(do.double())
    ref = q64.grad
    qb = _bf(qkv).requires_grad_(True)
    _attn_ref(qb, B, N, C, d)[0].backward(_bf(do))
    ref_bf = qb.grad
    qd, dod = qkv.to(cuda), do.to(cuda)
    o = _nan((B * N, C), cuda)
    lse = _nan((B, C // d, N), cuda)
    _call("ldm_op_attention_f32", _p(qd), _p(o), _p(lse), B, N, C, d, 0, _stream())
    outs = []
    for _ in range(2):
        delta = _nan((B * (C // d) * N,), cuda)
        dqkv = _nan((B * N, 3 * C), cuda)
        _call("ldm_op_attention_bwd_f32", _p(qd), _p(o), _p(dod), _p(lse), _p(delta), _p(dqkv), B, N, C, d, _stream())
        torch.cuda.synchronize()
        outs.append(dqkv.cpu())
    assert torch.equal(outs[0], outs[1])
    got = outs[0]
    for j, name in enumerate("qkv"):
        sl = slice(j * C, (j + 1) * C)
        _gate(got[:, sl], ref[:, sl], TOL_EXACT, f"attention_bwd_f32 d{name} B={B} N={N} C={C} d={d}", ref_bf[:, sl])


def _gn_ref(x, gamma, beta, groups, eps, act):
    y = F.group_norm(x, groups, gamma, beta, eps)
    return F.silu(y) if act == 1 else (F.leaky_relu(y, 0.2) if act == 2 else y)


@pytest.mark.parametrize("n,ca,cb,groups,dims,act,acc", [
    (1, 96, 0, 32, (5, 4, 3), 1, False),       # 3 channels per group
    (2, 128, 0, 32, (4, 5, 3), 0, True),       # 4 per group, batch 2: per-sample dgamma / dbeta rows summed (rowsum_n)
    (2, 512, 0, 16, (3, 3, 3), 1, True),       # 32 per group
    (1, 512, 256, 32, (3, 2, 3), 1, True),     # dual source (decoder concatenation), accumulating both sources
    (2, 512, 256, 32, (2, 3, 3), 0, False),
    (1, 64, 0, 32, (7, 3, 5), 2, False),       # LeakyReLU (discriminator InstanceNorm form uses groups = C)
])
def test_group_norm_bwd2_f32(cuda, n, ca, cb, groups, dims, act, acc):
    """gn_stats_f32 / gn_finalize (forward statistics), gnb32_stats, gn_bwd_finalize, gnb32_apply (two sources, acc_a / acc_b) and
    rowsum_n against fp64 autograd.  Measured rel-L2: dx 4.4e-8 ... 7.5e-8, dgamma / dbeta 6.6e-8 ... 1.1e-7."""
    g = torch.Generator().manual_seed(n + ca + cb + groups + act)
    C = ca + cb
    DHW = dims[0] * dims[1] * dims[2]
    x = 1.5 * torch.randn((n, C, *dims), generator=g) + 0.3
    gamma = 1 + 0.2 * torch.randn((C,), generator=g)
    beta = 0.2 * torch.randn((C,), generator=g)
    dy = torch.randn((n, C, *dims), generator=g)
    acc_t = 0.5 * torch.randn((n, C, *dims), generator=g) if acc else None
    eps = 1e-6

    def ref_of(xx, dd, gg):
        xx, gm, bt = xx.clone().requires_grad_(True), gg.clone().requires_grad_(True), beta.double().requires_grad_(True)
        _gn_ref(xx, gm, bt, groups, eps, act).backward(dd)
        dx = xx.grad + (acc_t.double() if acc else 0)
        return dx, gm.grad, bt.grad
    dx_ref, dg_ref, db_ref = ref_of(x.double(), dy.double(), gamma.double())
    dx_bf, dg_bf, db_bf = ref_of(_bf(x), _bf(dy), _bf(gamma))
    xn, dyn = _ndhwc(x), _ndhwc(dy)
    xa, xb = xn[..., :ca].contiguous().to(cuda), (xn[..., ca:].contiguous().to(cuda) if cb else None)
    acn = _ndhwc(acc_t) if acc else None
    aa = acn[..., :ca].contiguous().to(cuda) if acc else None
    ab_ = acn[..., ca:].contiguous().to(cuda) if (acc and cb) else None
    dy_d, gamma_d, beta_d = dyn.to(cuda), gamma.to(cuda), beta.to(cuda)
    L = _lib().lib()
    sb = L.ldm_op_group_norm_f32_scratch_bytes(n, C, DHW, groups)
    outs = []
    for _ in range(2):
        scratch = _nan(((sb + 3) // 4,), cuda)
        dxa, dxb = _nan((n * DHW, ca), cuda), (_nan((n * DHW, cb), cuda) if cb else None)
        dg, db = _nan((C,), cuda), _nan((C,), cuda)
        _call("ldm_op_group_norm_bwd2_f32", _p(dy_d), _p(xa), ca, _p(xb), cb, _p(gamma_d), _p(beta_d), groups, eps,
              act, _p(aa), _p(ab_), _p(dxa), _p(dxb), _p(dg), _p(db), n, DHW, _p(scratch), scratch.numel() * 4, _stream())
        torch.cuda.synchronize()
        dx = torch.cat([dxa, dxb], 1) if cb else dxa
        outs.append((dx.cpu(), dg.cpu(), db.cpu()))
    for a_, b_ in zip(outs[0], outs[1]):
        assert torch.equal(a_, b_)
    dx, dg, db = outs[0]
    what = f"group_norm_bwd2_f32 n={n} C={ca}+{cb} G={groups} {dims} act={act}{' +acc' if acc else ''}"
    _gate(dx, dx_ref.permute(0, 2, 3, 4, 1).reshape(-1, C), TOL_EXACT, what + " dx", dx_bf.permute(0, 2, 3, 4, 1).reshape(-1, C))
    _gate(dg[None], dg_ref[None], TOL_EXACT, what + " dgamma", dg_bf[None])
    _gate(db[None], db_ref[None], TOL_EXACT, what + " dbeta", db_bf[None])


def test_upsample_bwd_f32(cuda):
    """sumpool2_f32_kernel (adjoint of the fused nearest x2 upsample) against fp64 autograd of F.interpolate.  Measured rel-L2 5.6e-8."""
    g = torch.Generator().manual_seed(5)
    n, C, dims = 2, 96, (3, 5, 2)
    x = torch.zeros((n, C, *dims), dtype=torch.float64, requires_grad=True)
    dy = torch.randn((n, C, *(2 * s for s in dims)), generator=g)
    F.interpolate(x, scale_factor=2.0, mode="nearest").backward(dy.double())
    ref = x.grad.permute(0, 2, 3, 4, 1).reshape(-1, C)
    xb = torch.zeros_like(x).requires_grad_(True)
    F.interpolate(xb, scale_factor=2.0, mode="nearest").backward(_bf(dy))
    dyn = _ndhwc(dy).to(cuda)
    outs = []
    for _ in range(2):
        dx = _nan((n * dims[0] * dims[1] * dims[2], C), cuda)
        _call("ldm_op_upsample_bwd_f32", _p(dyn), _p(dx), n, *dims, C, _stream())
        torch.cuda.synchronize()
        outs.append(dx.cpu())
    assert torch.equal(outs[0], outs[1])
    _gate(outs[0], ref, TOL_EXACT, "upsample_bwd_f32", xb.grad.permute(0, 2, 3, 4, 1).reshape(-1, C))


def test_bad_arguments_are_refused_before_the_device(cuda):
    """Argument checks return LDM_ERR_BAD_ARG (-1) without launching anything."""
    L = _lib().lib()
    x = torch.zeros(64, device=cuda)
    s = _stream()
    # form 1 needs 32-channel sources; both / neither output; unknown bn
    assert L.ldm_op_conv3d_f32(_p(x), 16, None, 0, _p(x), None, None, 0, None, _p(x), 64, None, None, 1, 2, 2, 2, 3, 1, 1, 0, 64, 64,
                               1, 0, 1, None, 0, s) == -1
    assert L.ldm_op_conv3d_f32(_p(x), 16, None, 0, _p(x), None, None, 0, None, _p(x), 64, _p(x), None, 1, 2, 2, 2, 3, 1, 1, 0, 64, 64,
                               0, 0, 1, None, 0, s) == -1
    assert L.ldm_op_conv3d_f32(_p(x), 16, None, 0, _p(x), None, None, 0, None, _p(x), 64, None, None, 1, 2, 2, 2, 3, 1, 1, 0, 64, 64,
                               0, 96, 1, None, 0, s) == -1
    assert L.ldm_op_conv3d_wgrad_f32(_p(x), 32, _p(x), 32, _p(x), 32, 32, 16, 0, 1, 2, 2, 2, 3, 1, 1, 0, 1, s) == -1   # dw_ld < cin
    assert L.ldm_op_attention_f32(_p(x), _p(x), None, 1, 8, 96, 64, 0, s) == -1                                          # C % d
    assert L.ldm_op_group_norm_bwd2_f32(_p(x), _p(x), 30, None, 0, _p(x), _p(x), 3, 1e-6, 0, None, None, _p(x), None, _p(x), _p(x),
                                        1, 1, _p(x), 1 << 20, s) == -1                                                    # ca % 4
    assert L.ldm_op_weight_flip_transpose_f32(_p(x), _p(x), 3, 8, 64, 32, 16, 32, _p(x), 1 << 20, s) == -1              # slice past cin
    torch.cuda.synchronize()


_SECOND_DEVICE = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from ldm3d import _lib
L = _lib.lib()
for dev in (0, 1):
    torch.cuda.set_device(dev)
    for (N, C, d) in ((300, 128, 64), (100, 256, 256), (64, 128, 128)):
        g = torch.Generator().manual_seed(N)
        qkv = torch.randn((N, 3 * C), generator=g).cuda()
        o = torch.empty((N, C), device="cuda"); lse = torch.empty((C // d, N), device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        _lib.check(L.ldm_op_attention_f32(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), 1, N, C, d, 0, s))
        do = torch.randn((N, C), generator=g).cuda()
        delta = torch.empty(((C // d) * N,), device="cuda"); dq = torch.empty((N, 3 * C), device="cuda")
        _lib.check(L.ldm_op_attention_bwd_f32(qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(),
                                              1, N, C, d, s))
        torch.cuda.synchronize()
        assert torch.isfinite(o).all() and torch.isfinite(dq).all(), (dev, N, C, d)
print("ok")
"""


def test_attention_f32_on_a_second_device(cuda):
    """hipFuncSetAttribute (up to 74,880 B of dynamic LDS) is recorded per device: the fp32 attention forward and backward run on
    cuda:1 after cuda:0 in one process (a child, so this process's device state is untouched)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _SECOND_DEVICE, root], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
