"""Per-kernel parity of the bf16 training plans (-m gpu): every kernel the bf16 backward plans launch, called through its ldm_op_* entry
(the same launch helpers and geometry functions the plan executor uses), against plain torch on the CPU in float64 on exactly the bf16
inputs the kernel reads (and, for GroupNorm, the same fp32 saved statistics ab / mr); gradients from fp64 autograd where there is a
forward to differentiate (GroupNorm + act, nearest x2 upsample, Linear + SiLU, the clamp / exp head).

Why operator level: these kernels run only inside ldm_unet_train_backward / ldm_vae_train_backward, whose gates (test_gpu_train.py) sit
at the bf16 noise floor of whole-network gradients; a kernel wrong by a few 1e-3 of one tensor passes there.

Gates (the inputs are identical, so only the kernels' fp32 arithmetic and the final bf16 store remain):
  fp32 outputs (dgamma, dbeta, cs, column sums, linear dx / dW / db, exports, VAE heads): rel-L2 <= 1e-5, worst row <= 1e-4 of its norm;
  bf16 outputs (GroupNorm dx, sumpool, heads gradient): rel-L2 <= 1.2 x the floor rel-L2(bf16(ref), ref), and no element more than one
  bf16 ulp of ref from ref after an absolute allowance of 1e-5 max|ref|;
  data movement and exact sums (exports with nsplit 1, flip-transpose, add_bf16, sumpool2 on exactly summable inputs): bit-identical to
  torch, round-to-nearest-even included.
Every case NaN-fills outputs and scratch before the launch and requires finite outputs with padding exactly zero, a bit-identical second
launch (no atomics in these kernels), and shows on the CPU that one named plausible defect lands more than 10x outside its gate.
Measured values are printed (-s) and quoted in the docstrings.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from util import rup

pytestmark = pytest.mark.gpu
TOL = 1e-5           # fp32 outputs: rel-L2; worst row 10x
BF_FLOOR_X = 1.2     # bf16 outputs: rel-L2 <= 1.2 x the bf16 rounding floor
ERR_BAD_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -5


def _L():
    from ldm3d import _lib
    return _lib.lib()


def _call(name, *args):
    from ldm3d import _lib
    _lib.check(getattr(_L(), name)(*args))


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _nan(shape, cuda, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=cuda)


def _bfr(t):
    """round to bf16 (RNE), back to float64"""
    return t.to(torch.bfloat16).double()


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _worst_row(got, ref):
    g2, r2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    rn = r2.norm(dim=1)
    keep = rn > 1e-6 * rn.max()
    return float(((g2 - r2).norm(dim=1)[keep] / rn[keep]).max())


def _gate32(got, ref, what, defect=None, defect_name=""):
    """fp32 output: rel-L2 <= TOL, worst row <= 10 TOL; the defect (fp64, same layout) > 10x the gate away from ref."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    e, w = _rel(got, ref), _worst_row(got, ref)
    d = _rel(defect, ref) if defect is not None else float("nan")
    print(f"{what}: rel-L2 {e:.2e} (gate {TOL:.0e}), worst row {w:.2e} (gate {10 * TOL:.0e})"
          + (f"; defect '{defect_name}' {d:.1e}" if defect is not None else ""))
    assert e <= TOL, (what, e)
    assert w <= 10 * TOL, (what, w)
    if defect is not None:
        assert d > 10 * TOL, (what, f"the gate cannot see '{defect_name}'", d)
    return e


def _ulp_bf16(r):
    """one bf16 ulp at |r| (r float64): 2^(exponent - 7) with r = m 2^exponent, 1 <= m < 2"""
    _, ex = torch.frexp(r.abs().clamp_min(1e-38))
    return torch.ldexp(torch.ones_like(r), (ex - 8).to(torch.int32))


def _gate_bf(got, ref, what, defect=None, defect_name=""):
    """bf16 output: rel-L2 <= 1.2 x rel-L2(bf16(ref), ref); |got - ref| <= ulp(ref) + 1e-5 max|ref| everywhere; defect > 10x the gate."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    floor = _rel(_bfr(ref), ref)
    gate = BF_FLOOR_X * floor
    e = _rel(got, ref)
    allow = _ulp_bf16(ref) + 1e-5 * ref.abs().max()
    over = float(((got - ref).abs() / allow).max())
    d = _rel(defect, ref) if defect is not None else float("nan")
    print(f"{what}: rel-L2 {e:.3e} = {e / floor:.3f} x floor {floor:.3e} (gate {BF_FLOOR_X} x), worst |err| / (1 ulp + abs) {over:.2f}"
          + (f"; defect '{defect_name}' {d:.1e}" if defect is not None else ""))
    assert e <= gate, (what, e, floor)
    assert over <= 1.0, (what, "an element is more than one bf16 ulp off", over)
    if defect is not None:
        assert d > 10 * gate, (what, f"the gate cannot see '{defect_name}'", d, gate)
    return e


def _i64(rows):
    flat = [int(v) for r in rows for v in r]
    return (ctypes.c_int64 * len(flat))(*flat)


# ------------------------------------------------------------------------------------------------ GroupNorm(+act) backward
def _fold_geom(N, C, DHW):
    """gnb_fold_chunks of the planner, restated: (chunks, rows per block)"""
    slices = (C + 63) // 64
    ch = max(1, min(256 // (slices * N), (DHW + 31) // 32))
    rpb = rup((DHW + ch - 1) // ch, 32)
    return (DHW + rpb - 1) // rpb, rpb


def _act(u, act):
    return F.silu(u) if act == 1 else (F.leaky_relu(u, 0.2) if act == 2 else u)


GN_CASES = [
    # n, ca, cb, groups, dims, act, acc ("", "a", "ab")
    (1, 64, 0, 32, (6, 5, 7), 1, ""),         # cpg 2, ragged DHW (210 = 6 x 32 + 18)
    (1, 128, 0, 32, (6, 5, 7), 0, "a"),       # cpg 4
    (2, 256, 0, 32, (4, 4, 5), 2, "a"),       # cpg 8, batch 2 (rowsum_n), LeakyReLU
    (1, 512, 0, 32, (3, 5, 7), 1, "a"),       # cpg 16
    (1, 512, 256, 32, (3, 4, 5), 1, "a"),     # 768 = 512 + 256: cpg 24 groups straddle the 64-channel slices; only acc_a
    (2, 512, 512, 32, (2, 3, 5), 1, "ab"),    # 1024 = 512 + 512, batch 2, both accumulations
    (1, 96, 32, 4, (5, 5, 3), 1, "ab"),       # slice [64, 128) crosses the source boundary at 96
    (1, 192, 0, 4, (3, 4, 6), 1, ""),         # cpg 48: does not divide 64
    (2, 256, 0, 4, (3, 3, 4), 0, ""),         # cpg 64: the fold's eligibility limit
    (1, 256, 0, 2, (3, 3, 4), 1, "a"),        # cpg 128: finalize + apply only (the fold form is refused)
    (1, 64, 0, 32, (32, 32, 32), 1, "a"),     # 32^3: nslab = 512 and chunks = 256, their caps
]


def _gn_inputs(n, ca, cb, groups, dims, act, acc, seed):
    g = torch.Generator().manual_seed(seed)
    C = ca + cb
    eps = 1e-6
    x = _bfr(1.3 * torch.randn((n, C, *dims), generator=g) + 0.2)
    gamma = (1 + 0.3 * torch.randn((C,), generator=g)).float()
    beta = (0.2 * torch.randn((C,), generator=g)).float()
    # dy correlated with x and offset: both group-mean terms of dx (mean(gamma g), mean(gamma g xhat)) matter
    dy = _bfr(torch.randn((n, C, *dims), generator=g) + 0.5 * x.float() + 0.2)
    acc_a = _bfr(0.5 * torch.randn((n, ca, *dims), generator=g)) if "a" in acc else None
    acc_b = _bfr(0.5 * torch.randn((n, cb, *dims), generator=g)) if ("b" in acc and cb) else None
    xg = x.reshape(n, groups, -1)
    mean = xg.mean(2)
    rstd = 1.0 / torch.sqrt(xg.var(2, unbiased=False) + eps)
    mr = torch.stack([mean, rstd], 2).float()                       # [N][G][2], what the training forward keeps
    cpg = C // groups
    m_c, r_c = mr[..., 0].double().repeat_interleave(cpg, 1), mr[..., 1].double().repeat_interleave(cpg, 1)
    a = gamma.double() * r_c
    b = beta.double() - m_c * a
    ab = torch.stack([a, b], 2).float()                             # [N][C][2]
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, acc_a=acc_a, acc_b=acc_b, mr=mr, ab=ab, eps=eps)


def _gn_reference(t, n, ca, cb, groups, dims, act):
    """fp64 autograd through act(gamma (x - mean) rstd + beta) with the kernel's fp32 (mean, rstd) held fixed as the forward's statistics
    would be differentiated: dx = d/dx of the full GroupNorm (mean / rstd as functions of x), evaluated at the saved values."""
    C = ca + cb
    x = t["x"].clone().requires_grad_(True)
    gm = t["gamma"].double().clone().requires_grad_(True)
    bt = t["beta"].double().clone().requires_grad_(True)
    y = _act(F.group_norm(x, groups, gm, bt, t["eps"]), act)
    y.backward(t["dy"])
    dx = x.grad.clone()
    if t["acc_a"] is not None:
        dx[:, :ca] += t["acc_a"]
    if t["acc_b"] is not None:
        dx[:, ca:] += t["acc_b"]
    # the named defect of dx: the xhat * mean(gamma g xhat) term dropped (recomputed by hand from the same pieces)
    xh = (t["x"] - t["mr"][..., 0].double().repeat_interleave(C // groups, 1)[..., None, None, None]) \
        * t["mr"][..., 1].double().repeat_interleave(C // groups, 1)[..., None, None, None]
    u = gm.detach()[None, :, None, None, None] * xh + bt.detach()[None, :, None, None, None]
    uu = u.clone().requires_grad_(True)
    _act(uu, act).backward(t["dy"])
    gg = uu.grad
    m1 = (gm.detach()[None, :, None, None, None] * gg).reshape(n, groups, -1).mean(2).repeat_interleave(C // groups, 1)
    rs = t["mr"][..., 1].double().repeat_interleave(C // groups, 1)
    dx_def = rs[..., None, None, None] * (gm.detach()[None, :, None, None, None] * gg - m1[..., None, None, None]) + (dx - x.grad)
    return dx, gm.grad, bt.grad, gg, xh, dx_def


def _cl(t):
    """[N][C][D][H][W] -> [N*DHW][C]"""
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])


def _dev_bf(t, cuda):
    return t.permute(0, 2, 3, 4, 1).contiguous().to(torch.bfloat16).to(cuda) if t is not None else None


def _launch_gnb(cuda, t, n, ca, cb, groups, dims, act, form, chunks):
    C = ca + cb
    DHW = dims[0] * dims[1] * dims[2]
    xd = _dev_bf(t["x"], cuda)
    xa, xb = xd[..., :ca].contiguous(), (xd[..., ca:].contiguous() if cb else None)
    dyd = _dev_bf(t["dy"], cuda)
    aa, abb = _dev_bf(t["acc_a"], cuda), _dev_bf(t["acc_b"], cuda)
    abd, mrd, gmd = t["ab"].to(cuda), t["mr"].to(cuda), t["gamma"].to(cuda)
    sb = _L().ldm_op_group_norm_bwd_saved_scratch_bytes(n, C, DHW, groups)
    outs = []
    for _ in range(2):
        scratch = _nan(((sb + 3) // 4,), cuda)
        dxa = _nan((n * DHW, ca), cuda, torch.bfloat16)
        dxb = _nan((n * DHW, cb), cuda, torch.bfloat16) if cb else None
        dg, db = _nan((C,), cuda), _nan((C,), cuda)
        cs = _nan((n * chunks * C * 2,), cuda) if form == 1 else None
        _call("ldm_op_group_norm_bwd_saved", _p(dyd), _p(xa), ca, _p(xb), cb, _p(abd), _p(mrd), _p(gmd), groups, act, _p(aa), _p(abb),
              _p(dxa), _p(dxb), _p(dg), _p(db), _p(cs), n, DHW, form, _p(scratch), scratch.numel() * 4, _s())
        torch.cuda.synchronize()
        dx = torch.cat([dxa, dxb], 1) if cb else dxa
        outs.append([v.cpu() for v in (dx, dg, db)] + ([cs.cpu()] if cs is not None else []))
    for a_, b_ in zip(outs[0], outs[1]):
        assert torch.equal(a_, b_), "second launch differs"
    return outs[0]


@pytest.mark.parametrize("n,ca,cb,groups,dims,act,acc", GN_CASES)
def test_group_norm_bwd_saved_both_forms(cuda, n, ca, cb, groups, dims, act, acc):
    """gn_bwd_stats + gn_bwd_fold_apply (form 1, the plans' default at <= 64 channels per group) and gn_bwd_stats + gn_bwd_finalize +
    gn_bwd_apply (form 0), rowsum_n at N = 2, against fp64 autograd on the same bf16 x / dy / acc and fp32 ab / mr.  cs (form 1) against
    column sums of the STORED bf16 dx per row chunk.  Measured: dx at 1.00 x its bf16 floor (1.6e-3; worst element 0.50 of one ulp +
    allowance), dgamma / dbeta 2.7e-9 ... 2.0e-7, cs 0 ... 6.2e-9."""
    C = ca + cb
    DHW = dims[0] * dims[1] * dims[2]
    t = _gn_inputs(n, ca, cb, groups, dims, act, acc, seed=n * 7 + ca + 3 * cb + groups + act)
    dx_ref, dg_ref, db_ref, gg, xh, dx_def = _gn_reference(t, n, ca, cb, groups, dims, act)
    fold_ok = C // groups <= 64
    r = _L().ldm_op_group_norm_bwd_fold_chunks(n, C, groups, DHW)
    if not fold_ok:
        assert r == ERR_UNSUPPORTED
        sb = _L().ldm_op_group_norm_bwd_saved_scratch_bytes(n, C, DHW, groups)
        z = torch.zeros((sb // 4 + 64 + n * DHW * C,), device=cuda)
        assert _L().ldm_op_group_norm_bwd_saved(_p(z), _p(z), ca, None, 0, _p(z), _p(z), _p(z), groups, act, None, None, _p(z), None,
                                                _p(z), _p(z), None, n, DHW, 1, _p(z), sb, _s()) == ERR_UNSUPPORTED
    chunks, rpb = _fold_geom(n, C, DHW)
    if fold_ok:
        assert r == chunks, (r, chunks)
    # defects of the fp32 outputs: dgamma / dbeta with the last 32 rows of every sample skipped (a row-chunk end off by 32)
    keep = torch.ones(DHW, dtype=torch.bool)
    keep[-32:] = False
    gk = gg.reshape(n, C, DHW)[..., keep]
    xk = xh.reshape(n, C, DHW)[..., keep]
    dg_def, db_def = (gk * xk).sum((0, 2)), gk.sum((0, 2))
    what0 = f"gnb n={n} C={ca}+{cb} G={groups} {dims} act={act} acc={acc or '-'}"
    for form in ([0, 1] if fold_ok else [0]):
        dx, dg, db, *rest = _launch_gnb(cuda, t, n, ca, cb, groups, dims, act, form, chunks)
        what = f"{what0} form {form}"
        _gate_bf(dx.float(), _cl(dx_ref), what + " dx", _cl(dx_def), "xhat * mean(gamma g xhat) dropped")
        _gate32(dg[None], dg_ref[None], what + " dgamma", dg_def[None], "last 32 rows skipped")
        _gate32(db[None], db_ref[None], what + " dbeta", db_def[None], "last 32 rows skipped")
        if form == 1:
            cs = rest[0]
            cs_a = cs[:n * chunks * ca * 2].view(n, chunks, ca, 2)
            cs_b = cs[n * chunks * ca * 2:].view(n, chunks, cb, 2)
            assert torch.equal(cs_a[..., 1], torch.zeros_like(cs_a[..., 1])) and torch.equal(cs_b[..., 1], torch.zeros_like(cs_b[..., 1]))
            stored = dx.double().view(n, DHW, C)
            ref_cs = torch.stack([stored[:, j * rpb:(j + 1) * rpb].sum(1) for j in range(chunks)], 1)      # [N][chunks][C]
            def_cs = torch.stack([stored[:, j * rpb:min((j + 1) * rpb, DHW) - 32].sum(1) for j in range(chunks)], 1)
            got_cs = torch.cat([cs_a[..., 0], cs_b[..., 0]], 2)
            _gate32(got_cs, ref_cs, what + " cs", def_cs, "last 32 rows of each chunk skipped")


# ------------------------------------------------------------------------------------------------ column-sum finalize
def _colsum_case(cuda, descs, partial, out_len, seed):
    """descs: rows {partial_off, out_off, N, nslab, C, over_n, count, out_stride}; returns (single-launch results, batched result)"""
    pd = partial.to(cuda)
    ref = torch.full((out_len,), float("nan"), dtype=torch.float64)
    dfx = ref.clone()
    for (po, oo, N, ns, C, over, cnt, st) in descs:
        p = partial[po:po + N * ns * C * 2].double().view(N, ns, C, 2)[..., 0]
        if over:
            ref[oo:oo + cnt] = p.sum((0, 1))[:cnt]
            dfx[oo:oo + cnt] = p[:, :-1].sum((0, 1))[:cnt]
        else:
            for b in range(N):
                ref[oo + b * st:oo + b * st + cnt] = p[b].sum(0)[:cnt]
                dfx[oo + b * st:oo + b * st + cnt] = p[b, :-1].sum(0)[:cnt]
    written = ~torch.isnan(ref)
    res = {}
    for batched in (0, 1):
        runs = []
        for _ in range(2):
            out = _nan((out_len,), cuda)
            if batched:
                d = _i64(descs)
                wsb = _L().ldm_op_colsum_finalize_ws_bytes(d, len(descs))
                ws = torch.empty((wsb + 255) // 256 * 256, dtype=torch.uint8, device=cuda)
                _call("ldm_op_colsum_finalize", _p(pd), _p(out), d, len(descs), 1, _p(ws), ws.numel(), _s())
            else:
                for row in descs:
                    _call("ldm_op_colsum_finalize", _p(pd), _p(out), _i64([row]), 1, 0, None, 0, _s())
            torch.cuda.synchronize()
            runs.append(out.cpu())
        assert torch.equal(runs[0].nan_to_num(7.0), runs[1].nan_to_num(7.0)), "second launch differs"
        got = runs[0]
        assert torch.isnan(got[~written]).all(), "an entry outside [out_off, out_off + count) per row was written"
        res[batched] = got
        _gate32(got[written][None], ref[written][None], f"colsum batched={batched} descs={descs}", dfx[written][None], "last slab dropped")
    assert torch.equal(res[0][written], res[1][written]), "batched and single launches sum in different orders"


@pytest.mark.parametrize("N,nslab,C,over,count,stride", [
    (1, 7, 64, 1, 64, 0),        # bias gradient
    (2, 37, 96, 1, 40, 0),       # count % 16 != 0, summed over N
    (3, 5, 128, 0, 100, 130),    # per-sample rows (time embedding): out_stride > count, count % 16 != 0
    (1, 512, 64, 0, 64, 64),     # the slab cap of gn8_slabs
])
def test_colsum_finalize(cuda, N, nslab, C, over, count, stride):
    """colsum_finalize_kernel and colsum_finalize_batched_kernel (one descriptor) against fp64 sums of the same partials; the second
    entry of every pair is NaN and must be ignored.  Measured rel-L2 4.2e-8 ... 8.8e-8; the two forms are bit-identical."""
    g = torch.Generator().manual_seed(N * nslab + C)
    partial = torch.randn((N * nslab * C * 2,), generator=g) + 0.1
    partial.view(-1, 2)[:, 1] = float("nan")
    out_len = 3 + (count if over else (N - 1) * stride + count) + 5
    _colsum_case(cuda, [(0, 3, N, nslab, C, over, count, stride)], partial, out_len, 0)


def test_colsum_finalize_batched_mixed(cuda):
    """Four mixed descriptors (both modes, different N / nslab / C / count / stride) in one colsum_finalize_batched_kernel launch, each
    at its own offsets of one partial buffer and one output buffer.  Measured rel-L2 within 4.2e-8 ... 8.8e-8."""
    g = torch.Generator().manual_seed(11)
    rows, off = [], 0
    specs = [(2, 9, 64, 1, 64, 0), (2, 9, 64, 0, 60, 1280), (1, 33, 256, 1, 250, 0), (3, 4, 32, 0, 17, 40)]
    oo = [0, 70, 200, 600]
    for (N, ns, C, over, cnt, st), o in zip(specs, oo):
        rows.append((off, o, N, ns, C, over, cnt, st))
        off += N * ns * C * 2 + 6
    partial = torch.randn((off,), generator=g) + 0.05
    out_len = max(o + (cnt if over else (N - 1) * st + cnt) for (_, o, N, _, _, over, cnt, st) in rows) + 8
    _colsum_case(cuda, rows, partial, out_len, 0)


# ------------------------------------------------------------------------------------------------ weight-gradient export
def _export_ref(src, d):
    so, do_, ss, taps, rt, ld, ro, co, cout, cin, ns = d
    parts = [src[so + k * ss: so + k * ss + taps * rt * ld].double().view(taps, rt, ld)[:, ro:ro + cout, co:co + cin] for k in range(ns)]
    return parts, sum(parts).permute(1, 2, 0).reshape(-1)          # [cout][cin][taps]


def _export_run(cuda, descs, src, dst_len):
    sd = src.to(cuda)
    ref = torch.full((dst_len,), float("nan"), dtype=torch.float64)
    dfx = ref.clone()
    for d in descs:
        parts, r = _export_ref(src, d)
        n = r.numel()
        ref[d[1]:d[1] + n] = r
        dfx[d[1]:d[1] + n] = (sum(parts[:-1]) if len(parts) > 1 else parts[0] * 0).permute(1, 2, 0).reshape(-1)
    written = ~torch.isnan(ref)
    res = {}
    for batched in ([0, 1] if len(descs) == 1 else [1]):
        runs = []
        for _ in range(2):
            dst = _nan((dst_len,), cuda)
            dd = _i64(descs)
            if batched:
                wsb = _L().ldm_op_grad_export_ws_bytes(dd, len(descs))
                ws = torch.empty((wsb,), dtype=torch.uint8, device=cuda)
                _call("ldm_op_grad_export", _p(sd), _p(dst), dd, len(descs), 1, _p(ws), ws.numel(), _s())
            else:
                _call("ldm_op_grad_export", _p(sd), _p(dst), dd, 1, 0, None, 0, _s())
            torch.cuda.synchronize()
            runs.append(dst.cpu())
        assert torch.equal(runs[0].nan_to_num(7.0), runs[1].nan_to_num(7.0)), "second launch differs"
        got = runs[0]
        assert torch.isnan(got[~written]).all(), "an entry outside the exported parameters was written"
        res[batched] = got
        what = f"grad_export batched={batched} descs={descs}"
        if all(d[10] == 1 for d in descs):
            assert torch.equal(got[written].double(), ref[written]), what + ": nsplit 1 must move the values bit for bit"
            print(f"{what}: bit-identical")
        else:
            _gate32(got[written][None], ref[written][None], what, dfx[written][None], "last slab dropped")
    if len(res) == 2:
        assert torch.equal(res[0].nan_to_num(7.0), res[1].nan_to_num(7.0))


@pytest.mark.parametrize("taps,rt,ld,ro,co,cout,cin,ns", [
    (27, 64, 96, 0, 0, 64, 96, 1),       # cin = 96: the second 64-channel chunk is ragged
    (27, 64, 96, 0, 0, 64, 96, 3),       # three voxel-split slabs folded in order
    (27, 160, 192, 96, 64, 64, 96, 3),   # a slice: rows 96.., columns 64.. (row_off, col_off)
    (1, 1, 256, 0, 40, 1, 200, 1),       # bias export: one row, columns 40.. (export_bias)
    (1, 128, 256, 32, 0, 96, 130, 2),    # 1x1 conv
])
def test_grad_export(cuda, taps, rt, ld, ro, co, cout, cin, ns):
    """grad_export_kernel and grad_export_batched_kernel (one descriptor): nsplit 1 bit-identical (pure data movement), nsplit > 1 against
    fp64 sums of the slabs.  Measured: nsplit 1 bit-identical; nsplit 2 / 3 rel-L2 2.7e-8 ... 3.5e-8; the two forms bit-identical."""
    g = torch.Generator().manual_seed(taps + rt + ld + ro + co + ns)
    ss = taps * rt * ld + 40
    src = torch.randn((ss * ns + 17,), generator=g)
    d = (5, 11, ss, taps, rt, ld, ro, co, cout, cin, ns)
    _export_run(cuda, [d], src, 11 + cout * cin * taps + 9)


def test_grad_export_batched_mixed(cuda):
    """Three descriptors (taps 27 / 1, nsplit 1 / 2 / 3, slices) in one grad_export_batched_kernel launch.  Measured rel-L2 <= 3.5e-8."""
    g = torch.Generator().manual_seed(3)
    src = torch.randn((700000,), generator=g)
    descs = [(0, 0, 27 * 64 * 96, 27, 64, 96, 0, 0, 64, 96, 3),
             (500000, 27 * 64 * 96 + 5, 0, 1, 1, 256, 0, 40, 1, 200, 1),
             (520000, 27 * 64 * 96 + 300, 27 * 32 * 64 + 8, 27, 32, 64, 16, 32, 16, 32, 2)]
    _export_run(cuda, descs, src, 27 * 64 * 96 + 300 + 16 * 32 * 27 + 10)


# ------------------------------------------------------------------------------------------------ batched flip-transpose (bf16)
def _wt_ref(w, d):
    wo, wto, k, cout, cout_pad, cin, ci_off, ci_cnt = d
    taps = k ** 3
    rows, cols = rup(ci_cnt, 64), rup(cout, 32)
    src = w[wo:wo + taps * cout_pad * cin].view(taps, cout_pad, cin)
    out = torch.zeros((taps, rows, cols), dtype=torch.bfloat16)
    out[:, :ci_cnt, :cout] = src.flip(0)[:, :cout, ci_off:ci_off + ci_cnt].transpose(1, 2)
    return out.reshape(-1)


@pytest.mark.parametrize("descs", [
    [(0, 0, 3, 64, 64, 128, 0, 128)],                                  # whole weight, one descriptor
    [(0, 0, 3, 96, 128, 768, 0, 512), (0, 27 * 512 * 96, 3, 96, 128, 768, 512, 256)],   # two sources of a 512 + 256 conv (ci_off / ci_cnt)
    [(0, 0, 3, 40, 64, 96, 0, 96), (27 * 64 * 96, 27 * 128 * 64, 1, 200, 256, 72, 8, 40),
     (27 * 64 * 96 + 256 * 72, 27 * 128 * 64 + 64 * 224, 3, 8, 64, 32, 0, 32)],       # three mixed: cout 40 / 200 / 8, ragged slices
])
def test_weight_flip_transpose_batched(cuda, descs):
    """weight_flip_transpose_batched_kernel (bf16) over k descriptors in one launch: bit-identical to torch's flip / transpose, rows >=
    ci_cnt and columns >= cout exactly zero; rows cout .. cout_pad of the source (NaN here) never read.  Single full-cin descriptors are
    also bit-identical to ldm_op_weight_flip_transpose (the per-conv kernel of OP_WT)."""
    g = torch.Generator().manual_seed(len(descs))
    wlen = max(d[0] + d[2] ** 3 * d[4] * d[5] for d in descs)
    w = torch.randn((wlen,), generator=g).to(torch.bfloat16)
    for d in descs:                                                     # padding rows of the source: must not leak
        wo, _, k, cout, cout_pad, cin = d[:6]
        w[wo:wo + k ** 3 * cout_pad * cin].view(k ** 3, cout_pad, cin)[:, cout:] = float("nan")
    wd = w.to(cuda)
    refs = [_wt_ref(w, d) for d in descs]
    wtlen = max(d[1] + r.numel() for d, r in zip(descs, refs)) + 64
    dd = _i64(descs)
    wsb = _L().ldm_op_weight_flip_transpose_batched_ws_bytes(dd, len(descs))
    runs = []
    for _ in range(2):
        wt = _nan((wtlen,), cuda, torch.bfloat16)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=cuda)
        _call("ldm_op_weight_flip_transpose_batched", _p(wd), _p(wt), dd, len(descs), _p(ws), ws.numel(), _s())
        torch.cuda.synchronize()
        runs.append(wt.cpu())
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16)), "second launch differs"
    for d, r in zip(descs, refs):
        got = runs[0][d[1]:d[1] + r.numel()]
        assert torch.equal(got.view(torch.int16), r.view(torch.int16)), f"flip-transpose {d} differs from torch"
        if d[6] == 0 and d[7] == d[5]:
            wt1 = _nan((r.numel(),), cuda, torch.bfloat16)
            _call("ldm_op_weight_flip_transpose", _p(wd[d[0]:]), _p(wt1), d[2], d[3], d[4], d[5], _s())
            torch.cuda.synchronize()
            assert torch.equal(wt1.cpu().view(torch.int16), got.view(torch.int16)), "batched and per-conv kernels differ"
    print(f"weight_flip_transpose_batched {descs}: bit-identical")


# ------------------------------------------------------------------------------------------------ Linear backward (time embedding)
@pytest.mark.parametrize("B,I,O,silu,dys,xs", [
    (1, 512, 6400, 1, 6400, 512),     # the stacked time_emb_proj of the benchmark UNet: nz = 64
    (3, 512, 1000, 1, 1008, 520),     # nz = 15, last slice ragged (1000 = 14 x 67 + 62); strides > O / I
    (3, 128, 32, 0, 32, 128),         # nz = 1
    (1, 128, 512, 1, 512, 136),       # the MLP's second layer: nz = 8
])
def test_linear_bwd(cuda, B, I, O, silu, dys, xs):
    """linear_bwd_dx_part + linear_bwd_dx_fold (with the plan's nz) and linear_bwd_dw against fp64 autograd of W act(x) + b on the same
    bf16 W.  Measured rel-L2 0 ... 2.5e-7 over dx, dW and db."""
    nz = _L().ldm_op_linear_bwd_nz(O)
    assert nz == max(1, min(64, O // 64))
    g = torch.Generator().manual_seed(B * I + O + silu)
    W = (torch.randn((O, I), generator=g) / I ** 0.5).to(torch.bfloat16)
    dy = torch.randn((B, dys), generator=g)
    xp = torch.randn((B, xs), generator=g)
    x64 = xp[:, :I].double().requires_grad_(True)
    W64 = W.double().requires_grad_(True)
    b64 = torch.zeros(O, dtype=torch.float64, requires_grad=True)
    y = (F.silu(x64) if silu else x64) @ W64.t() + b64
    y.backward(dy[:, :O].double())
    per = (O + nz - 1) // nz
    o_last = (nz - 1) * per
    xd = x64.detach().clone().requires_grad_(True)                  # defect: the last nz slice dropped
    ((F.silu(xd) if silu else xd) @ W64.detach()[:o_last].t()).backward(dy[:, :o_last].double())
    Wd, dyd, xpd = W.to(cuda), dy.to(cuda), xp.to(cuda)
    runs = []
    for _ in range(2):
        dx = _nan((B, xs), cuda)
        dW, db = _nan((O, I), cuda), _nan((O,), cuda)
        part = _nan((nz * B * I,), cuda)
        _call("ldm_op_linear_bwd", _p(Wd), _p(dyd), _p(xpd), _p(dx), _p(dW), _p(db), B, I, O, dys, xs, silu, _p(part), part.numel() * 4, _s())
        torch.cuda.synchronize()
        runs.append((dx.cpu(), dW.cpu(), db.cpu()))
    for a_, b_ in zip(runs[0], runs[1]):
        assert torch.equal(a_.nan_to_num(7.0), b_.nan_to_num(7.0)), "second launch differs"
    dx, dW, db = runs[0]
    assert torch.isnan(dx[:, I:]).all(), "dx written past I in a strided row"
    what = f"linear_bwd B={B} I={I} O={O} nz={nz} silu={silu}"
    _gate32(dx[:, :I], x64.grad, what + " dx", xd.grad, "last nz slice dropped")
    # dW defect: the last batch row dropped (B > 1) or the SiLU of the input left out (B == 1)
    xa = F.silu(x64.detach()) if silu else x64.detach()
    dW_def = dy[:B - 1, :O].double().t() @ xa[:B - 1] if B > 1 else dy[:, :O].double().t() @ (x64.detach() if silu else 0.5 * xa)
    _gate32(dW, W64.grad, what + " dW", dW_def, "a batch row dropped" if B > 1 else "act(x) replaced")
    _gate32(db[None], b64.grad[None], what + " db")


# ------------------------------------------------------------------------------------------------ sumpool2 / add_bf16
def test_upsample_bwd_exact_sums(cuda):
    """sumpool2_kernel on inputs whose 8-term fp32 sums are exact (integers times 2^-6, |v| <= 127): the bf16 output must equal torch's
    round-to-nearest-even of the exact sum bit for bit (the sums need up to 10 significant bits, so most of them round)."""
    g = torch.Generator().manual_seed(2)
    n, C, dims = 2, 64, (3, 5, 2)
    dy = (torch.randint(-127, 128, (n, C, *(2 * s for s in dims)), generator=g).double() * 2.0 ** -6)
    x = torch.zeros((n, C, *dims), dtype=torch.float64, requires_grad=True)
    F.interpolate(x, scale_factor=2.0, mode="nearest").backward(dy)
    ref = _cl(x.grad).to(torch.bfloat16)
    dyd = _dev_bf(dy, cuda)
    runs = []
    for _ in range(2):
        dx = _nan((n * dims[0] * dims[1] * dims[2], C), cuda, torch.bfloat16)
        _call("ldm_op_upsample_bwd", _p(dyd), _p(dx), n, *dims, C, _s())
        torch.cuda.synchronize()
        runs.append(dx.cpu())
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16))
    rounded = int((_cl(x.grad) != ref.double()).sum())
    assert rounded > 0
    assert torch.equal(runs[0].view(torch.int16), ref.view(torch.int16)), "sumpool2 differs from RNE of the exact sum"
    print(f"upsample_bwd exact sums: bit-identical ({rounded} of {ref.numel()} outputs needed rounding)")


@pytest.mark.parametrize("n,C,dims", [(1, 64, (3, 4, 5)), (2, 96, (5, 3, 2)), (1, 512, (3, 3, 3))])
def test_upsample_bwd(cuda, n, C, dims):
    """sumpool2_kernel on general bf16 gradients against fp64 autograd of F.interpolate(nearest, x2).  Measured: 1.00 x the bf16 floor
    (1.6e-3), worst element 0.50 ulp."""
    g = torch.Generator().manual_seed(n * C)
    dy = _bfr(torch.randn((n, C, *(2 * s for s in dims)), generator=g))
    x = torch.zeros((n, C, *dims), dtype=torch.float64, requires_grad=True)
    F.interpolate(x, scale_factor=2.0, mode="nearest").backward(dy)
    ref = _cl(x.grad)
    xd_ = torch.zeros_like(x).requires_grad_(True)                   # defect: only 7 of the 8 fine voxels (the last one dropped)
    dy7 = dy.clone()
    dy7[:, :, 1::2, 1::2, 1::2] = 0
    F.interpolate(xd_, scale_factor=2.0, mode="nearest").backward(dy7)
    dyd = _dev_bf(dy, cuda)
    runs = []
    for _ in range(2):
        dx = _nan((n * dims[0] * dims[1] * dims[2], C), cuda, torch.bfloat16)
        _call("ldm_op_upsample_bwd", _p(dyd), _p(dx), n, *dims, C, _s())
        torch.cuda.synchronize()
        runs.append(dx.cpu())
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16))
    _gate_bf(runs[0].float(), ref, f"upsample_bwd n={n} C={C} {dims}", _cl(xd_.grad), "one fine voxel dropped")


def test_add_bf16(cuda):
    """add_bf16_kernel: bit-identical to torch's bf16(a + b) (two bf16 values sum exactly in fp32), with exact ties that must round to
    even placed at the front."""
    g = torch.Generator().manual_seed(4)
    n = 8 * 1000
    a = torch.randn((n,), generator=g).to(torch.bfloat16)
    b = torch.randn((n,), generator=g).to(torch.bfloat16)
    ties = [(1.0, 2.0 ** -8), (1.0 + 2.0 ** -7, 2.0 ** -8), (-3.0, -2.0 ** -7), (1.5, 2.0 ** -9 + 2.0 ** -17)]
    for j, (u, v) in enumerate(ties):
        a[j], b[j] = u, v
    ref = (a.double() + b.double()).to(torch.bfloat16)
    assert ref[0] == 1.0 and ref[1] == 1.0 + 2.0 ** -6
    ad, bd = a.to(cuda), b.to(cuda)
    runs = []
    for _ in range(2):
        out = _nan((n,), cuda, torch.bfloat16)
        _call("ldm_op_add_bf16", _p(ad), _p(bd), _p(out), n, _s())
        torch.cuda.synchronize()
        runs.append(out.cpu())
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16))
    assert torch.equal(runs[0].view(torch.int16), ref.view(torch.int16)), "add_bf16 differs from RNE of the exact sum"
    print("add_bf16: bit-identical")


# ------------------------------------------------------------------------------------------------ AutoencoderKL heads
LV_SPECIAL = [-30.0, 20.0, -30.5, 20.5, -29.98, 19.98, -31.0, 25.0]


def _heads_inputs(N, L, DHW, seed):
    g = torch.Generator().manual_seed(seed)
    ml = torch.randn((N, 2 * L, DHW), generator=g)
    ml[:, L:] = 2.0 * torch.randn((N, L, DHW), generator=g)
    mu, lv = ml[:, :L].reshape(-1), ml[:, L:].reshape(-1)
    eps = torch.randn((N, L, DHW), generator=g)
    for j, v in enumerate(LV_SPECIAL):                            # the clamp bounds exactly, just inside, just outside; mu = 0 and
        lv[7 * j + 3], mu[7 * j + 3] = v, 0.0                     # eps = 1 there, so that z - mu = sigma survives fp32 even at lv = -30
        eps.view(-1)[7 * j + 3] = 1.0
    ml[:, :L], ml[:, L:] = mu.view(N, L, DHW), lv.view(N, L, DHW)
    return ml, eps


def test_vae_heads(cuda):
    """vae_heads_kernel: mu, sigma = exp(0.5 clamp(lv, -30, 20)), z = mu + sigma eps against fp64, with lv at and around both bounds.
    Measured rel-L2: sigma 4.2e-8, z 4.2e-8 (mu is copied exactly)."""
    N, L, DHW = 2, 3, 6 * 5 * 7
    ml, eps = _heads_inputs(N, L, DHW, 1)
    m64, lv64 = ml[:, :L].double(), ml[:, L:].double()
    sg = torch.exp(0.5 * lv64.clamp(-30, 20))
    z = m64 + sg * eps.double()
    sg_def = torch.exp(0.5 * lv64.clamp(-30, 19.5))               # defect: the upper clamp bound misplaced
    mld, epsd = ml.to(cuda), eps.to(cuda)
    runs = []
    for _ in range(2):
        mu, sigma, zz = _nan((N, L, DHW), cuda), _nan((N, L, DHW), cuda), _nan((N, L, DHW), cuda)
        _call("ldm_op_vae_heads", _p(mld), _p(epsd), _p(mu), _p(sigma), _p(zz), N, L, DHW, _s())
        torch.cuda.synchronize()
        runs.append((mu.cpu(), sigma.cpu(), zz.cpu()))
    for a_, b_ in zip(runs[0], runs[1]):
        assert torch.equal(a_, b_)
    mu, sigma, zz = runs[0]
    assert torch.equal(mu, ml[:, :L])
    _gate32(sigma, sg, "vae_heads sigma", sg_def, "clamp at 19.5")
    _gate32(zz, z, "vae_heads z", m64 + sg_def * eps.double(), "clamp at 19.5")


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("kl", [False, True])
def test_vae_heads_bwd(cuda, fp32, kl):
    """vae_heads_bwd_kernel<bf16_t | float> against fp64 autograd of mu + exp(0.5 clamp(lv, -30, 20)) eps (eps recovered from the forward's
    fp32 z, as the kernel does) plus the KL-term gradients g_mu / g_sigma (null or set).  lv sits exactly on both clamp bounds, just inside
    and just outside: torch.clamp passes the gradient on the closed interval [-30, 20], so the bound elements must carry it and the
    elements outside must be exactly zero.  L = 3 in Cs = 32 stored channels (padding exactly zero), dz with Ls = 32.  Measured: bf16
    storage at 1.00 x its floor, fp32 storage rel-L2 3.6e-8; the bound elements within 0.2 % (bf16) / 1e-7 (fp32) of torch.  Before the
    kernel's clamp interval was closed this test failed: d_lv = 0 on lv = -30 and lv = 20."""
    N, L, DHW, Cs, Ls = 2, 3, 5 * 4 * 7, 32, 32
    ml, eps = _heads_inputs(N, L, DHW, 2 + fp32 + 2 * kl)
    g = torch.Generator().manual_seed(9)
    lvc = ml[:, L:].clamp(-30, 20)
    z = (ml[:, :L] + torch.exp(0.5 * lvc) * eps).float()           # what the forward kernel keeps (fp32)
    dz = torch.randn((N * DHW, Ls), generator=g)
    if not fp32:
        dz = dz.to(torch.bfloat16).float()
    g_mu = torch.randn((N, L, DHW), generator=g) if kl else None
    g_sg = torch.randn((N, L, DHW), generator=g) if kl else None
    mu64 = ml[:, :L].double().requires_grad_(True)
    lv64 = ml[:, L:].double().requires_grad_(True)
    sig_fix = torch.exp(0.5 * ml[:, L:].double().clamp(-30, 20))
    eps_eff = (z.double() - ml[:, :L].double()) / sig_fix
    sig = torch.exp(0.5 * lv64.clamp(-30, 20))
    zz = mu64 + sig * eps_eff
    dzc = dz[:, :L].double().view(N, DHW, L).permute(0, 2, 1)
    loss = (dzc * zz).sum() + ((g_mu.double() * mu64).sum() + (g_sg.double() * sig).sum() if kl else 0.0)
    loss.backward()
    ref = torch.zeros((N * DHW, Cs), dtype=torch.float64)
    ref[:, :L] = mu64.grad.permute(0, 2, 1).reshape(-1, L)
    ref[:, L:2 * L] = lv64.grad.permute(0, 2, 1).reshape(-1, L)
    # defect: the open interval (-30, 20) of the kernel before it matched torch.clamp
    lvf = ml[:, L:].permute(0, 2, 1).reshape(-1, L)
    dfx = ref.clone()
    dfx[:, L:2 * L][(lvf == -30.0) | (lvf == 20.0)] = 0.0
    dt = torch.float32 if fp32 else torch.bfloat16
    dzd = dz.to(dt).to(cuda)
    mld, zd = ml.to(cuda), z.to(cuda)
    gmd, gsd = (g_mu.to(cuda), g_sg.to(cuda)) if kl else (None, None)
    runs = []
    for _ in range(2):
        dy = _nan((N * DHW, Cs), cuda, dt)
        _call("ldm_op_vae_heads_bwd", _p(dzd), Ls, _p(mld), _p(zd), _p(gmd), _p(gsd), _p(dy), N, L, Cs, DHW, fp32, _s())
        torch.cuda.synchronize()
        runs.append(dy.cpu().float())
    assert torch.equal(runs[0], runs[1])
    got = runs[0]
    assert torch.equal(got[:, 2 * L:], torch.zeros_like(got[:, 2 * L:])), "padding channels must be exactly zero"
    what = f"vae_heads_bwd {'fp32' if fp32 else 'bf16'}{' +kl' if kl else ''}"
    # tensor-wide gates on the ordinary elements (the special lv positions carry gradients from 1e-7 to 1e4, which would swamp them);
    # defect there: d_lv without its factor 0.5
    special = torch.zeros_like(ref, dtype=torch.bool)
    special[:, L:2 * L] = torch.isin(lvf, torch.tensor(LV_SPECIAL, dtype=lvf.dtype))
    special[:, :L] = special[:, L:2 * L]
    g0, r0 = got[:, :2 * L].double().masked_fill(special[:, :2 * L], 0), ref[:, :2 * L].masked_fill(special[:, :2 * L], 0)
    d0 = r0.clone()
    d0[:, L:] *= 2
    if fp32:
        _gate32(g0, r0, what, d0, "d_lv without 0.5")
    else:
        _gate_bf(g0, r0, what, d0, "d_lv without 0.5")
    # the special elements on their own: on the bounds the gradient must match torch.clamp's (closed interval), outside it is zero
    on = (lvf == -30.0) | (lvf == 20.0)
    out = (lvf < -30.0) | (lvf > 20.0)
    assert on.sum() >= 2 and out.sum() >= 2
    rtol = 1e-5 if fp32 else 2.0 ** -8

    def bounds_ok(t):
        gl, rl = t[:, L:2 * L].double(), ref[:, L:2 * L]
        return bool(((gl[on] - rl[on]).abs() <= rtol * rl[on].abs()).all() and (gl[out] == 0).all())
    assert (ref[:, L:2 * L][on] != 0).all() and (ref[:, L:2 * L][out] == 0).all()
    assert not bounds_ok(dfx), "the bound check cannot see the open clamp interval"
    print(f"{what}: d_lv on the clamp bounds {got[:, L:2 * L][on].tolist()} vs torch {ref[:, L:2 * L][on].tolist()}; "
          f"defect 'open clamp interval' gives {dfx[:, L:2 * L][on].tolist()}")
    assert bounds_ok(got), (what, "clamp-bound gradients differ from torch.clamp's")


# ------------------------------------------------------------------------------------------------ argument checks
def test_bad_arguments_are_refused_before_the_device(cuda):
    """Argument checks return LDM_ERR_BAD_ARG (-1) / LDM_ERR_WORKSPACE (-5) without launching anything."""
    L = _L()
    x = torch.zeros(1 << 16, device=cuda)
    s = _s()
    sb = L.ldm_op_group_norm_bwd_saved_scratch_bytes(1, 64, 8, 32)
    gnb = L.ldm_op_group_norm_bwd_saved
    assert gnb(None, _p(x), 64, None, 0, _p(x), _p(x), _p(x), 32, 1, None, None, _p(x), None, _p(x), _p(x), None, 1, 8, 0, _p(x), sb, s) == -1
    assert gnb(_p(x), _p(x), 60, None, 0, _p(x), _p(x), _p(x), 30, 1, None, None, _p(x), None, _p(x), _p(x), None, 1, 8, 0, _p(x), sb, s) == -1  # ca % 8
    assert gnb(_p(x), _p(x), 64, _p(x), 12, _p(x), _p(x), _p(x), 4, 1, None, None, _p(x), _p(x), _p(x), _p(x), None, 1, 8, 0, _p(x), 1 << 20,
               s) == -1                                                                                                            # cb % 8
    assert gnb(_p(x), _p(x), 64, _p(x), 64, _p(x), _p(x), _p(x), 32, 1, None, None, _p(x), None, _p(x), _p(x), None, 1, 8, 0, _p(x), 1 << 20,
               s) == -1                                                                                                            # no dxb
    assert gnb(_p(x), _p(x), 64, None, 0, _p(x), _p(x), _p(x), 32, 1, None, None, _p(x), None, _p(x), _p(x), _p(x), 1, 8, 0, _p(x), sb, s) == -1  # cs, form 0
    assert gnb(_p(x), _p(x), 64, None, 0, _p(x), _p(x), _p(x), 32, 3, None, None, _p(x), None, _p(x), _p(x), None, 1, 8, 0, _p(x), sb, s) == -1  # act 3
    assert gnb(_p(x), _p(x), 64, None, 0, _p(x), _p(x), _p(x), 32, 1, None, None, _p(x), None, _p(x), _p(x), None, 1, 8, 0, _p(x), sb - 4,
               s) == ERR_WORKSPACE
    assert L.ldm_op_group_norm_bwd_fold_chunks(1, 60, 30, 8) == -1
    d1 = _i64([(0, 0, 1, 4, 64, 1, 64, 0)])
    assert L.ldm_op_colsum_finalize(_p(x), _p(x), d1, 0, 1, _p(x), 1 << 16, s) == -1                                    # k = 0
    assert L.ldm_op_colsum_finalize(_p(x), _p(x), _i64([(0, 0, 1, 4, 64, 1, 65, 0)]), 1, 0, None, 0, s) == -1          # count > C
    assert L.ldm_op_colsum_finalize(_p(x), _p(x), _i64([(0, 0, 2, 4, 64, 0, 64, 32)]), 1, 0, None, 0, s) == -1         # stride < count
    assert L.ldm_op_colsum_finalize(_p(x), _p(x), _i64([(0, 0, 1, 4, 64, 1, 64, 0)] * 2), 2, 0, None, 0, s) == -1      # k = 2 single
    assert L.ldm_op_colsum_finalize(_p(x), _p(x), d1, 1, 1, _p(x), 16, s) == ERR_WORKSPACE
    e1 = (0, 0, 0, 27, 64, 96, 0, 0, 64, 96, 1)
    assert L.ldm_op_grad_export(_p(x), _p(x), _i64([e1]), 0, 1, _p(x), 1 << 16, s) == -1                               # k = 0
    assert L.ldm_op_grad_export(_p(x), _p(x), _i64([(0, 0, 0, 28, 64, 96, 0, 0, 64, 96, 1)]), 1, 0, None, 0, s) == -1  # taps > 27
    assert L.ldm_op_grad_export(_p(x), _p(x), _i64([(0, 0, 0, 27, 64, 96, 0, 8, 64, 96, 1)]), 1, 0, None, 0, s) == -1  # col_off + cin > ld
    assert L.ldm_op_grad_export(_p(x), _p(x), _i64([(0, 0, 100, 27, 64, 96, 0, 0, 64, 96, 2)]), 1, 0, None, 0, s) == -1  # slabs overlap
    assert L.ldm_op_grad_export(_p(x), _p(x), _i64([e1]), 1, 1, _p(x), 8, s) == ERR_WORKSPACE
    w1 = (0, 0, 3, 64, 64, 128, 64, 96)                                                                                # slice past cin
    assert L.ldm_op_weight_flip_transpose_batched(_p(x), _p(x), _i64([w1]), 1, _p(x), 1 << 16, s) == -1
    assert L.ldm_op_weight_flip_transpose_batched(_p(x), _p(x), _i64([(0, 0, 3, 64, 32, 128, 0, 128)]), 1, _p(x), 1 << 16, s) == -1  # cout_pad < cout
    assert L.ldm_op_weight_flip_transpose_batched(_p(x), _p(x), _i64([(0, 0, 3, 64, 64, 128, 0, 128)]), 0, _p(x), 1 << 16, s) == -1  # k = 0
    assert L.ldm_op_weight_flip_transpose_batched(_p(x), _p(x), _i64([(0, 0, 3, 64, 64, 128, 0, 128)]), 1, _p(x), 64, s) == ERR_WORKSPACE
    assert L.ldm_op_linear_bwd(_p(x), _p(x), _p(x), _p(x), None, None, 1, 64, 64, 32, 64, 1, _p(x), 1 << 16, s) == -1  # dy_stride < O
    assert L.ldm_op_linear_bwd(None, _p(x), _p(x), _p(x), None, None, 1, 64, 64, 64, 64, 1, _p(x), 1 << 16, s) == -1   # dx without W
    assert L.ldm_op_linear_bwd(_p(x), _p(x), _p(x), _p(x), None, None, 2, 64, 6400, 6400, 64, 1, _p(x), 4 * 64 * 64, s) == ERR_WORKSPACE
    assert L.ldm_op_upsample_bwd(_p(x), _p(x), 1, 2, 2, 2, 12, s) == -1                                               # C % 8
    assert L.ldm_op_add_bf16(_p(x), _p(x), _p(x), 12, s) == -1                                                        # n % 8
    assert L.ldm_op_add_bf16(_p(x), x.data_ptr() + 2, _p(x), 16, s) == -1                                             # unaligned
    assert L.ldm_op_vae_heads(None, None, _p(x), None, None, 1, 3, 8, s) == -1
    assert L.ldm_op_vae_heads_bwd(_p(x), 2, _p(x), _p(x), None, None, _p(x), 1, 3, 32, 8, 0, s) == -1                 # Ls < L
    assert L.ldm_op_vae_heads_bwd(_p(x), 32, _p(x), _p(x), None, None, _p(x), 1, 3, 4, 8, 0, s) == -1                 # Cs < 2L
    torch.cuda.synchronize()
