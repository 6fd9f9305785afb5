"""Per-kernel parity of the kernels that only the launch plans run (-m gpu): conv3_thin_kernel (bf16 and 3 x bf16 form), the time
embedding (temb_sinusoid_kernel, gemv_bf16_kernel, gemv_f32_kernel), the input packing (pack2 / guided pack2 / im2col / guided im2col)
and the derived weights (phase, im2col, x3, x3 phase) with the (hi | lo) operand split.  Each is called through its ldm_op_* entry,
which launches through the helper the plan executor, ensure_derived and ensure_temb_table use, and is compared with plain torch on the
CPU in float64 (numeric kernels) or with a bit-exact torch construction (layout kernels).

Why operator level: these kernels have no other entry, so the only gates on them were whole-network ones at the bf16 noise floor or
comparisons of two plans with each other.

Gates: TOL = 1e-5 rel-L2 for fp32 outputs of exact-product kernels, TOL_X3 = 3e-5 for the 3 x bf16 form, and per element
max |got - ref| <= 10 tol rms(ref) (rows here hold 1 .. 4 channels, so a per-row norm says nothing).  Every numeric gate also shows, on
the CPU, that one named plausible defect lands more than 10x outside it.  Outputs and workspaces are NaN-filled before the launch and
must come back finite, padding exactly zero, elements outside the written range still NaN, and a second launch bit-identical.
Measured values are printed (-s) and quoted in each test's docstring.
"""
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from util import pack_conv_weight, rup, to_ndhwc_bf16

pytestmark = pytest.mark.gpu
TOL = 1e-5
TOL_X3 = 3e-5
ERR_BAD_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -5
GUARD = 64                      # elements behind every output that must stay NaN
OP_CONV_THIN = 39               # enum OpKind, as tools/plan_trace.py's KINDS


def _lib():
    from ldm3d import _lib
    return _lib


def _call(name, *args):
    _lib().check(getattr(_lib().lib(), name)(*args))


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(n, cuda, dtype=torch.float32):
    """n elements + GUARD, all NaN."""
    return torch.full((n + GUARD,), float("nan"), dtype=dtype, device=cuda)


def _take(buf, n):
    """The n written elements on the CPU; everything behind them must still be NaN."""
    torch.cuda.synchronize()
    b = buf.cpu()
    assert torch.isnan(b[n:].float()).all(), "wrote past the end of its output"
    return b[:n]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(got, want, what):
    g, w = _bits(got.reshape(-1)), _bits(want.reshape(-1))
    bad = int((g != w).sum())
    print(f"{what}: {g.numel()} elements, {bad} differ")
    assert bad == 0, (what, bad, torch.nonzero(g != w)[:4].flatten().tolist())


def _errs(got, ref):
    """(rel-L2, max |got - ref| / rms(ref)) in float64."""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    rms = float(ref.pow(2).mean().sqrt())
    return float((got - ref).norm() / ref.norm()), float((got - ref).abs().max()) / rms


def _gate(got, ref, tol, what, defect, defect_name):
    """rel-L2 <= tol and max element error <= 10 tol rms(ref); `defect` (a plausible wrong result, CPU) is > 10x outside both."""
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    e, m = _errs(got, ref)
    de, dm = _errs(defect, ref)
    print(f"{what}: rel-L2 {e:.2e} (gate {tol:.0e}), max element {m:.2e} rms (gate {10 * tol:.0e}); {defect_name}: {de:.1e} / {dm:.1e} rms")
    assert e <= tol, (what, e)
    assert m <= 10 * tol, (what, m)
    assert de > 10 * tol and dm > 10 * 10 * tol, (what, "the gate cannot see: " + defect_name, de, dm)
    return e, m


# ------------------------------------------------------------------------------------------------ thin conv
# N, Cin, CoutReal, (D, H, W), bias
THIN_CASES = [(1, 32, 1, (4, 4, 16), True),       # one block, one channel chunk
              (2, 64, 4, (5, 6, 17), True),       # ragged in all three dimensions (2 x 2 x 2 blocks), two samples
              (1, 128, 3, (3, 2, 9), True),       # volume smaller than a block, four chunks, weight row 3 unused
              (1, 96, 2, (8, 8, 32), True),       # blocks whose halo is all interior, three chunks
              (1, 64, 1, (5, 6, 17), False)]      # bias == nullptr
COUT_PAD = 64


def _thin_inputs(n, cin, cout, dims, bias, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, cin, *dims), generator=g)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g) / (27 * cin) ** 0.5
    b = 0.1 * torch.randn((cout,), generator=g) if bias else None
    return x, w, b


def _clamped_high_w(x, w, b):
    """The defect: the halo column behind the last w holds the last column instead of zero."""
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    xp[..., 1:-1, 1:-1, -1] = x[..., -1]
    return F.conv3d(xp, w, b)


@pytest.mark.parametrize("n,cin,cout,dims,bias", THIN_CASES)
def test_thin_conv_bf16_against_fp64(cuda, n, cin, cout, dims, bias):
    """conv3_thin_kernel on bf16 operands vs F.conv3d in float64 on exactly those operands.
    Measured (MI355X): rel-L2 <= 3.0e-7 and <= 2.5e-6 rms per element over the five cases (gates 1e-5 / 1e-4); on the CPU the clamped
    high-W halo sits at >= 0.097 rel-L2 and >= 1.1 rms.  Pad weight rows 0 vs 3.0: same bits; second launch: same bits."""
    x, w, b = _thin_inputs(n, cin, cout, dims, bias, 100 + cin + cout)
    xb, wb = x.to(torch.bfloat16), w.to(torch.bfloat16)
    ref = F.conv3d(xb.double(), wb.double(), None if b is None else b.double(), padding=1)
    defect = _clamped_high_w(xb.double(), wb.double(), None if b is None else b.double())
    xd = to_ndhwc_bf16(xb.float(), cin).to(cuda)
    bd = None if b is None else b.to(cuda)
    outs = []
    for fill in (0.0, 3.0, 0.0):
        wp = pack_conv_weight(wb.float(), cin, COUT_PAD)
        wp[:, cout:] = fill
        wd = wp.to(cuda)
        out = _nan(ref.numel(), cuda)
        _call("ldm_op_conv3d_thin", _p(xd), cin, _p(wd), _p(bd), _p(out), n, *dims, cout, COUT_PAD, _stream())
        outs.append(_take(out, ref.numel()).reshape(ref.shape))
    _gate(outs[0], ref, TOL, f"thin conv bf16 N{n} Cin{cin} Cout{cout} {dims}", defect, "high-W halo clamped")
    assert torch.equal(outs[0], outs[1]), "weight rows >= CoutReal are read"
    assert torch.equal(outs[0], outs[2]), "second launch differs"


@pytest.mark.parametrize("n,cin,cout,dims,bias", [(n, {96: 64}.get(cin, cin), co, d, b) for n, cin, co, d, b in THIN_CASES])
def test_thin_conv_fp32_form_against_fp64(cuda, n, cin, cout, dims, bias):
    """The chain the fp32 plans run (split of x, [hi | lo | hi] weights, conv3_thin_kernel with x3_c) vs float64 on the unrounded fp32 inputs.
    The five shapes of the bf16 test with Cin 32 / 64 / 128 (64 where that one has 96).
    Measured (MI355X): rel-L2 <= 5.0e-6, <= 1.9e-5 rms per element (gates 3e-5 / 3e-4); on the CPU the same convolution on bf16-rounded
    operands sits at >= 2.2e-3 / 6.3e-3 rms; vs ldm_op_conv3d_f32(form 1) <= 6.1e-7 (gate 6e-5)."""
    x, w, b = _thin_inputs(n, cin, cout, dims, bias, 200 + cin + cout)
    ref = F.conv3d(x.double(), w.double(), None if b is None else b.double(), padding=1)
    defect = F.conv3d(x.to(torch.bfloat16).double(), w.to(torch.bfloat16).double(), None if b is None else b.double(), padding=1)
    xd = x.permute(0, 2, 3, 4, 1).contiguous().to(cuda)
    bd = None
    if b is not None:
        bd = torch.zeros(COUT_PAD)
        bd[:cout] = b
        bd = bd.to(cuda)
    L = _lib().lib()
    need = L.ldm_op_conv3d_thin_f32_ws_bytes(cin, n, *dims, COUT_PAD)
    assert need % 4 == 0
    outs = []
    for fill in (0.0, 3.0, 0.0):
        wp = torch.full((27, COUT_PAD, cin), fill)
        wp[:, :cout] = w.reshape(cout, cin, 27).permute(2, 0, 1)
        wd = wp.to(cuda)
        ws = _nan(need // 4, cuda)
        out = _nan(ref.numel(), cuda)
        _call("ldm_op_conv3d_thin_f32", _p(xd), cin, _p(wd), _p(bd), _p(out), n, *dims, cout, COUT_PAD, _p(ws), need, _stream())
        outs.append(_take(out, ref.numel()).reshape(ref.shape))
        _take(ws, need // 4)
    what = f"thin conv fp32 N{n} Cin{cin} Cout{cout} {dims}"
    _gate(outs[0], ref, TOL_X3, what, defect, "bf16-rounded operands")
    assert torch.equal(outs[0], outs[1]), "weight rows >= CoutReal are read"
    assert torch.equal(outs[0], outs[2]), "second launch differs"
    # the general 3 x bf16 conv kernel on the same inputs
    wp = torch.zeros((27, COUT_PAD, cin))
    wp[:, :cout] = w.reshape(cout, cin, 27).permute(2, 0, 1)
    M = n * dims[0] * dims[1] * dims[2]
    scratch = torch.empty((64 * M * COUT_PAD,), device=cuda)
    o2 = _nan(ref.numel(), cuda)
    _call("ldm_op_conv3d_f32", _p(xd), cin, None, 0, _p(wp.to(cuda)), _p(bd), None, 0, None, None, 0, _p(o2), None, n, *dims, 3, 1, 1, 0,
          cout, COUT_PAD, 1, 0, 0, _p(scratch), scratch.numel() * 4, _stream())
    other = _take(o2, ref.numel()).reshape(ref.shape)
    e = _errs(outs[0], other)[0]
    print(f"{what}: vs ldm_op_conv3d_f32 form 1 rel-L2 {e:.2e} (gate {2 * TOL_X3:.0e})")
    assert e <= 2 * TOL_X3, e


_THIN_PLAN_CHILD = r'''
import json, sys, torch
sys.path.insert(0, "tests")
import cfgs
from ldm3d import _lib
from ldm3d.networks import AutoencoderKL
from oracle import autoencoder as oa
from oracle.unet import init_state_dict
cfg = dict(cfgs.VAE_TINY, channels=[64, 64, 64])
sd = init_state_dict(oa.ae_param_shapes(cfg), 21)
z = torch.randn((1, 8, 4, 4, 4), generator=torch.Generator().manual_seed(22))
dev = torch.device("cuda:0")
m = AutoencoderKL(**cfg); m.load_state_dict(sd); m = m.to(dev).eval()
m.set_precision("fp32")
L = _lib.lib()
_lib.check(L.ldm_set_plan_trace(sys.argv[1].encode()))
try:
    with torch.no_grad():
        rec = m.decode(z.to(dev))
    torch.cuda.synchronize()
finally:
    _lib.check(L.ldm_set_plan_trace(None))
kinds = [int(ln.split(",")[2]) for ln in open(sys.argv[1]).read().splitlines()]
with torch.no_grad():
    ref = oa.decode(sd, cfg, z)
print(json.dumps({"kinds": kinds, "rec": rec.flatten().double().cpu().tolist(), "ref": ref.flatten().double().tolist()}))
'''


def test_fp32_plan_takes_the_thin_conv_from_the_knob(cuda, tmp_path):
    """The fp32 branch of the planner reads LDM_CONV_THIN_MIN like the bf16 branch: an AutoencoderKL (VAE_TINY with 64 channels at full
    resolution, the narrowest last layer whose GroupNorm writes the (hi | lo) split) decoding 16^3 in the fp32 precision mode runs its last
    conv as OP_CONV_THIN with LDM_CONV_THIN_MIN=1 and on the 3 x bf16 halo kernel without it.  Everything in front of that conv is the same
    plan, so the two reconstructions are two 3 x bf16 evaluations of one layer on the same bits: each is within TOL_X3 of that layer in
    float64, hence rel-L2 <= 2 TOL_X3 of each other; the end-to-end distance to the fp32 CPU oracle keeps BASELINE's 1e-3 bar.
    Measured (MI355X): thin vs halo plan 6.0e-7; vs the oracle 1.5e-5 / 1.5e-5.  Child processes: the knob is read once per process.
    Not teacher-forced through decode_taps on VAE_TINY itself: its last layer has 32 input channels, whose GroupNorm never writes the split
    (x3_halo_ok: C % 64), and a tapped plan never does (vae_run_layout: the tap would export the split), so neither plan can hold the op
    (measured: 0 OP_CONV_THIN rows in both with the knob at 1)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    recs = {}
    for tag, env in (("default", {}), ("thin", {"LDM_CONV_THIN_MIN": "1"})):
        base = {k: v for k, v in os.environ.items() if k != "LDM_CONV_THIN_MIN"}
        r = subprocess.run([sys.executable, "-c", _THIN_PLAN_CHILD, str(tmp_path / f"{tag}.csv")], cwd=root, env=dict(base, **env),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        recs[tag] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert recs["default"]["kinds"].count(OP_CONV_THIN) == 0, recs["default"]["kinds"]
    assert recs["thin"]["kinds"].count(OP_CONV_THIN) == 1, recs["thin"]["kinds"]
    assert recs["thin"]["kinds"][-1] == OP_CONV_THIN
    a, b = (torch.tensor(recs[k]["rec"], dtype=torch.float64) for k in ("default", "thin"))
    ref = torch.tensor(recs["thin"]["ref"], dtype=torch.float64)
    e_ab, e_a, e_b = _errs(b, a)[0], _errs(a, ref)[0], _errs(b, ref)[0]
    print(f"fp32 decode 16^3, thin vs halo plan: rel-L2 {e_ab:.2e} (gate {2 * TOL_X3:.0e}); vs the fp32 CPU oracle {e_a:.2e} / {e_b:.2e} (gate 1e-3)")
    assert torch.isfinite(b).all()
    assert e_ab <= 2 * TOL_X3 and e_a <= 1e-3 and e_b <= 1e-3, (e_ab, e_a, e_b)


# ------------------------------------------------------------------------------------------------ time embedding
T_STEPS = [0.0, 1.0, 37.0, 500.0, 911.0, 999.0]


def _sinusoid_ref(dim, denom_off=0, sin_first=False):
    half = dim // 2
    j = torch.arange(half, dtype=torch.float64)
    arg = math.log(10000.0) * j / (half - denom_off)
    a = torch.tensor(T_STEPS, dtype=torch.float64)[:, None] * torch.exp(-arg)[None, :]
    parts = (torch.sin(a), torch.cos(a)) if sin_first else (torch.cos(a), torch.sin(a))
    return torch.cat(parts, 1), torch.cat((a, a), 1), torch.cat((arg, arg))[None, :]


@pytest.mark.parametrize("dim", [64, 96, 256])
def test_timestep_embedding_against_fp64(cuda, dim):
    """temb_sinusoid_kernel vs float64 cos | sin of t exp(-ln(1e4) j / half), cos first.  Per-element allowance from one rounding per
    fp32 operation and 1 ulp for expf / cosf / sinf (the figure HIP's math API documents for them), u = 2^-24, arg = ln(1e4) j / half:
    |err| <= |a| (3 arg u + 3 u) + 2 u.  Measured (MI355X): worst error / bound 0.26 (dim 64), 0.30 (96), 0.33 (256); on the CPU `half - 1`
    in the denominator lands >= 1.2e4 x over the bound in every row with t > 0, sin first >= 2.4e6 x in every row."""
    u = 2.0 ** -24
    ref, a, arg = _sinusoid_ref(dim)
    bound = a.abs() * (3 * arg * u + 3 * u) + 2 * u
    assert float(bound[1].max()) < 4e-7                       # the t = 1 row: the gate is sharp there
    t = torch.tensor(T_STEPS).to(cuda)
    outs = []
    for _ in range(2):
        out = _nan(len(T_STEPS) * dim, cuda)
        _call("ldm_op_timestep_embedding", _p(t), _p(out), len(T_STEPS), dim, _stream())
        outs.append(_take(out, len(T_STEPS) * dim).reshape(len(T_STEPS), dim))
    got = outs[0]
    assert torch.isfinite(got).all() and torch.equal(outs[0], outs[1])
    ratio = (got.double() - ref).abs() / bound
    d1 = ((_sinusoid_ref(dim, denom_off=1)[0] - ref).abs() / bound)[1:].amax(dim=1)
    d2 = ((_sinusoid_ref(dim, sin_first=True)[0] - ref).abs() / bound).amax(dim=1)
    print(f"sinusoid dim {dim}: worst error / bound {float(ratio.max()):.2f} (per row {[round(float(v), 2) for v in ratio.amax(dim=1)]}); "
          f"half - 1 denominator {float(d1.min()):.1e} x the bound in its best row, sin first {float(d2.min()):.1e} x")
    assert float(ratio.max()) <= 1.0, (dim, float(ratio.max()), int(ratio.argmax()))
    assert float(d1.min()) > 1e4 and float(d2.min()) > 10.0


# B, I, O, x_stride, y_stride, silu, bias
GEMV_CASES = [(2, 64, 256, 64, 256, 0, True),          # eight active lanes
              (3, 1024, 1024, 1024, 1024, 1, True),    # two trips of the 512-wide loop
              (2, 384, 70, 400, 72, 1, True),          # idle lanes, last workgroup with two idle waves, padded rows
              (1000, 256, 36, 256, 36, 1, True),       # the table build's batch, grid.y = 1000
              (2, 64, 256, 64, 256, 0, False)]         # bias == nullptr


@pytest.mark.parametrize("fp32_w", [0, 1])
@pytest.mark.parametrize("B,I,O,xs,ys,silu,bias", GEMV_CASES)
def test_gemv_against_fp64(cuda, fp32_w, B, I, O, xs, ys, silu, bias):
    """gemv_bf16_kernel / gemv_f32_kernel vs float64 on the same weights and fp32 x (SiLU in float64).
    Measured (MI355X): rel-L2 <= 9.0e-8 (bf16 weights) / 9.7e-8 (fp32), <= 7.7e-7 rms per element (gates 1e-5 / 1e-4); on the CPU, without
    SiLU on the input (or, in the cases that have none, with one) the result is >= 0.49 rel-L2 and >= 1.7 rms away."""
    g = torch.Generator().manual_seed(300 + I + O)
    w = torch.randn((O, I), generator=g) / I ** 0.5
    if not fp32_w:
        w = w.to(torch.bfloat16)
    b = 0.1 * torch.randn((O,), generator=g) if bias else None
    x = torch.randn((B, xs), generator=g)
    if silu:
        x[:, :5] = torch.tensor([100.0, -100.0, 20.0, -20.0, 0.0])
    xr = x[:, :I].double()
    act, other = (F.silu(xr), xr) if silu else (xr, F.silu(xr))
    ref = act @ w.double().T + (0 if b is None else b.double())
    defect = other @ w.double().T + (0 if b is None else b.double())
    wd, xd, bd = w.to(cuda), x.to(cuda), None if b is None else b.to(cuda)
    outs = []
    for _ in range(2):
        y = _nan(B * ys, cuda)
        _call("ldm_op_gemv", _p(wd), fp32_w, _p(bd), _p(xd), _p(y), B, I, O, xs, ys, silu, _stream())
        outs.append(_take(y, B * ys).reshape(B, ys))
    assert torch.isnan(outs[0][:, O:]).all(), "y[O .. y_stride) was written"
    _gate(outs[0][:, :O], ref, TOL, f"gemv {'fp32' if fp32_w else 'bf16'} B{B} I{I} O{O} silu {silu}", defect,
          "SiLU dropped" if silu else "SiLU applied")
    assert torch.equal(outs[0][:, :O], outs[1][:, :O]), "second launch differs"


# ------------------------------------------------------------------------------------------------ packing
SPECIALS = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.0, -0.0, -(1 + 3 * 2.0 ** -8)]   # exact RNE ties of bf16, +-0


def _special_randn(shape, g):
    x = torch.randn(shape, generator=g)
    k = min(len(SPECIALS), x.numel())
    x.view(-1)[:k] = torch.tensor(SPECIALS[:k])
    return x


def _pack2_ref(x, cond, cs, fp32_out, guided, fill):
    """[N][DHW][Cs]: (x | cond) channel-concatenated, zero channel padding; guided: (x | fill) samples, then (x | cond) samples."""
    if guided:
        full = torch.cat([torch.cat([x, torch.full_like(cond, fill)], 1), torch.cat([x, cond], 1)], 0)
    else:
        full = x if cond is None else torch.cat([x, cond], 1)
    out = torch.zeros((full.shape[0], full.shape[2], cs))
    out[..., :full.shape[1]] = full.permute(0, 2, 1)
    return out if fp32_out else out.to(torch.bfloat16)


@pytest.mark.parametrize("fp32_out", [0, 1])
@pytest.mark.parametrize("n,cx,cc,cs,dhw,guided,fill", [(2, 4, 4, 32, 105, 0, 0.0), (1, 3, 0, 32, 1, 0, 0.0), (3, 1, 8, 32, 64, 0, 0.0),
                                                       (2, 4, 4, 32, 105, 1, -1.0), (2, 4, 4, 32, 105, 1, 0.3)])
def test_pack2_is_bit_identical_to_torch(cuda, fp32_out, n, cx, cc, cs, dhw, guided, fill):
    """pack2_ncdhw_kernel / pack2_ncdhw_f32_kernel with a condition tensor and guided_pack2_ncdhw_kernel<bf16_t | float> vs a torch
    construction (bf16 RNE through .to(torch.bfloat16)), compared as integers: ties, +-0, mixed signs, zero padding channels, fill
    rounded by the store (bf16(0.3) / 0.3f).  n = the caller's batch; the guided output holds 2 n samples."""
    g = torch.Generator().manual_seed(400 + cx + cc)
    x = _special_randn((n, cx, dhw), g)
    cond = _special_randn((n, cc, dhw), g) if cc else None
    want = _pack2_ref(x, cond, cs, fp32_out, guided, fill)
    n_out = 2 * n if guided else n
    dt = torch.float32 if fp32_out else torch.bfloat16
    xd, cd = x.to(cuda), None if cond is None else cond.to(cuda)
    outs = []
    for _ in range(2):
        out = _nan(want.numel(), cuda, dt)
        _call("ldm_op_pack2", _p(xd), cx, _p(cd), cc, _p(out), n_out, cs, dhw, fp32_out, n if guided else 0, fill, _stream())
        outs.append(_take(out, want.numel()))
    _same_bits(outs[0], want, f"pack2 {'fp32' if fp32_out else 'bf16'} N{n} cx{cx} cc{cc} DHW{dhw} guided {guided} fill {fill}")
    _same_bits(outs[1], want, "second launch")
    if guided:
        col = outs[0].reshape(n_out, dhw, cs)[:n, :, cx:cx + cc]
        assert (_bits(col) == _bits(torch.tensor([fill]).to(dt))).all()
        assert (_bits(outs[0].reshape(n_out, dhw, cs)[..., cx + cc:]) == 0).all()


def _im2col_k(cin):
    """Model::im2col_k: the builder's K of the first conv's patch matrix."""
    k = 27 * cin
    return rup(k, 32) if k <= 96 else rup(k, 128)


def _im2col_ref(full, kp):
    """[N D H W][Kp] bf16: column tap * cin + c, zero outside the volume and behind 27 cin."""
    n, cin, d, h, w = full.shape
    xp = F.pad(full, (1, 1, 1, 1, 1, 1))
    cols = [xp[:, :, kd:kd + d, kh:kh + h, kw:kw + w].permute(0, 2, 3, 4, 1) for kd in range(3) for kh in range(3) for kw in range(3)]
    out = torch.zeros((n * d * h * w, kp))
    out[:, :27 * cin] = torch.stack(cols, 4).reshape(n * d * h * w, 27 * cin)
    return out.to(torch.bfloat16)


@pytest.mark.parametrize("cx,cc,dims,guided", [(4, 0, (3, 4, 5), 0), (4, 4, (3, 4, 5), 0), (1, 0, (3, 4, 5), 0), (3, 2, (3, 4, 5), 0),
                                               (4, 4, (1, 1, 1), 0), (4, 4, (3, 4, 5), 1)])
def test_pack_im2col_is_bit_identical_to_torch(cuda, cx, cc, dims, guided):
    """pack_im2col_kernel / guided_pack_im2col_kernel (N 2) vs the torch construction of the 3^3 pad-1 patch matrix, Kp from the builder's
    rule: every tap of every voxel, out-of-volume taps and the pad columns k >= 27 cin exactly +0 (1 x 1 x 1: every tap but the centre)."""
    n, fill = 2, -1.0
    g = torch.Generator().manual_seed(500 + cx + cc)
    x = _special_randn((n, cx, *dims), g)
    cond = _special_randn((n, cc, *dims), g) if cc else None
    kp = _im2col_k(cx + cc)
    if guided:
        full = torch.cat([torch.cat([x, torch.full_like(cond, fill)], 1), torch.cat([x, cond], 1)], 0)
    else:
        full = x if cond is None else torch.cat([x, cond], 1)
    want = _im2col_ref(full, kp)
    xd, cd = x.to(cuda), None if cond is None else cond.to(cuda)
    outs = []
    for _ in range(2):
        out = _nan(want.numel(), cuda, torch.bfloat16)
        _call("ldm_op_pack_im2col", _p(xd), cx, _p(cd), cc, _p(out), full.shape[0], *dims, kp, n if guided else 0, fill, _stream())
        outs.append(_take(out, want.numel()))
    _same_bits(outs[0], want, f"im2col cx{cx} cc{cc} {dims} Kp{kp} guided {guided}")
    _same_bits(outs[1], want, "second launch")
    assert (_bits(outs[0].reshape(-1, kp)[:, 27 * (cx + cc):]) == 0).all()
    if dims == (1, 1, 1):
        centre = 13 * (cx + cc)
        rest = torch.cat([outs[0].reshape(-1, kp)[:, :centre], outs[0].reshape(-1, kp)[:, centre + cx + cc:]], 1)
        assert (_bits(rest) == 0).all()


# ------------------------------------------------------------------------------------------------ derived weights and splits
def _split(x):
    """hi = bf16(x), lo = bf16(x - hi) in fp32 (f32_path.h split_bf16x4)."""
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def _phase_taps(defect=False):
    """Taps (kd * 3 + kh) * 3 + kw summed into [parity * 8 + tap2], kernel order (norm_elem.h phase_weights_kernel): per dimension
    parity 0 reads k0 | k1 + k2, parity 1 reads k0 + k1 | k2.  defect: parity 1, tap 0 takes k0 alone."""
    def rng(p, t):
        if p == 0:
            return [1, 2] if t else [0]
        return [2] if t else ([0] if defect else [0, 1])
    out = []
    for ph in range(8):
        for tp in range(8):
            r = [rng((ph >> s) & 1, (tp >> s) & 1) for s in (2, 1, 0)]
            out.append([(kd * 3 + kh) * 3 + kw for kd in r[0] for kh in r[1] for kw in r[2]])
    return out


def _phase_sums(w3, dtype, defect=False):
    """[64][cout_pad][cin] sums of w3 [27][cout_pad][cin] in the kernel's kd, kh, kw order, accumulated in `dtype`."""
    out = []
    for taps in _phase_taps(defect):
        acc = torch.zeros(w3.shape[1:], dtype=dtype)
        for t in taps:
            acc = acc + w3[t].to(dtype)
        out.append(acc)
    return torch.stack(out)


def _ordered(t):
    """bf16 -> integers in which neighbouring values differ by one."""
    i = _bits(t).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7fff), i)


def _run_phase(cuda, w3):
    _, cout_pad, cin_s = w3.shape
    n = 64 * cout_pad * cin_s
    wd = w3.to(cuda)
    outs = []
    for _ in range(2):
        out = _nan(n, cuda, torch.bfloat16)
        _call("ldm_op_phase_weights", _p(wd), _p(out), cout_pad, cin_s, _stream())
        outs.append(_take(out, n).reshape(64, cout_pad, cin_s))
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "second launch differs"
    assert torch.isfinite(outs[0].float()).all()
    return outs[0]


@pytest.mark.parametrize("cin_s", [32, 64])
def test_phase_weights_exact_sums_round_to_nearest_even(cuda, cin_s):
    """phase_weights_kernel on weights k / 256, integer k in [-128, 128): every sum of up to 8 taps is exact in fp32, so the result is
    bf16(sum) bit for bit; 3.0 % of the sums need the rounding.  The defect (parity 1, tap 0 = k0 alone) changes 58 % of the elements.
    Measured (MI355X): 0 of 131072 / 262144 elements differ."""
    g = torch.Generator().manual_seed(600 + cin_s)
    w3 = (torch.randint(-128, 128, (27, COUT_PAD, cin_s), generator=g).float() / 256).to(torch.bfloat16)
    s = _phase_sums(w3, torch.float32)
    assert torch.equal(s.double(), _phase_sums(w3, torch.float64))          # exact
    want = s.to(torch.bfloat16)
    rounded = float((want.float() != s).float().mean())
    bad = float((_bits(_phase_sums(w3, torch.float32, defect=True).to(torch.bfloat16)) != _bits(want)).float().mean())
    print(f"phase weights cin_s {cin_s}: {rounded:.3f} of the sums are rounded; the defect changes {bad:.2f} of the elements")
    assert rounded > 0.01 and bad > 0.1
    _same_bits(_run_phase(cuda, w3), want, f"phase weights, exact sums, cin_s {cin_s}")


@pytest.mark.parametrize("cin_s", [32, 64])
def test_phase_weights_random_against_fp64(cuda, cin_s):
    """phase_weights_kernel on random bf16 weights N(0, 1 / (27 cin)) vs bf16(float64 sum): no element more than one bf16 ulp away, at
    most 1e-3 of the elements different at all (a condition: on the CPU the fp32-sum construction differs in 0 of 262144).
    Measured (MI355X): 0 of 131072 / 0 of 262144 differ; the defect differs in 0.58 of the elements by up to 3e4 ulps."""
    g = torch.Generator().manual_seed(610 + cin_s)
    w3 = (torch.randn((27, COUT_PAD, cin_s), generator=g) / (27 * cin_s) ** 0.5).to(torch.bfloat16)
    want = _phase_sums(w3, torch.float64).to(torch.bfloat16)
    got = _run_phase(cuda, w3)
    d = (_ordered(got) - _ordered(want)).abs()
    dd = (_ordered(_phase_sums(w3, torch.float32, defect=True).to(torch.bfloat16)) - _ordered(want)).abs()
    frac, dfrac = float((d > 0).float().mean()), float((dd > 0).float().mean())
    print(f"phase weights random cin_s {cin_s}: {int((d > 0).sum())} of {d.numel()} differ, worst {int(d.max())} ulp; "
          f"defect: {dfrac:.2f} differ, worst {int(dd.max())} ulp")
    assert int(d.max()) <= 1 and frac <= 1e-3, (int(d.max()), frac)
    assert dfrac > 10 * 1e-3 and int(dd.max()) > 10


@pytest.mark.parametrize("cin,cin_s", [(1, 32), (4, 32), (8, 32), (5, 64)])
def test_im2col_weights_are_bit_identical_to_torch(cuda, cin, cin_s):
    """im2col_weights_kernel: w2[co][tap cin + c] = w3[tap][co][c], columns >= 27 cin +0, Kp from the builder's rule."""
    g = torch.Generator().manual_seed(620 + cin)
    w3 = torch.randn((27, COUT_PAD, cin_s), generator=g).to(torch.bfloat16)
    kp = _im2col_k(cin)
    want = torch.zeros((COUT_PAD, kp), dtype=torch.bfloat16)
    want[:, :27 * cin] = w3[:, :, :cin].permute(1, 0, 2).reshape(COUT_PAD, 27 * cin)
    wd = w3.to(cuda)
    outs = []
    for _ in range(2):
        out = _nan(want.numel(), cuda, torch.bfloat16)
        _call("ldm_op_im2col_weights", _p(wd), _p(out), COUT_PAD, cin_s, cin, kp, _stream())
        outs.append(_take(out, want.numel()))
    _same_bits(outs[0], want, f"im2col weights cin {cin} Kp {kp}")
    _same_bits(outs[1], want, "second launch")


def _special_f32(shape, g, scale=1.0):
    return _special_randn(shape, g) * scale


@pytest.mark.parametrize("cin", [32, 64])
def test_x3_weights_are_bit_identical_to_torch(cuda, cin):
    """x3_weights_kernel: fp32 [rows][cin] -> bf16 [rows][hi | lo | hi] (f32_path.h: the halo / thin kernels' weight layout)."""
    rows = 27 * COUT_PAD
    w = _special_f32((rows, cin), torch.Generator().manual_seed(630 + cin), 0.05)
    hi, lo = _split(w)
    want = torch.cat([hi, lo, hi], 1)
    assert float((hi.double() + lo.double() - w.double()).abs().max()) <= 2.0 ** -16 * float(w.abs().max())
    wd = w.to(cuda)
    outs = []
    for _ in range(2):
        out = _nan(want.numel(), cuda, torch.bfloat16)
        _call("ldm_op_x3_weights", _p(wd), _p(out), rows, cin, _stream())
        outs.append(_take(out, want.numel()))
    _same_bits(outs[0], want, f"x3 weights cin {cin}")
    _same_bits(outs[1], want, "second launch")


@pytest.mark.parametrize("up", [0, 1])
def test_split_f32_is_bit_identical_to_torch(cuda, up):
    """upsample_split_f32_kernel: fp32 NDHWC -> [hi(C) | lo(C)] bf16 rows, nearest x2 upsampled when up (N 2, C 32, 2 x 3 x 5)."""
    n, c, dims = 2, 32, (2, 3, 5)
    x = _special_f32((n, *dims, c), torch.Generator().manual_seed(640 + up))
    src = x
    if up:
        for ax in (1, 2, 3):
            src = src.repeat_interleave(2, dim=ax)
    hi, lo = _split(src)
    want = torch.cat([hi, lo], -1)
    xd = x.to(cuda)
    outs = []
    for _ in range(2):
        out = _nan(want.numel(), cuda, torch.bfloat16)
        _call("ldm_op_split_f32", _p(xd), _p(out), n, c, *dims, up, _stream())
        outs.append(_take(out, want.numel()))
    _same_bits(outs[0], want, f"split up {up}")
    _same_bits(outs[1], want, "second launch")


@pytest.mark.parametrize("cin", [32, 64])
def test_x3_phase_weights_layout_and_sums(cuda, cin):
    """x3_phase_weights_kernel: [parity 8][tap 8][cout_pad][hi | hi | lo] (f32_path.h; NOT the [hi | lo | hi] of x3_weights_kernel) of the
    phase sums.  Bit-identical to the split of fp32 sums accumulated in the kernel's kd, kh, kw order, and
    |hi + lo - s64| <= 2^-16 |s64| + 7 u sum |w| against the float64 sums.  Measured (MI355X): 0 elements differ, worst error / bound 0.49;
    the defect puts 58 % of the float64 sums more than 10x outside the bound."""
    g = torch.Generator().manual_seed(650 + cin)
    w3 = torch.randn((27, COUT_PAD, cin), generator=g) / (27 * cin) ** 0.5
    hi, lo = _split(_phase_sums(w3, torch.float32))
    want = torch.cat([hi, hi, lo], -1)
    wd = w3.to(cuda)
    outs = []
    for _ in range(2):
        out = _nan(want.numel(), cuda, torch.bfloat16)
        _call("ldm_op_x3_phase_weights", _p(wd), _p(out), COUT_PAD, cin, _stream())
        outs.append(_take(out, want.numel()))
    _same_bits(outs[0], want, f"x3 phase weights cin {cin}")
    _same_bits(outs[1], want, "second launch")
    got = outs[0].reshape(64, COUT_PAD, 3 * cin).double()
    assert torch.equal(got[..., :cin], got[..., cin:2 * cin])
    s64, sabs = _phase_sums(w3, torch.float64), _phase_sums(w3.abs(), torch.float64)
    ratio = (got[..., :cin] + got[..., 2 * cin:] - s64).abs() / (2.0 ** -16 * s64.abs() + 7 * 2.0 ** -24 * sabs)
    d64 = _phase_sums(w3, torch.float64, defect=True)
    dratio = (d64 - s64).abs() / (2.0 ** -16 * s64.abs() + 7 * 2.0 ** -24 * sabs)
    print(f"x3 phase weights cin {cin}: worst error / bound {float(ratio.max()):.2f}; defect: {float((dratio > 10).float().mean()):.2f} of the "
          f"elements > 10 x the bound")
    assert float(ratio.max()) <= 1.0
    assert float((dratio > 10).float().mean()) > 0.3


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_before_the_device(cuda):
    """Argument checks return LDM_ERR_BAD_ARG (-1) / LDM_ERR_UNSUPPORTED (-2) / LDM_ERR_WORKSPACE (-5) without launching anything: the
    NaN-filled output every call points at stays NaN."""
    L = _lib().lib()
    x = torch.zeros(1 << 21, device=cuda)
    o = torch.full((1 << 21,), float("nan"), device=cuda)
    s = _stream()
    X, O = _p(x), _p(o)
    thin = L.ldm_op_conv3d_thin
    assert thin(X, 48, X, X, O, 1, 2, 2, 2, 1, 64, s) == ERR_BAD_ARG                   # cin % 32
    assert thin(X, 32, X, X, O, 1, 2, 2, 2, 0, 64, s) == ERR_BAD_ARG                   # cout_real 0
    assert thin(X, 32, X, X, O, 1, 2, 2, 2, 5, 64, s) == ERR_BAD_ARG                   # cout_real 5
    assert thin(X, 32, X, X, O, 1, 2, 2, 2, 3, 2, s) == ERR_BAD_ARG                    # cout_pad < cout_real
    assert thin(X, 32, X, X, None, 1, 2, 2, 2, 1, 64, s) == ERR_BAD_ARG                # no output
    assert thin(X, 32, X, X, O, 1, 0, 2, 2, 1, 64, s) == ERR_BAD_ARG                   # empty volume
    assert thin(X, 160, X, X, O, 1, 2, 2, 2, 1, 64, s) == ERR_UNSUPPORTED              # cin > 128
    thin32 = L.ldm_op_conv3d_thin_f32
    need = L.ldm_op_conv3d_thin_f32_ws_bytes(32, 1, 2, 2, 2, 64)
    assert need == rup(8 * 64 * 2, 256) + 27 * 64 * 96 * 2
    assert thin32(X, 40, X, X, O, 1, 2, 2, 2, 1, 64, O, 1 << 22, s) == ERR_BAD_ARG     # cin % 32
    assert thin32(X, 256, X, X, O, 1, 2, 2, 2, 1, 64, O, 1 << 22, s) == ERR_UNSUPPORTED
    assert thin32(X, 32, X, X, O, 1, 2, 2, 2, 1, 64, O, need - 1, s) == ERR_WORKSPACE
    assert thin32(X, 32, X, X, O, 1, 2, 2, 2, 1, 64, None, need, s) == ERR_WORKSPACE
    temb = L.ldm_op_timestep_embedding
    assert temb(X, O, 0, 64, s) == ERR_BAD_ARG
    assert temb(X, O, 2, 1, s) == ERR_BAD_ARG
    assert temb(None, O, 2, 64, s) == ERR_BAD_ARG
    assert temb(X, O, 4097, 256, s) == ERR_UNSUPPORTED                                 # more elements than the grid has threads
    gemv = L.ldm_op_gemv
    assert gemv(X, 0, X, X, O, 2, 68, 4, 68, 4, 0, s) == ERR_BAD_ARG                   # bf16 weights: I % 8
    assert gemv(X, 1, X, X, O, 2, 66, 4, 68, 4, 0, s) == ERR_BAD_ARG                   # fp32 weights: I % 4
    assert gemv(X, 1, X, X, O, 2, 64, 4, 66, 4, 0, s) == ERR_BAD_ARG                   # fp32 weights: x_stride % 4
    assert gemv(X, 1, X, X + 4, O, 2, 64, 4, 64, 4, 0, s) == ERR_BAD_ARG               # fp32 weights: x not 16-byte aligned
    assert gemv(X, 0, X, X, O, 2, 64, 4, 56, 4, 0, s) == ERR_BAD_ARG                   # x_stride < I
    assert gemv(X, 0, X, X, O, 2, 64, 8, 64, 4, 0, s) == ERR_BAD_ARG                   # y_stride < O
    assert gemv(X, 0, X, X, O, 70000, 8, 1, 8, 1, 0, s) == ERR_BAD_ARG                 # B past grid.y
    pack2 = L.ldm_op_pack2
    assert pack2(X, 4, X, 4, O, 2, 4, 8, 0, 0, 0.0, s) == ERR_BAD_ARG                  # cx + cc > Cs
    assert pack2(X, 4, X, 4, O, 2, 32, 0, 0, 0, 0.0, s) == ERR_BAD_ARG                 # DHW 0
    assert pack2(X, 4, X, 4, O, 3, 32, 8, 1, 1, 0.0, s) == ERR_BAD_ARG                 # guided: N != 2 B
    assert pack2(X, 4, None, 4, O, 2, 32, 8, 0, 1, 0.0, s) == ERR_BAD_ARG              # guided without a condition
    im2col = L.ldm_op_pack_im2col
    assert im2col(X, 4, None, 0, O, 1, 2, 2, 2, 108, 0, 0.0, s) == ERR_BAD_ARG         # Kp % 8
    assert im2col(X, 4, None, 0, O, 1, 2, 2, 2, 104, 0, 0.0, s) == ERR_BAD_ARG         # Kp < 27 cin
    assert im2col(X, 4, X, 4, O, 1, 2, 2, 2, 128, 0, 0.0, s) == ERR_BAD_ARG            # Kp < 27 (cx + cc)
    assert im2col(X, 4, None, 0, O, 2, 2, 2, 2, 128, 1, 0.0, s) == ERR_BAD_ARG         # guided without a condition
    assert L.ldm_op_phase_weights(X, O, 64, 12, s) == ERR_BAD_ARG                      # cin_s % 8
    assert L.ldm_op_phase_weights(X, None, 64, 32, s) == ERR_BAD_ARG
    assert L.ldm_op_im2col_weights(X, O, 64, 32, 4, 104, s) == ERR_BAD_ARG             # Kp < 27 cin
    assert L.ldm_op_im2col_weights(X, O, 64, 32, 33, 1024, s) == ERR_BAD_ARG           # cin > cin_s
    assert L.ldm_op_x3_weights(X, O, 4, 6, s) == ERR_BAD_ARG                           # cin % 4
    assert L.ldm_op_x3_weights(X, O, 0, 32, s) == ERR_BAD_ARG
    assert L.ldm_op_x3_phase_weights(X, O, 64, 6, s) == ERR_BAD_ARG
    assert L.ldm_op_split_f32(X, O, 1, 6, 2, 2, 2, 0, s) == ERR_BAD_ARG                # C % 4
    assert L.ldm_op_split_f32(X, O, 1, 32, 2, 2, 2, 2, s) == ERR_BAD_ARG               # up 2
    torch.cuda.synchronize()
    assert torch.isnan(o).all()
