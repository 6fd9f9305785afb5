"""conv3_dgrad_thin_kernel (csrc/conv_dgrad_thin.h) through ldm_op_conv3d_dgrad_thin (-m gpu): the data gradient of the UNet's first
conv w.r.t. its 1 .. 32 real input channels, written as fp32 NCDHW into two destinations (dx | dcond).

Checker: fp64 ``conv_transpose3d`` on the operands as the kernel sees them.

* bf16 mode: dy and w rounded to bf16 -> products exact, fp32 accumulation: rel-L2 <= 1e-5, worst row <= 1e-4 (the fp32-output gate of
  test_gpu_bf16_train_ops.py).
* fp32 mode (3 x bf16 on the hi | lo split): TOL_X3 = 3e-5, ten times that per row (test_gpu_f32_ops.py), with that file's control that
  the same gradient from bf16-rounded operands sits more than 10x the gate away.

Cases: (cx, cc) across the 16-row tile boundary and both tiles full, 64 and 96 dy channels, N = 2, volumes of exactly one block, ragged on
every axis, narrower than a block in W, and one voxel; dx only, dcond only and both (a NULL destination's guard band stays untouched).
Defect control: the reference with unmirrored taps lies more than 10x the gate away wherever D, H, W > 1.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL_BF16 = 1e-5
TOL_X3 = 3e-5
GUARD = 64

SPLITS = [(3, 0), (1, 2), (4, 4), (8, 8), (16, 0), (16, 16), (17, 0)]
DIMS = [(4, 4, 16), (5, 6, 17), (8, 12, 4), (1, 1, 1)]
N = 2


def _lib():
    from ldm3d import _lib
    return _lib


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


MIN_ROW = 16


def _worst_row(got, ref, scale=None):
    """Rows = the kernel's own output rows: one input channel over the batch and the volume (what this gate adds to rel-L2 is a wrong
    channel that is small in the tensor's norm), error relative to the row's own norm.  ``scale`` (fp32 mode only): a row of fewer than
    MIN_ROW elements is measured against the norm of its term scale sum |dy| |w| instead: one or two dot products can cancel to a
    small fraction of their terms, and the 3 x bf16 product's error is relative to the terms, not to their sum (measured at the
    one-voxel volume: 4.7e-4 of its own value on a single element of a tensor that is 4.8e-6 away as a whole).  In bf16 mode the
    products are exact and every row is gated against its own norm."""
    c = got.shape[1]
    g2, r2 = got.double().cpu().transpose(0, 1).reshape(c, -1), ref.transpose(0, 1).reshape(c, -1)
    rn = r2.norm(dim=1)
    if scale is not None and g2.shape[1] < MIN_ROW:
        rn = scale.transpose(0, 1).reshape(c, -1).norm(dim=1)
    keep = rn > 1e-6 * rn.max()
    return float(((g2 - r2).norm(dim=1)[keep] / rn[keep]).max())


def _operands(cdy, cin, dims, seed):
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn((N, cdy, *dims), generator=g)
    w = torch.randn((cdy, cin, 3, 3, 3), generator=g) / (27 * cdy) ** 0.5
    return dy, w


def _ref(dy, w):
    """d/dx of conv3d(x, w, padding=1) given dy, fp64."""
    return F.conv_transpose3d(dy.double(), w.double(), padding=1)


def _ref_unmirrored(dy, w):
    """The defect: taps not mirrored (a correlation with the transposed weights)."""
    return F.conv3d(dy.double(), w.double().transpose(0, 1).contiguous(), padding=1)


def _launch(cuda, dy, w, cx, cc, fp32_mode, want_dx=True, want_dcond=True):
    """dy [N][C][D][H][W] fp32 on the CPU; returns (dx, dcond) on the CPU, each None when not asked for, guard bands checked."""
    n, cdy = dy.shape[:2]
    dims = tuple(dy.shape[2:])
    dhw = dims[0] * dims[1] * dims[2]
    dyl = dy.permute(0, 2, 3, 4, 1).contiguous()
    dyd = (dyl if fp32_mode else dyl.to(torch.bfloat16)).to(cuda)
    wd = w.contiguous().to(cuda)
    bufs = {}
    for name, c, want in (("dx", cx, want_dx), ("dcond", cc, want_dcond)):
        bufs[name] = torch.full((GUARD + n * c * dhw + GUARD,), float("nan"), dtype=torch.float32, device=cuda)
    ptr = lambda name, want, c: (bufs[name].data_ptr() + 4 * GUARD) if (want and c) else None
    L = _lib()
    L.check(L.lib().ldm_op_conv3d_dgrad_thin(dyd.data_ptr(), cdy, wd.data_ptr(), cdy, cx + cc, cx, cc, ptr("dx", want_dx, cx),
                                             ptr("dcond", want_dcond, cc), n, *dims, 1 if fp32_mode else 0,
                                             torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = []
    for name, c, want in (("dx", cx, want_dx), ("dcond", cc, want_dcond)):
        b = bufs[name].cpu()
        assert torch.isnan(b[:GUARD]).all() and torch.isnan(b[-GUARD:]).all(), f"{name}: guard band written"
        body = b[GUARD:GUARD + n * c * dhw]
        if want and c:
            assert torch.isfinite(body).all(), f"{name}: element not written"
            out.append(body.view(n, c, *dims))
        else:
            assert torch.isnan(body).all(), f"{name}: a destination that was not asked for was written"
            out.append(None)
    return out


def _check(what, got_dx, got_dc, ref, cx, cc, tol, control=None, unmirrored=None, scale=None):
    parts = [t for t in (got_dx, got_dc) if t is not None]
    got = torch.cat(parts, dim=1).double()
    e, worst = _rel(got, ref), _worst_row(got, ref, scale)
    msg = f"{what}: rel-L2 {e:.2e} (gate {tol:.0e}), worst row {worst:.2e} (gate {10 * tol:.0e})"
    if control is not None:
        msg += f", bf16 operands {control:.1e}"
    if unmirrored is not None:
        msg += f", unmirrored taps {unmirrored:.1e}"
    print(msg)
    assert e <= tol, (what, e)
    assert worst <= 10 * tol, (what, worst)
    if control is not None:
        assert control > 10 * tol, (what, "the gate cannot tell fp32 from bf16 operands", control)
    if unmirrored is not None:
        assert unmirrored > 10 * tol, (what, "the gate cannot tell mirrored from unmirrored taps", unmirrored)


@pytest.mark.parametrize("fp32_mode", [0, 1], ids=["bf16", "fp32"])
@pytest.mark.parametrize("cdy", [64, 96])
@pytest.mark.parametrize("split", SPLITS, ids=lambda s: f"cx{s[0]}cc{s[1]}")
def test_thin_dgrad_matches_fp64_conv_transpose(cuda, split, cdy, fp32_mode):
    """Every (cx, cc), dy width and precision mode over the four volumes, both destinations."""
    cx, cc = split
    for k, dims in enumerate(DIMS):
        dy, w = _operands(cdy, cx + cc, dims, 100 * cdy + 10 * cx + cc + k)
        if fp32_mode:
            ref = _ref(dy, w)
            control = _rel(_ref(dy.to(torch.bfloat16), w.to(torch.bfloat16)), ref)
            tol = TOL_X3
        else:
            dy, w = dy.to(torch.bfloat16).float(), w.to(torch.bfloat16).float()
            ref, control, tol = _ref(dy, w), None, TOL_BF16
        unm = _rel(_ref_unmirrored(dy, w), ref) if min(dims) > 1 else None
        dx, dc = _launch(cuda, dy, w, cx, cc, fp32_mode)
        scale = _ref(dy.abs(), w.abs()) if fp32_mode else None
        _check(f"dgrad_thin {'fp32' if fp32_mode else 'bf16'} C{cdy} cx{cx} cc{cc} {dims}", dx, dc, ref, cx, cc, tol, control, unm, scale)


@pytest.mark.parametrize("fp32_mode", [0, 1], ids=["bf16", "fp32"])
@pytest.mark.parametrize("which", ["dx", "dcond"])
def test_null_destination_is_not_stored(cuda, which, fp32_mode):
    """dx only and dcond only: the other part's buffer (body and guard bands) stays NaN, the stored part equals the both-destinations run."""
    for (cx, cc), dims in (((4, 4), (5, 6, 17)), ((16, 16), (4, 4, 16)), ((1, 2), (8, 12, 4))):
        dy, w = _operands(64, cx + cc, dims, 7 + cx)
        if not fp32_mode:
            dy, w = dy.to(torch.bfloat16).float(), w.to(torch.bfloat16).float()
        both = _launch(cuda, dy, w, cx, cc, fp32_mode)
        one = _launch(cuda, dy, w, cx, cc, fp32_mode, want_dx=which == "dx", want_dcond=which == "dcond")
        k = 0 if which == "dx" else 1
        assert one[1 - k] is None
        assert torch.equal(one[k], both[k])
        ref = _ref(dy, w)[:, :cx] if which == "dx" else _ref(dy, w)[:, cx:]
        e = _rel(one[k], ref)
        print(f"dgrad_thin {which} only, cx{cx} cc{cc} {dims}: rel-L2 {e:.2e}")
        assert e <= (TOL_X3 if fp32_mode else TOL_BF16)


def test_bad_arguments_are_refused(cuda):
    L = _lib()
    t = torch.zeros(4096, device=cuda)
    s = torch.cuda.current_stream().cuda_stream
    f = L.lib().ldm_op_conv3d_dgrad_thin
    assert f(t.data_ptr(), 64, t.data_ptr(), 64, 8, 4, 4, None, None, 1, 1, 1, 1, 0, s) != 0        # no destination
    assert f(t.data_ptr(), 48, t.data_ptr(), 48, 8, 4, 4, t.data_ptr(), None, 1, 1, 1, 1, 0, s) != 0   # dy channels not a multiple of 32
    assert f(t.data_ptr(), 64, t.data_ptr(), 64, 33, 33, 0, t.data_ptr(), None, 1, 1, 1, 1, 0, s) != 0   # more than 32 real channels
    assert f(t.data_ptr(), 64, t.data_ptr(), 64, 8, 4, 3, t.data_ptr(), None, 1, 1, 1, 1, 0, s) != 0   # cx + cc != cin_real
