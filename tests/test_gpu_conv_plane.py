"""conv3_plane_kernel (conv_plane.h): the 3^3 stride-1 convs of volumes past 6^3 up to 12^3, unsplit: one workgroup per (sample, output
plane, 16-cout slice) over the whole K range, the epilogue and the GroupNorm partials in the kernel.  Through the operator ABI
(ldm_op_conv3d with no forced tile or split takes the kernel where the plans do) against torch fp32 on the same bf16 inputs, against the
LDM_CONV_PLANE=0 split-K halo path, and for run-to-run bit stability; the statistics it leaves through the operator-level GroupNorm; the
planner's decisions host side; then a whole UNet plan with the switch off and on."""
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch
from test_gpu_conv_cube import TOL_SAME_ROUNDING, _run_conv
from util import bf16_round, from_ndhwc, pack_conv_weight, pad_vec, rel_l2, rup, to_ndhwc_bf16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "unet_full_24_conv_cfgs_before_conv_plane.json")


@contextlib.contextmanager
def _knob(value):
    old = os.environ.get("LDM_CONV_PLANE")
    os.environ["LDM_CONV_PLANE"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("LDM_CONV_PLANE", None)
        else:
            os.environ["LDM_CONV_PLANE"] = old


CASES = [  # (n, cin, cout, dims, skip, temb, residual)
    (1, 128, 32, (12, 12, 12), None, False, False),         # the minimum: four 32-channel stages
    (1, 192, 64, (12, 12, 12), None, True, False),          # six stages: every buffer is refilled twice
    (1, 128, 32, (7, 12, 9), None, False, True),            # ragged volume, just past the cube kernel's limit
    (2, 128, 48, (8, 7, 12), (64, 64), True, True),         # batch 2, dual-source skip (one two-chunk skip stage), couts that do not fill the last slice
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,cin,cout,dims,skip,temb,residual", CASES)
def test_conv_plane_against_torch_and_the_split_k_halo_path(cuda, built_lib, n, cin, cout, dims, skip, temb, residual):
    kw = dict(n=n, cin=cin, cout=cout, dims=dims, skip=skip, temb=temb, residual=residual)
    with _knob("1"):
        (a, b), ref = _run_conv(cuda, reps=2, **kw)
    assert torch.equal(a, b), "conv3_plane_kernel must reproduce its output bit for bit"
    err = rel_l2(a, bf16_round(ref))
    with _knob("0"):
        (h,), _ = _run_conv(cuda, **kw)
    print(f"conv3_plane_kernel {cin}->{cout} {dims} n={n}: vs torch {err:.3e}, vs LDM_CONV_PLANE=0 {rel_l2(a, h):.3e}")
    assert err <= TOL_SAME_ROUNDING, err
    # both are one bf16 rounding of the same fp32 sum in different orders
    assert rel_l2(a, h) <= 2 * TOL_SAME_ROUNDING, rel_l2(a, h)


@pytest.mark.gpu
def test_conv_plane_leaves_the_6cubed_volumes_to_the_cube_kernel(cuda, built_lib):
    """A 6^3 volume must not take the kernel: the knob changes nothing there, bit for bit (the two kernels sum in different orders)."""
    kw = dict(n=1, cin=128, cout=32, dims=(6, 6, 6), skip=None, temb=True, residual=True)
    with _knob("1"):
        (a,), ref = _run_conv(cuda, **kw)
    with _knob("0"):
        (h,), _ = _run_conv(cuda, **kw)
    assert torch.equal(a, h)
    assert rel_l2(a, bf16_round(ref)) <= TOL_SAME_ROUNDING


@pytest.mark.gpu
def test_conv_plane_statistics_through_the_group_norm(cuda, built_lib):
    """The (sum, sum of squares) slab rows the kernel leaves (one per plane) through gn_fused_apply_kernel, as the plans launch the pair,
    against the same pair with the conv on the split-K path (statistics from the write-through finalize) at LDM_CONV_PLANE=0."""
    import torch.nn.functional as F
    from ldm3d import _lib
    n, cin, cout, dims, groups = 1, 192, 64, (12, 12, 12), 32
    g = torch.Generator().manual_seed(7)
    x = bf16_round(torch.randn((n, cin, *dims), generator=g))
    w = bf16_round(torch.randn((cout, cin, 3, 3, 3), generator=g) / (27 * cin) ** 0.5)
    b = 0.1 * torch.randn((cout,), generator=g)
    gamma = 1.0 + 0.1 * torch.randn((cout,), generator=g)
    beta = 0.1 * torch.randn((cout,), generator=g)
    ref = F.silu(F.group_norm(bf16_round(F.conv3d(x, w, b, padding=1)), groups, gamma, beta, 1e-6))
    cout_pad = rup(cout, 64)
    xa, wp, bp = to_ndhwc_bf16(x).to(cuda), pack_conv_weight(w, cin, cout_pad).to(cuda), pad_vec(b, cout_pad).to(cuda)
    gd, bd = gamma.to(cuda), beta.to(cuda)
    scratch = torch.empty((built_lib.ldm_op_conv3d_gn_scratch_bytes(n, *dims, cout_pad, 8),), dtype=torch.uint8, device=cuda)

    def pair(knob, splitk):
        conv_out = torch.full((n, *dims, cout), float("nan"), dtype=torch.bfloat16, device=cuda)
        gn_out = torch.full((n, *dims, cout), float("nan"), dtype=torch.bfloat16, device=cuda)
        with _knob(knob):
            _lib.check(built_lib.ldm_op_conv3d_gn(xa.data_ptr(), cin, wp.data_ptr(), bp.data_ptr(), gd.data_ptr(), bd.data_ptr(), groups, 1e-6, 1,
                                                  conv_out.data_ptr(), gn_out.data_ptr(), n, *dims, cout, cout_pad, 0, splitk,
                                                  scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return from_ndhwc(conv_out.cpu(), cout), from_ndhwc(gn_out.cpu(), cout)

    conv1, gn1 = pair("1", 0)                  # no forced split: the plane kernel
    conv0, gn0 = pair("0", 8)                  # split over K as the parent planned the 12^3 level
    e_ref, e_conv, e_gn = rel_l2(gn1, bf16_round(ref)), rel_l2(conv1, conv0), rel_l2(gn1, gn0)
    print(f"conv3_plane_kernel -> GroupNorm: pair vs torch {e_ref:.3e}; vs LDM_CONV_PLANE=0: conv {e_conv:.3e}, GroupNorm {e_gn:.3e}")
    assert e_ref <= TOL_SAME_ROUNDING, e_ref
    assert e_conv <= 2 * TOL_SAME_ROUNDING and e_gn <= 2 * TOL_SAME_ROUNDING, (e_conv, e_gn)


def test_conv_plane_is_planned_for_the_12cubed_convs_only(built_lib, monkeypatch):
    """Host side, the benchmark UNet at 24^3.  With every Cin class admitted (LDM_CONV_PLANE_MAX_CIN=768) its ten stride-1 12^3 convs run
    on conv3_plane_kernel (halo code 6), unsplit, ten launches fewer (their finalizes); the convs on the general kernel (code 0) and on
    conv3_cube_kernel (code 5) stay; LDM_CONV_PLANE=0 plans every conv as the commit before the kernel did (tests/golden: its
    ldm_model_plan_conv_cfgs rows).  The DEFAULT admits only the classes that won per op on the GPU (profiles/r07_summary.md: Cin 256
    wins, 512 ties, 768 loses), so without the knob it is the seven convs with a 256-channel main source."""
    import cfgs
    from ldm3d import _lib
    from ldm3d.networks import DiffusionModelUNet

    def launches(model):
        buf = (C.c_int * (4 * 512))()
        k = _lib.lib().ldm_model_plan_conv_cfgs(model._h, b"unet", 1, 24, 24, 24, buf, 512)
        assert 0 < k <= 512, k
        return [[buf[4 * i + j] for j in range(4)] for i in range(k)], _lib.lib().ldm_model_plan_launches(model._h, b"unet", 1, 24, 24, 24)

    code = lambda rows, c: [r for r in rows if r[2] >> 8 == c]   # noqa: E731
    monkeypatch.delenv("LDM_CONV_PLANE", raising=False)
    monkeypatch.delenv("LDM_CONV_PLANE_MAX_CIN", raising=False)
    dflt, n_dflt = launches(DiffusionModelUNet(**cfgs.UNET_FULL))
    monkeypatch.setenv("LDM_CONV_PLANE_MAX_CIN", "768")
    on, n_on = launches(DiffusionModelUNet(**cfgs.UNET_FULL))
    monkeypatch.setenv("LDM_CONV_PLANE", "0")
    off, n_off = launches(DiffusionModelUNet(**cfgs.UNET_FULL))
    assert len(code(on, 6)) == 10 and all(r[3] == 1 for r in code(on, 6)), code(on, 6)
    assert not code(off, 6) and len(on) == len(off) == len(dflt)
    assert len(code(on, 0)) == len(code(off, 0)) == 4 and len(code(on, 5)) == len(code(off, 5)) == 14
    assert n_on <= n_off - 10, (n_on, n_off)
    assert len(code(dflt, 6)) == 7 and all(r[3] == 1 for r in code(dflt, 6)) and n_dflt == n_off - 7, (code(dflt, 6), n_dflt, n_off)
    assert len(code(dflt, 0)) == 4 and len(code(dflt, 5)) == 14
    with open(GOLDEN) as f:
        assert off == json.load(f)["conv_cfgs"]


_PLAN_CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import cfgs
from ldm3d.networks import DiffusionModelUNet
from oracle import unet as ou
cfg = dict(cfgs.UNET_TINY, channels=[64, 128, 256])
sd = ou.init_state_dict(ou.unet_param_shapes(cfg), 0)
m = DiffusionModelUNet(**cfg); m.load_state_dict(sd); m = m.to("cuda:0").eval()
g = torch.Generator().manual_seed(3)
x = torch.randn((1, 4, 24, 24, 24), generator=g).to("cuda:0")
t = torch.tensor([321.0], device="cuda:0")
with torch.no_grad():
    a = m(x=x, timesteps=t).float().cpu(); b = m(x=x, timesteps=t).float().cpu()
    m.enable_graph_replay(True)
    c = [m(x=x, timesteps=t).float().cpu() for _ in range(3)]
assert torch.equal(a, b) and all(torch.equal(a, o) for o in c), "eager runs and graph replays must be bit-stable"
np.save(sys.argv[2], a.numpy())
"""


@pytest.mark.gpu
def test_unet_plan_with_the_plane_kernel_on_and_off(cuda, built_lib, tmp_path):
    """A UNet with a 128-channel 12^3 level (24^3 -> 12^3 -> 6^3) in two child processes, LDM_CONV_PLANE=0 and 1: replay-stable, and the two
    outputs within the 5e-2 that test_gpu_models.py allows an alternative plan of the same network."""
    import numpy as np
    outs = {}
    for v in ("0", "1"):
        f = tmp_path / f"eps_{v}.npy"
        env = dict(os.environ, LDM_CONV_PLANE=v)
        r = subprocess.run([sys.executable, "-c", _PLAN_CHILD, ROOT, str(f)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[v] = torch.from_numpy(np.load(f))
    err = rel_l2(outs["1"], outs["0"])
    print(f"UNet eps, LDM_CONV_PLANE=1 vs 0: rel-L2 {err:.3e}")
    assert err <= 5e-2, err


@pytest.mark.gpu
def test_conv_plane_does_not_spill(built_lib):
    """No scratch: five accumulator tiles and two fragment sets stay in registers (ISA dump of `make asm`, as test_conv_cube_does_not_spill)."""
    csrc = os.path.join(ROOT, "3d-latent-diffusion-model_amd", "csrc")
    res = os.path.join(csrc, "resource_usage.txt")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hip"))]
    if not os.path.exists(res) or os.path.getmtime(res) < max(os.path.getmtime(f) for f in srcs):
        subprocess.run(["make", "-C", csrc, "asm"], check=True, capture_output=True, timeout=900)
    text = open(res).read()
    i = text.index("Function Name: _Z18conv3_plane_kernel")
    block = text[i:i + 2000]
    assert "ScratchSize [bytes/lane]: 0 " in block and "VGPRs Spill: 0 " in block, block
