"""conv3_cube_kernel (conv_cube.h): the 3^3 stride-1 convs of volumes up to 6^3 with the weights and the whole volume in LDS once per
(sample, 16-cout slice, 64-channel Cin chunk) workgroup.  Every 6^3 conv shape of the benchmark UNet through the operator ABI (ldm_op_conv3d
with no forced tile or split takes the kernel where the plans do) against torch fp32 on the same bf16 inputs, against the LDM_CONV_CUBE=0
split-K halo path, and for run-to-run bit stability; then the whole UNet plan with the switch off and on."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F
from util import bf16_round, from_ndhwc, pack_conv_weight, pad_vec, rel_l2, rup, to_ndhwc_bf16

pytestmark = pytest.mark.gpu
TOL_SAME_ROUNDING = 3e-4     # as tests/test_gpu_ops.py: identical rounding points, fp32 summation order only
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_conv(cuda, *, n, cin, cout, dims, skip=None, temb=False, residual=False, cube=True, reps=1, seed=0):
    """One conv through ldm_op_conv3d (auto tile / split); returns (bf16 outputs of each repetition, fp32 torch reference)."""
    from ldm3d import _lib
    lib = _lib.lib()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, cin, *dims), generator=g)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g) / (cin * 27) ** 0.5
    b = 0.1 * torch.randn((cout,), generator=g)
    ref = F.conv3d(bf16_round(x), bf16_round(w), b, padding=1)
    cout_pad = rup(cout, 64)
    keep, x1a, x1b, w1, b2, s_a, s_b = [], None, None, None, None, 0, 0
    if skip is not None:
        s_a, s_b = skip
        xs = torch.randn((n, s_a + s_b, *dims), generator=g)
        ws = torch.randn((cout, s_a + s_b, 1, 1, 1), generator=g) / (s_a + s_b) ** 0.5
        bs = 0.1 * torch.randn((cout,), generator=g)
        ref = ref + F.conv3d(bf16_round(xs), bf16_round(ws), bs)
        x1a = to_ndhwc_bf16(xs[:, :s_a]).to(cuda)
        x1b = to_ndhwc_bf16(xs[:, s_a:]).to(cuda) if s_b else None
        w1 = pack_conv_weight(ws, s_a + s_b, cout_pad).to(cuda)
        b2 = pad_vec(bs, cout_pad).to(cuda)
    te = res = None
    if temb:
        tv = torch.randn((n, cout_pad), generator=g)
        ref = ref + tv[:, :cout, None, None, None]
        te = tv.to(cuda)
    if residual:
        rv = bf16_round(torch.randn(ref.shape, generator=g))
        ref = ref + rv
        res = to_ndhwc_bf16(rv).to(cuda)
    xa = to_ndhwc_bf16(x).to(cuda)
    wp = pack_conv_weight(w, cin, cout_pad).to(cuda)
    bp = pad_vec(b, cout_pad).to(cuda)
    m = n * dims[0] * dims[1] * dims[2]
    scratch = torch.empty((64 * m * cout_pad * 4 + 256,), dtype=torch.uint8, device=cuda)
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    outs = []
    old = os.environ.get("LDM_CONV_CUBE")
    os.environ["LDM_CONV_CUBE"] = "1" if cube else "0"
    try:
        for _ in range(reps):
            out = torch.empty((n, *dims, rup(cout, 32)), dtype=torch.bfloat16, device=cuda)
            st = lib.ldm_op_conv3d(xa.data_ptr(), cin, None, 0, wp.data_ptr(), bp.data_ptr(), ptr(x1a), s_a, ptr(x1b), s_b, ptr(w1), ptr(b2),
                                   ptr(te), cout_pad, ptr(res), out.data_ptr(), None, n, *dims, 3, 1, 1, 0, cout, cout_pad, 0, 0,
                                   scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream)
            _lib.check(st)
            torch.cuda.synchronize()
            outs.append(from_ndhwc(out.cpu(), cout))
    finally:
        if old is None:
            os.environ.pop("LDM_CONV_CUBE", None)
        else:
            os.environ["LDM_CONV_CUBE"] = old
    return outs, ref


CASES = [  # (n, cin, cout, dims, skip, temb, residual): every 6^3 conv of the benchmark UNet, then batch 2 and a ragged volume
    (1, 256, 512, (6, 6, 6), None, True, False),           # down_blocks.2 conv1
    (1, 512, 512, (6, 6, 6), (256, 0), False, False),      # down_blocks.2 conv2 + 1x1 skip over 256 channels
    (1, 512, 512, (6, 6, 6), None, True, False),           # ResBlock conv1 (time embedding)
    (1, 512, 512, (6, 6, 6), None, False, True),           # ResBlock conv2 (residual)
    (1, 1024, 512, (6, 6, 6), None, True, False),          # up_blocks.0 conv1 over cat(h, skip)
    (1, 512, 512, (6, 6, 6), (512, 512), False, False),    # up_blocks.0 conv2 + dual-source 1x1 skip over 1024
    (1, 768, 512, (6, 6, 6), None, True, False),           # up_blocks.0 last conv1 over cat(h, 256-channel skip)
    (1, 512, 512, (6, 6, 6), (512, 256), False, False),    # ... its conv2 + dual-source 1x1 skip over 768
    (2, 512, 512, (6, 6, 6), (256, 0), True, False),       # batch 2
    (2, 256, 128, (5, 6, 4), (128, 64), True, True),       # ragged volume, every epilogue term, dual-source skip
]


@pytest.mark.parametrize("n,cin,cout,dims,skip,temb,residual", CASES)
def test_conv_cube_against_torch_and_the_split_k_halo_path(cuda, built_lib, n, cin, cout, dims, skip, temb, residual):
    (a, b), ref = _run_conv(cuda, n=n, cin=cin, cout=cout, dims=dims, skip=skip, temb=temb, residual=residual, cube=True, reps=2)
    assert torch.equal(a, b), "conv3_cube_kernel must reproduce its output bit for bit"
    err = rel_l2(a, bf16_round(ref))
    assert err <= TOL_SAME_ROUNDING, err
    (h,), _ = _run_conv(cuda, n=n, cin=cin, cout=cout, dims=dims, skip=skip, temb=temb, residual=residual, cube=False)
    # both are one bf16 rounding of the same fp32 sum in different orders
    assert rel_l2(a, h) <= 2 * TOL_SAME_ROUNDING, rel_l2(a, h)


def test_conv_cube_is_planned_for_the_6cubed_convs_only(built_lib, monkeypatch):
    """Host side: the benchmark UNet's 14 stride-1 6^3 convs on conv3_cube_kernel (halo code 5), splitk = Cin / 64; LDM_CONV_CUBE=0 puts
    them back on the halo kernel; the number of conv launches stays."""
    import cfgs
    from ldm3d import _lib
    from ldm3d.networks import DiffusionModelUNet

    def launches(model):
        buf = (C.c_int * (4 * 512))()
        k = _lib.lib().ldm_model_plan_conv_cfgs(model._h, b"unet", 1, 24, 24, 24, buf, 512)
        return [(buf[4 * i + 2] >> 8, buf[4 * i + 3]) for i in range(k)], _lib.lib().ldm_model_plan_launches(model._h, b"unet", 1, 24, 24, 24)

    on, n_on = launches(DiffusionModelUNet(**cfgs.UNET_FULL))
    monkeypatch.setenv("LDM_CONV_CUBE", "0")
    off, n_off = launches(DiffusionModelUNet(**cfgs.UNET_FULL))
    cube = [c for c in on if c[0] == 5]
    assert len(cube) == 14 and sorted({c[1] for c in cube}) == [4, 8, 12, 16], cube
    assert not any(c[0] == 5 for c in off) and len(on) == len(off)
    assert n_on <= n_off, (n_on, n_off)


_PLAN_CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import cfgs
from ldm3d.networks import DiffusionModelUNet
from oracle import unet as ou
sd = ou.init_state_dict(ou.unet_param_shapes(cfgs.UNET_FULL), 0)
m = DiffusionModelUNet(**cfgs.UNET_FULL); m.load_state_dict(sd); m = m.to("cuda:0").eval()
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


def test_unet_plan_with_the_cube_kernel_on_and_off(cuda, built_lib, tmp_path):
    """The benchmark UNet (24^3 -> 12^3 -> 6^3) in two child processes, LDM_CONV_CUBE=0 and 1: replay-stable, and the two outputs within the
    distance two correct bf16 evaluations of this network keep: ~3e-2 is what the bf16 plan shows against the oracle;
    test_gpu_models.py holds the fused finalize + GroupNorm plan to 5e-2 of the default one.  Measured: 1.1e-2."""
    import numpy as np
    outs = {}
    for v in ("0", "1"):
        f = tmp_path / f"eps_{v}.npy"
        env = dict(os.environ, LDM_CONV_CUBE=v)
        r = subprocess.run([sys.executable, "-c", _PLAN_CHILD, ROOT, str(f)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[v] = torch.from_numpy(np.load(f))
    err = rel_l2(outs["1"], outs["0"])
    print(f"UNet eps, LDM_CONV_CUBE=1 vs 0: rel-L2 {err:.3e}")
    assert err <= 3e-2, err


def test_conv_cube_does_not_spill(built_lib):
    """No scratch: the kernel keeps its 8 accumulator tiles and two fragment sets in registers (ISA dump of `make asm`, as test_isa_checks.py)."""
    csrc = os.path.join(ROOT, "3d-latent-diffusion-model_amd", "csrc")
    res = os.path.join(csrc, "resource_usage.txt")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hip"))]
    if not os.path.exists(res) or os.path.getmtime(res) < max(os.path.getmtime(f) for f in srcs):
        subprocess.run(["make", "-C", csrc, "asm"], check=True, capture_output=True, timeout=900)
    text = open(res).read()
    i = text.index("Function Name: _Z17conv3_cube_kernel")
    block = text[i:i + 2000]
    assert "ScratchSize [bytes/lane]: 0 " in block and "VGPRs Spill: 0 " in block, block
