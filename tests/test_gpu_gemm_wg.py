"""gemm_wg_kernel (csrc/gemm_wg.h): the light GEMM of the 1x1x1 convolutions on operand tiles that a workgroup shares in LDS, against
gemm_light_kernel BIT FOR BIT (same accumulation order, same epilogue, same GroupNorm partial rows) and against torch; its GroupNorm
prologue against the gn_fused_apply_kernel + GEMM pair bit for bit; the planner's choices (knobs LDM_GEMM_WG, LDM_GEMM_WG_GN); registers."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from test_gpu_ops import TOL_SAME_ROUNDING
from util import bf16_round, rel_l2, rup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _Case:
    """One GEMM's device buffers; fill(seed) writes new inputs into the SAME buffers, run(kernel) launches into poisoned outputs."""

    def __init__(self, cuda, M, ca, cb, cout, big, res, stats):
        self.cuda, self.M, self.ca, self.cb, self.cout, self.big = cuda, M, ca, cb, cout, big
        self.K = ca + cb
        self.cout_pad, self.couts = rup(cout, 64), rup(cout, 32)
        self.rows = 64 if big else 32
        self.mt = (M + self.rows - 1) // self.rows
        bf = dict(dtype=torch.bfloat16, device=cuda)
        self.xa = torch.empty((M, ca), **bf)
        self.xb = torch.empty((M, cb), **bf) if cb else None
        self.w = torch.zeros((self.cout_pad, self.K), **bf)
        self.bias = torch.zeros((self.cout_pad,), device=cuda)
        self.r = torch.empty((M, self.couts), **bf) if res else None
        self.want_stats = stats

    def fill(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.xa.copy_(torch.randn((self.M, self.ca), generator=g))
        if self.xb is not None:
            self.xb.copy_(torch.randn((self.M, self.cb), generator=g))
        self.w[:self.cout].copy_(torch.randn((self.cout, self.K), generator=g) / self.K ** 0.5)
        self.bias[:self.cout].copy_(torch.randn((self.cout,), generator=g))
        if self.r is not None:
            self.r.copy_(torch.randn((self.M, self.couts), generator=g))

    def run(self, kernel, gn=None, fold=0):
        """gn = (slabs, nrb, dhw, gamma, beta, groups, eps): the GroupNorm of xa in front of the GEMM"""
        from ldm3d import _lib
        out = torch.full((self.M, self.couts), float("nan"), dtype=torch.bfloat16, device=self.cuda)
        stats = torch.full((self.mt, self.couts, 2), float("nan"), device=self.cuda) if self.want_stats else None
        scratch = torch.full((self.M, self.K), float("nan"), dtype=torch.bfloat16, device=self.cuda) if gn is not None and not fold else None
        slabs, nrb, dhw, gamma, beta, groups, eps = gn if gn is not None else (None, 0, 0, None, None, 0, 0.0)
        _lib.check(_lib.lib().ldm_op_linear_bf16(_ptr(self.xa), self.ca, _ptr(self.xb), self.cb, _ptr(self.w), _ptr(self.bias), _ptr(self.r),
                                                 _ptr(out), _ptr(stats), self.M, self.cout_pad, self.couts, self.big, kernel,
                                                 _ptr(slabs), nrb, dhw, _ptr(gamma), _ptr(beta), groups, eps, fold, _ptr(scratch),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        return out, stats

    def reference(self):
        """fp32 torch on the bf16-rounded inputs, rounded to bf16 like the store"""
        x = torch.cat([self.xa, self.xb], 1) if self.xb is not None else self.xa
        ref = x.float().cpu() @ self.w[:self.couts].float().cpu().t() + self.bias[:self.couts].cpu()
        if self.r is not None:
            ref = ref + self.r.float().cpu()
        return bf16_round(ref)


def _check(case, kernels=(0, 1)):
    for seed in (11, 12):                                   # twice, new inputs in the same buffers: stale LDS, replay stability
        case.fill(seed)
        outs = [case.run(k) for k in kernels]
        o0, s0 = outs[0]
        for o, s in outs[1:]:
            assert torch.equal(o, o0), "gemm_wg_kernel must give gemm_light_kernel's output bit for bit"
            if case.want_stats:
                assert torch.equal(s, s0), "gemm_wg_kernel must give gemm_light_kernel's GroupNorm partial rows bit for bit"
        assert torch.isfinite(o0.float()).all()
        err = rel_l2(o0.float(), case.reference())
        assert err <= TOL_SAME_ROUNDING, err
        if case.want_stats:
            o = o0.double()
            pad = case.mt * case.rows - case.M
            o = torch.cat([o, torch.zeros((pad, case.couts), dtype=torch.float64, device=case.cuda)]).view(case.mt, case.rows, case.couts)
            # fp32 sums of <= 64 stored values (squares up to ~20 each): 64 roundings of 6e-8 x the running magnitude (<= ~300) ~ 1e-3
            assert torch.allclose(s0[..., 0].double(), o.sum(1), rtol=1e-5, atol=1e-3)
            assert torch.allclose(s0[..., 1].double(), (o * o).sum(1), rtol=1e-5, atol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,cout,big,res,stats", [
    (216, 512, 512, 0, True, True),          # out_proj at 6^3: residual + statistics
    (216, 512, 1536, 0, False, False),       # q|k|v at 6^3
    (130, 256, 768, 1, False, True),         # 64-row tiles, ragged last tile of 2 rows
    (70, 128, 96, 0, True, True),            # ragged cout tile: CoutS 96 of CoutPad 128
    (8, 128, 384, 0, False, True),           # fewer rows than one MFMA tile
    (192, 384, 64, 0, False, True),          # odd count of 128-channel blocks
    (210, 256, 256, 0, True, False),         # 2 samples x 105 rows: tiles straddle samples, no statistics
    (256, 256, 256, 0, False, True),         # 2 samples x 128 rows: statistics rows
    (256, 512, 192, 1, True, True),          # 64-row tiles at K = 512: the two-wave 64 x 64 workgroup
    (130, 384, 192, 1, False, True),         # 64-row tiles at K = 384: the 64 x 128 workgroup at its LDS limit, two waves past CoutPad
])
def test_gemm_wg_equals_gemm_light_bit_for_bit(cuda, M, K, cout, big, res, stats):
    _check(_Case(cuda, M, K, 0, cout, big, res, stats))


@pytest.mark.gpu
def test_refused_shapes_stay_on_gemm_light(cuda):
    """Two sources and K = 96: gemm_wg_ok() refuses both, the planner's choice (kernel -1) is gemm_light_kernel, and forcing
    gemm_wg_kernel is an error rather than a wrong answer."""
    from ldm3d import _lib
    for ca, cb in ((256, 256), (96, 0)):
        case = _Case(cuda, 216, ca, cb, 128, 0, True, True)
        _check(case, kernels=(0, -1))
        out = torch.empty((case.M, case.couts), dtype=torch.bfloat16, device=cuda)
        rc = _lib.lib().ldm_op_linear_bf16(_ptr(case.xa), ca, _ptr(case.xb), cb, _ptr(case.w), _ptr(case.bias), None, _ptr(out), None,
                                           case.M, case.cout_pad, case.couts, 0, 1, None, 0, 0, None, None, 0, 0.0, 0, None, None)
        assert rc == -2, rc                                 # LDM_ERR_UNSUPPORTED


@pytest.mark.gpu
@pytest.mark.parametrize("dhw", [216, 105])
@pytest.mark.parametrize("nrb", [1, 5, 12])
@pytest.mark.parametrize("Cc", [256, 512])
def test_group_norm_prologue_equals_the_two_launch_pair_bit_for_bit(cuda, Cc, nrb, dhw):
    """fold 1 (GroupNorm in gemm_wg_kernel's prologue) against fold 0 (gn_fused_apply_kernel into scratch, then the GEMM), two samples with
    clearly different statistics, partial rows computed on the host from the bf16 input; 32- and 64-row tiles (105 rows: tiles straddle the
    samples).  Against torch (fp64 GroupNorm, rounded to bf16, then the product) at the gate test_gpu_ops.py applies to its GroupNorm pairs."""
    groups, eps, n = 32, 1e-6, 2
    big = 1 if nrb == 5 else 0
    case = _Case(cuda, n * dhw, Cc, 0, 384, big, True, True)
    g = torch.Generator().manual_seed(Cc + nrb + dhw)
    gamma = (1.0 + 0.3 * torch.randn((Cc,), generator=g)).to(cuda)
    beta = (0.3 * torch.randn((Cc,), generator=g)).to(cuda)
    for seed in (21, 22):
        case.fill(seed)
        x = case.xa.float().view(n, dhw, Cc)
        x[1] = 3.0 * x[1] + 2.0
        case.xa.copy_(x.view(n * dhw, Cc))
        xd = case.xa.double().view(n, dhw, Cc).cpu()
        bounds = [round(j * dhw / nrb) for j in range(nrb + 1)]
        slabs = torch.stack([torch.stack([xd[i, bounds[j]:bounds[j + 1]].sum(0), (xd[i, bounds[j]:bounds[j + 1]] ** 2).sum(0)], -1)
                             for i in range(n) for j in range(nrb)]).float().to(cuda)          # [n * nrb][C][2]
        gn = (slabs, nrb, dhw, gamma, beta, groups, eps)
        o1, s1 = case.run(1, gn, fold=1)
        for kern in (1, 0):
            o0, s0 = case.run(kern, gn, fold=0)
            assert torch.equal(o1, o0) and torch.equal(s1, s0), (kern, rel_l2(o1.float(), o0.float()))
        xg = xd.view(n, dhw, groups, Cc // groups)
        mean, var = xg.mean((1, 3), keepdim=True), xg.var((1, 3), unbiased=False, keepdim=True)
        xn = ((xg - mean) / torch.sqrt(var + eps)).view(n, dhw, Cc) * gamma.double().cpu() + beta.double().cpu()
        xn = bf16_round(xn.float()).view(n * dhw, Cc)
        ref = xn @ case.w[:case.couts].float().cpu().t() + case.bias[:case.couts].cpu() + case.r.float().cpu()
        err = rel_l2(o1.float(), bf16_round(ref))
        print(f"GroupNorm prologue C={Cc} nrb={nrb} dhw={dhw} big={big}: vs torch {err:.3e}")
        assert err <= TOL_SAME_ROUNDING, err


@pytest.mark.gpu
def test_group_norm_prologue_refuses_what_the_plans_keep_apart(cuda):
    """K = 128 and 17 partial rows stay on the two launches: fold 1 is LDM_ERR_UNSUPPORTED there, not a wrong answer."""
    from ldm3d import _lib
    for Cc, nrb in ((128, 4), (256, 17)):
        case = _Case(cuda, 216, Cc, 0, 128, 0, False, False)
        case.fill(1)
        slabs = torch.zeros((nrb, Cc, 2), device=cuda)
        gb = torch.ones((Cc,), device=cuda)
        out = torch.empty((216, 128), dtype=torch.bfloat16, device=cuda)
        rc = _lib.lib().ldm_op_linear_bf16(_ptr(case.xa), Cc, None, 0, _ptr(case.w), _ptr(case.bias), None, _ptr(out), None, 216, case.cout_pad,
                                           case.couts, 0, 1, _ptr(slabs), nrb, 216, _ptr(gb), _ptr(gb), 32, 1e-6, 1, None, None)
        assert rc == -2, rc


_PLAN_CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
from ldm3d import _lib
from ldm3d.networks import DiffusionModelUNet
from oracle import unet as ou
cfg = dict(spatial_dims=3, in_channels=4, out_channels=4, channels=[256, 256], attention_levels=[False, True],
           num_head_channels=[0, 64], num_res_blocks=1, norm_num_groups=32)
sd = ou.init_state_dict(ou.unet_param_shapes(cfg), 0)
m = DiffusionModelUNet(**cfg); m.load_state_dict(sd); m = m.to("cuda:0").eval()
g = torch.Generator().manual_seed(3)
x = torch.randn((1, 4, 16, 16, 16), generator=g).to("cuda:0")
t = torch.tensor([321.0], device="cuda:0")
with torch.no_grad():
    a = m(x=x, timesteps=t).float().cpu(); b = m(x=x, timesteps=t).float().cpu()
    m.enable_graph_replay(True)
    c = [m(x=x, timesteps=t).float().cpu() for _ in range(3)]
assert torch.isfinite(a).all()
assert torch.equal(a, b) and all(torch.equal(a, o) for o in c), "eager runs and graph replays must be bit-stable"
np.save(sys.argv[2], a.numpy())
print(_lib.lib().ldm_model_plan_launches(m._h, b"unet", 1, 16, 16, 16), sum(k.endswith("attn.qkv.weight") or k.endswith("attn.to_q.weight") for k in sd))
"""


@pytest.mark.gpu
def test_unet_plan_is_bit_identical_across_the_knobs(cuda, built_lib, tmp_path):
    """A UNet with a 256-channel attention level (16^3 -> 8^3: conv3_plane_kernel leaves 8 partial rows in front of every attention block)
    in child processes with (LDM_GEMM_WG, LDM_GEMM_WG_GN) = (0, 0), (1, 0), (1, 1): eager launches and three graph replays agree within
    each, the outputs are identical bit for bit across the three, and the (1, 1) plan has exactly one launch fewer per attention block."""
    import numpy as np
    outs, launches, blocks = {}, {}, 0
    for arm in ((0, 0), (1, 0), (1, 1)):
        f = tmp_path / f"eps_{arm[0]}{arm[1]}.npy"
        env = dict(os.environ, LDM_GEMM_WG=str(arm[0]), LDM_GEMM_WG_GN=str(arm[1]))
        r = subprocess.run([sys.executable, "-c", _PLAN_CHILD, ROOT, str(f)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[arm] = np.load(f)
        launches[arm], blocks = (int(v) for v in r.stdout.strip().splitlines()[-1].split())
    print(f"launches {launches}, attention blocks {blocks}")
    assert np.array_equal(outs[(0, 0)], outs[(1, 0)]) and np.array_equal(outs[(0, 0)], outs[(1, 1)])
    assert blocks > 0 and launches[(0, 0)] == launches[(1, 0)] == launches[(1, 1)] + blocks, (launches, blocks)


def test_knobs_on_the_benchmark_plan(built_lib, monkeypatch):
    """Host side, the benchmark UNet at 24^3: LDM_GEMM_WG picks the kernel of the OP_GEMM_LIGHT rows and changes nothing else; with
    LDM_GEMM_WG_GN the five 12^3 attention blocks lose their GroupNorm launch (the 6^3 ones take the split-K finalize's GroupNorm
    output); the conv configuration rows never change."""
    import cfgs
    from ldm3d import _lib
    from ldm3d.networks import DiffusionModelUNet

    def plan(wg, gn):
        monkeypatch.setenv("LDM_GEMM_WG", str(wg))
        monkeypatch.setenv("LDM_GEMM_WG_GN", str(gn))
        model = DiffusionModelUNet(**cfgs.UNET_FULL)
        buf = (C.c_int * (4 * 512))()
        k = _lib.lib().ldm_model_plan_conv_cfgs(model._h, b"unet", 1, 24, 24, 24, buf, 512)
        assert 0 < k <= 512, k
        return list(buf[:4 * k]), _lib.lib().ldm_model_plan_launches(model._h, b"unet", 1, 24, 24, 24)

    off, wg, fold, gn_alone = plan(0, 0), plan(1, 0), plan(1, 1), plan(0, 1)
    assert off[0] == wg[0] == fold[0] == gn_alone[0]
    assert off[1] == wg[1] == gn_alone[1] > 0, "the fold needs gemm_wg_kernel"
    assert fold[1] == off[1] - 5, (fold[1], off[1])


def test_gemm_wg_does_not_spill(built_lib):
    """No scratch in any gemm_wg_kernel instantiation (resource usage of `make asm`, as test_conv_cube_does_not_spill)."""
    csrc = os.path.join(ROOT, "3d-latent-diffusion-model_amd", "csrc")
    res = os.path.join(csrc, "resource_usage.txt")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hip"))]
    if not os.path.exists(res) or os.path.getmtime(res) < max(os.path.getmtime(f) for f in srcs):
        subprocess.run(["make", "-C", csrc, "asm"], check=True, capture_output=True, timeout=900)
    text = open(res).read()
    blocks = text.split("Function Name: ")[1:]
    mine = [b for b in blocks if b.startswith("_Z14gemm_wg_kernel")]
    assert len(mine) >= 3, [b[:60] for b in mine]
    for b in mine:
        assert "ScratchSize [bytes/lane]: 0 " in b and "VGPRs Spill: 0 " in b, b
