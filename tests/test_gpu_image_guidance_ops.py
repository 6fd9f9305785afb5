"""The image-space guidance kernels on the GPU (-m gpu): ldm_op_guidance_x0, ldm_op_image_residual (image_residual_kernel and its fold)
and ldm_op_guidance_chain against tests/image_guidance_ref.py (fp64).

Shapes (C, D, H, W, pool): a cube edge of 3 with an odd W, pool 4 with W = 20 (five cubes per row), pool 2, and the voxel-identity path at
sizes that are no multiple of anything; B = 2, target / weight batch 1 and B, with, without and with a fractional weight.  Gates, the
latent kernels' in test_gpu_guided_sampling.py: rel-L2 <= 1e-5 for g_img, z0, grad_out and gx, relative 1e-5 for norm2 (fp32 element-wise
arithmetic and a double fold against fp64).  A repeat gives the same bits, slot 0 at B = 1 equals slot 0 at B = 2, g_img may alias y_hat.
One more shape has more cubes per row than a tile holds and more than one chunk, so that the segment and chunk edges are walked.
"""
import pytest
import torch

import image_guidance_ref as ir
from util import rel_l2

pytestmark = pytest.mark.gpu

SHAPES = [(2, 6, 12, 9, 3), (1, 8, 8, 20, 4), (2, 4, 6, 10, 2), (1, 5, 7, 11, 1)]
PRED_ID = {"epsilon": 0, "sample": 1, "v_prediction": 2}


def _problem(C, D, H, W, pool, B, tb, weight_kind, seed=3):
    g = torch.Generator().manual_seed(seed)
    y_hat = torch.randn((B, C, D, H, W), generator=g)
    pd = (C, D // pool, H // pool, W // pool)
    target = torch.randn((tb, *pd), generator=g)
    weight = {"none": None, "ones": torch.ones((1, *pd)), "fractional": torch.rand((tb, *pd), generator=g)}[weight_kind]
    return y_hat, target, weight


def _run(cuda, y_hat, target, weight, pool, alias=False):
    from ldm3d import _lib
    L = _lib.lib()
    B, C, D, H, W = y_hat.shape
    yd, td = y_hat.to(cuda).contiguous(), target.to(cuda).contiguous()
    wd = None if weight is None else weight.to(cuda).contiguous()
    nbytes = int(L.ldm_image_residual_scratch_bytes(B, C, D, H, W, pool))
    assert nbytes >= 8 * B
    part = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=cuda)
    g = yd if alias else torch.full_like(yd, float("nan"))
    n2 = torch.full((B,), float("nan"), device=cuda)
    _lib.check(L.ldm_op_image_residual(yd.data_ptr(), td.data_ptr(), td.shape[0], _lib.ptr(wd), 1 if wd is None else wd.shape[0], pool,
                                       g.data_ptr(), n2.data_ptr(), part.data_ptr(), nbytes, B, C, D, H, W,
                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return g, n2, part


@pytest.mark.parametrize("tb,weight_kind", [(1, "none"), (2, "fractional"), (1, "fractional"), (2, "none"), (2, "ones")])
@pytest.mark.parametrize("C,D,H,W,pool", SHAPES + [(1, 4, 4, 1040, 2), (3, 24, 24, 40, 1)])
def test_image_residual_matches_the_fp64_reference(cuda, C, D, H, W, pool, tb, weight_kind):
    B = 2
    y_hat, target, weight = _problem(C, D, H, W, pool, B, tb, weight_kind)
    g, n2, part = _run(cuda, y_hat, target, weight, pool)
    rg, rn2 = ir.image_terms(y_hat, target, weight, pool)
    e_g, e_n = rel_l2(g.cpu(), rg), float(((n2.cpu().double() - rn2).abs() / rn2).max())
    print(f"{(C, D, H, W)} pool {pool} target batch {tb} weight {weight_kind}: g_img {e_g:.2e}, norm2 {e_n:.2e}, "
          f"{part.numel() // B} chunk(s) per sample")
    assert torch.isfinite(g).all() and torch.isfinite(part).all()
    assert e_g <= 1e-5 and e_n <= 1e-5
    g2, n22, part2 = _run(cuda, y_hat, target, weight, pool)                    # the same inputs give the same bits
    assert torch.equal(g, g2) and torch.equal(n2, n22) and torch.equal(part, part2)
    ga, n2a, _ = _run(cuda, y_hat, target, weight, pool, alias=True)            # in place
    assert torch.equal(ga, g) and torch.equal(n2a, n2)
    sl = lambda t: None if t is None else t[:1]                                 # slot 0 does not depend on B
    g1, n21, _ = _run(cuda, y_hat[:1], sl(target), sl(weight), pool)
    assert torch.equal(g1[0], g[0]) and torch.equal(n21[0], n2[0])


@pytest.mark.parametrize("pred", ["epsilon", "sample", "v_prediction"])
def test_x0_and_chain_kernels_match_the_fp64_reference(cuda, pred):
    from ldm3d import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(8)
    abar, sf = 0.23, 0.83
    for shape in ((2, 8, 2, 4, 3), (1, 4, 5, 7, 11)):
        x, m, dz = (torch.randn(shape, generator=g) for _ in range(3))
        xd, md, dzd = x.to(cuda), m.to(cuda), dz.to(cuda)
        z0, go, gx = (torch.full_like(xd, float("nan")) for _ in range(3))
        coef = (abar ** 0.5, (1 - abar) ** 0.5, PRED_ID[pred], 1.0 / sf)
        _lib.check(L.ldm_op_guidance_x0(xd.data_ptr(), md.data_ptr(), *coef, z0.data_ptr(), x.numel(), s))
        _lib.check(L.ldm_op_guidance_chain(dzd.data_ptr(), *coef, go.data_ptr(), gx.data_ptr(), x.numel(), s))
        torch.cuda.synchronize()
        rgo, rgx = ir.chain(pred, abar, dz, sf)
        e_z, e_go = rel_l2(z0.cpu(), ir.z0(pred, abar, x, m, sf)), rel_l2(go.cpu(), rgo)
        e_gx = rel_l2(gx.cpu(), rgx) if pred != "sample" else float(gx.abs().max())
        print(f"{pred} {shape}: z0 {e_z:.2e}, grad_out {e_go:.2e}, gx {e_gx:.2e}")
        assert e_z <= 1e-5 and e_go <= 1e-5 and e_gx <= 1e-5
        z02 = torch.empty_like(z0)
        _lib.check(L.ldm_op_guidance_x0(xd.data_ptr(), md.data_ptr(), *coef, z02.data_ptr(), x.numel(), s))
        assert torch.equal(z0, z02)


def test_op_entries_refuse_before_they_launch(cuda):
    from ldm3d import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    y = torch.zeros((2, 1, 4, 4, 4), device=cuda)
    t = torch.zeros((1, 1, 2, 2, 2), device=cuda)
    g, n2 = torch.full_like(y, 7.0), torch.full((2,), 7.0, device=cuda)
    part = torch.zeros((64,), dtype=torch.float64, device=cuda)
    ok = (y.data_ptr(), t.data_ptr(), 1, None, 1, 2, g.data_ptr(), n2.data_ptr(), part.data_ptr(), part.numel() * 8, 2, 1, 4, 4, 4, s)

    def bad(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.ldm_op_image_residual(*a)
    assert bad(a0=None) == -1 and bad(a1=None) == -1 and bad(a6=None) == -1 and bad(a8=None) == -1
    assert bad(a5=3) == -1 and b"pool" in L.ldm_last_error()
    assert bad(a5=0) == -1
    assert bad(a2=3) == -1 and b"target_batch" in L.ldm_last_error()
    assert bad(a3=t.data_ptr(), a4=3) == -1 and b"weight_batch" in L.ldm_last_error()
    assert bad(a9=0) == -5
    assert bad(a8=part.data_ptr() + 4) == -5
    assert bad(a10=0) == -1
    assert L.ldm_op_guidance_x0(y.data_ptr(), y.data_ptr(), 0.0, 1.0, 0, 1.0, g.data_ptr(), y.numel(), s) == -1
    assert L.ldm_op_guidance_x0(y.data_ptr(), y.data_ptr(), 0.5, 0.5, 3, 1.0, g.data_ptr(), y.numel(), s) == -1
    assert L.ldm_op_guidance_chain(None, 0.5, 0.5, 0, 1.0, g.data_ptr(), g.data_ptr(), y.numel(), s) == -1
    torch.cuda.synchronize()
    assert bool((g == 7.0).all()) and bool((n2 == 7.0).all())
    assert L.ldm_op_image_residual(*ok) == 0
