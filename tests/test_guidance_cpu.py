"""Measurement guidance without a GPU: the fp64 reference formulae (tests/guidance_ref.py) against torch autograd, ldm3d/guidance.py's
host arithmetic against the reference, argument validation, the refusal table, and the backward-plan variants as host-side objects."""
import math

import pytest
import torch
import torch.nn.functional as F

import cfgs
import guidance_ref as gr

PREDS = ("epsilon", "sample", "v_prediction")


def _problem(pool, seed=0, B=2, C=3, dims=(4, 4, 8)):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, C, *dims), generator=g, dtype=torch.float64)
    pdims = tuple(v // pool for v in dims)
    y = torch.randn((B, C, *pdims), generator=g, dtype=torch.float64)
    w = torch.rand((1, C, *pdims), generator=g, dtype=torch.float64)
    k = torch.randn((C, C, 3, 3, 3), generator=g, dtype=torch.float64) * 0.2
    f = lambda t: torch.tanh(F.conv3d(t, k, padding=1))
    return x, y, w, f


@pytest.mark.parametrize("pool", [1, 2])
@pytest.mark.parametrize("pred", PREDS)
def test_reference_gradient_equals_autograd(pred, pool):
    """grad_x L of guidance_ref == autograd of 1/2 |w (P x0_hat(x, f(x)) - y)|^2 through a small differentiable f, to 1e-10."""
    x, y, w, f = _problem(pool, seed=3 + pool)
    abar = 0.37
    a, s = math.sqrt(abar), math.sqrt(1 - abar)
    xg = x.clone().requires_grad_(True)
    m = f(xg)
    x0 = (xg - s * m) / a if pred == "epsilon" else m if pred == "sample" else a * xg - s * m
    loss = 0.5 * (w * (F.avg_pool3d(x0, pool) if pool > 1 else x0) - w * y).pow(2).sum()
    want, = torch.autograd.grad(loss, xg)

    xv = x.clone().requires_grad_(True)
    mv = f(xv)
    vjp = lambda v: torch.autograd.grad(mv, xv, v, retain_graph=True)[0]
    got, norm = gr.grad_x(pred, abar, x, mv.detach(), vjp, y, w, pool)
    err = float((got - want).norm() / want.norm())
    print(f"{pred} pool {pool}: reference vs autograd {err:.2e}")
    assert err <= 1e-10
    r = w * ((F.avg_pool3d(x0, pool) if pool > 1 else x0) - y)
    assert torch.allclose(norm, r.detach().reshape(2, -1).norm(dim=1), rtol=1e-12)


@pytest.mark.parametrize("pred", PREDS)
def test_host_coefficients_equal_the_reference(built_lib, pred):
    from ldm3d import guidance
    for abar in (0.999, 0.5, 0.0047):
        assert guidance.coefficients(pred, abar) == pytest.approx(gr.coefs(pred, abar), rel=1e-15)
    with pytest.raises(ValueError):
        guidance.coefficients("flow", 0.5)


def test_zeta_and_update_match_the_reference(built_lib):
    from ldm3d.guidance import ConsistencyGuidance
    norm = torch.tensor([2.0, 0.0, 1e-20], dtype=torch.float64)
    for normalize in (True, False):
        m = ConsistencyGuidance(torch.zeros(1, 1, 1, 1, 1), scale=0.3, normalize=normalize)
        assert torch.allclose(m.zeta(norm), gr.zeta(norm, 0.3, normalize), rtol=1e-15)
    assert float(gr.zeta(norm, 0.3, True)[1]) == 0.3 / 1e-12


def test_host_residual_equals_the_reference(built_lib):
    from ldm3d.guidance import ConsistencyGuidance
    for pool in (1, 2, 4):
        x, y, w, _ = _problem(pool, seed=9, dims=(4, 8, 8))
        m = ConsistencyGuidance(y, w, pool=pool)
        assert torch.allclose(m.residual(x, y, w), gr.residual(x, y, w, pool), rtol=1e-12, atol=1e-14)


def test_argument_validation(built_lib):
    from ldm3d.guidance import ConsistencyGuidance
    t = torch.zeros(1, 4, 4, 4, 4)
    with pytest.raises(ValueError, match="divide"):
        ConsistencyGuidance(torch.zeros(1, 4, 2, 2, 2), pool=3).check((1, 4, 8, 8, 8))
    with pytest.raises(ValueError, match=">= 0"):
        ConsistencyGuidance(t, weight=torch.tensor([-1.0]))
    with pytest.raises(ValueError, match="target must be"):
        ConsistencyGuidance(t, pool=2).check((1, 4, 8, 8, 6))          # shape mismatch
    with pytest.raises(ValueError, match="target must be"):
        ConsistencyGuidance(torch.zeros(3, 4, 4, 4, 4), pool=2).check((2, 4, 8, 8, 8))   # batch neither 1 nor B
    with pytest.raises(ValueError, match="broadcastable"):
        ConsistencyGuidance(t, weight=torch.ones(5, 4, 4))
    with pytest.raises(ValueError, match="pool"):
        ConsistencyGuidance(t, pool=0)
    ConsistencyGuidance(t, weight=torch.rand(4, 4, 4), pool=2).check((2, 4, 8, 8, 8))


def test_refusal_table_names_what_it_refuses(built_lib):
    from ldm3d import guidance
    from ldm3d.schedulers import (DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, PNDMScheduler, RFlowScheduler)
    for ok in (DDPMScheduler(**cfgs.SCHED), DDIMScheduler(**cfgs.SCHED)):
        assert ok.measurable
        guidance.check_measurable(ok)
    for cls in (PNDMScheduler, DPMSolverMultistepScheduler, RFlowScheduler):
        sch = cls(num_train_timesteps=1000)
        assert not sch.measurable
        with pytest.raises(NotImplementedError, match=cls.__name__):
            guidance.check_measurable(sch)
    ddim = DDIMScheduler(**cfgs.SCHED)
    for kw, word in ((dict(cfg=2.0), "cfg"), (dict(inpaint=True), "inpainting"), (dict(windows=True), "sliding windows"),
                     (dict(ensemble=True), "ensembles"), (dict(concurrent=True), "sample_concurrent")):
        with pytest.raises(NotImplementedError, match=word):
            guidance.check_measurable(ddim, **kw)


def test_backward_plan_variants_are_plans_of_their_own(built_lib, monkeypatch):
    """Host-side plans: the data-only backward has fewer launches than the full one (no column sums, weight gradients or exports); the
    parameter-and-input one adds only conv_in's data gradient: by default the general data-gradient conv (with its split-K finalize
    where the planner splits) and the unpack, with LDM_DGRAD_THIN=1 exactly the weight re-pack and the thin kernel."""
    from ldm3d import _lib
    from ldm3d.networks import DiffusionModelUNet
    L = _lib.lib()
    ch0, dhw = cfgs.UNET_TINY_COND["channels"][0], 8 * 8 * 8
    for thin in (0, 1):
        monkeypatch.setenv("LDM_DGRAD_THIN", str(thin))
        m = DiffusionModelUNet(**cfgs.UNET_TINY_COND)
        n = {k: L.ldm_model_plan_launches(m._h, k.encode(), 1, 8, 8, 8) for k in ("train", "train_px", "train_x")}
        print(thin, n)
        assert n["train_px"] - n["train"] in ((2,) if thin else (2, 3))
        assert n["train_x"] < n["train"] - 10
        ws = L.ldm_unet_train_workspace_bytes(m._h, 1, 8, 8, 8)
        wsi = L.ldm_unet_train_input_workspace_bytes(m._h, 1, 8, 8, 8)
        # all the workspace grows by: the re-packed weights [27][32][channels[0]] bf16 (thin), or the flip-transposed weights
        # [27][64][channels[0]] bf16 and the bf16 gradient of the packed 32-channel input (general)
        grow = 27 * 32 * ch0 * 2 if thin else 27 * 64 * ch0 * 2 + dhw * 32 * 2
        assert wsi >= ws and wsi - ws <= grow + 8192, (thin, wsi - ws, grow)


def test_record_is_per_volume(built_lib):
    """One record per volume of a batch: its own first and last stepped residual norm, never the batch mean; a warm chain's skipped
    rows (left at 0) are not the first."""
    from ldm3d.guidance import ConsistencyGuidance
    m = ConsistencyGuidance(torch.zeros(1, 1, 2, 2, 2), pool=2, scale=0.25, normalize=False)
    assert m.record(0)["residual_norm_first"] is None
    m.norms = torch.tensor([[0.0, 0.0], [4.0, 8.0], [3.0, 6.0], [1.0, 5.0]])
    r0, r1 = m.record(0), m.record(1)
    assert (r0["residual_norm_first"], r0["residual_norm_last"]) == (4.0, 1.0)
    assert (r1["residual_norm_first"], r1["residual_norm_last"]) == (8.0, 5.0)
    assert r0["pool"] == 2 and r0["scale"] == 0.25 and r0["normalize"] is False
