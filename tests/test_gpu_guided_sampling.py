"""Measurement-guided sampling on the GPU (-m gpu): the residual and update kernels against tests/guidance_ref.py (fp64), the fused step
(ldm_unet_denoise_step_measured) against the host composition and against the CPU oracle, teacher-forced per step, and the chain's
contracts through LatentDiffusionInferer.sample: the |r| = 0 division, determinism, untouched caller tensors, refusals.

UNET_TINY_COND, latent (8, 8, 8), 4 DDIM or DDPM steps.  Gates: kernels 1e-5 rel-L2 (fp32 element-wise arithmetic against fp64); fused
step in fp32 mode 1e-3 per step (the gate of test_config0_ddim_teacher_forced_fp32_meets_1e3_per_step); in bf16 mode 1.5 x the
forward's bf16 floor (bf16-mode against fp32-mode model output on the same x_t, measured per step here) + 2e-3.
"""
import pytest
import torch

import cfgs
import guidance_ref as gr
from util import rel_l2

pytestmark = pytest.mark.gpu

CFG = cfgs.UNET_TINY_COND
DIMS = (8, 8, 8)
PREDS = ("epsilon", "sample", "v_prediction")
PRED_ID = {"epsilon": 0, "sample": 1, "v_prediction": 2}
_MODELS = {}


def _sd():
    from oracle import unet as ou
    if "sd" not in _MODELS:
        _MODELS["sd"] = ou.init_state_dict(ou.unet_param_shapes(CFG), 3, gain=0.5)
    return _MODELS["sd"]


def _model(cuda, precision):
    """One module per precision mode, shared by the tests (weights never change)."""
    from ldm3d.networks import DiffusionModelUNet
    if precision not in _MODELS:
        m = DiffusionModelUNet(**CFG)
        m.load_state_dict(_sd())
        m = m.to(cuda).eval()
        if precision == "fp32":
            m.set_precision("fp32")
        _MODELS[precision] = m
    return _MODELS[precision]


def _scheduler(kind, pred, steps=4):
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler
    sch = (DDIMScheduler if kind == "ddim" else DDPMScheduler)(**cfgs.SCHED, prediction_type=pred)
    sch.set_timesteps(steps)
    return sch


def _inputs(B=2, seed=11):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, *DIMS), generator=g)
    cond = torch.randn((B, 4, *DIMS), generator=g)
    return x, cond


def _measurement(pool, weight_kind, target_batch, B=2, seed=5, **kw):
    from ldm3d.guidance import ConsistencyGuidance
    g = torch.Generator().manual_seed(seed)
    pd = tuple(v // pool for v in DIMS)
    target = torch.randn((target_batch, 4, *pd), generator=g)
    weight = {"none": None, "fractional": torch.rand((target_batch, 4, *pd), generator=g),
              "broadcast": torch.rand((4, 1, 1, 1), generator=g)}[weight_kind]
    return ConsistencyGuidance(target, weight, pool=pool, **kw)


def _full_weight(meas):
    return None if meas.weight is None else meas.weight.expand(torch.broadcast_shapes(meas.weight.shape, meas.target.shape))


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("pool,weight_kind,target_batch", [(1, "none", 2), (2, "fractional", 2), (4, "broadcast", 1), (2, "none", 1),
                                                           (1, "fractional", 1), (4, "fractional", 2), (2, "broadcast", 2)])
def test_residual_and_update_kernels_match_the_fp64_reference(cuda, pool, weight_kind, target_batch, pred):
    from ldm3d import _lib
    B, abar = 2, 0.23
    x, m = _inputs(B, seed=17)
    meas = _measurement(pool, weight_kind, target_batch)
    tgt, wgt = meas.device_tensors(x.shape, cuda)
    xd, md = x.to(cuda), m.to(cuda)
    go, gx = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
    n2 = torch.full((B,), float("nan"), device=cuda)
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    args = (xd.data_ptr(), md.data_ptr(), tgt.data_ptr(), tgt.shape[0], _lib.ptr(wgt), 1 if wgt is None else wgt.shape[0],
            abar ** 0.5, (1 - abar) ** 0.5, PRED_ID[pred], pool)
    _lib.check(L.ldm_op_guidance_residual(*args, go.data_ptr(), gx.data_ptr(), n2.data_ptr(), B, 4, *DIMS, s))
    _, _, rgo, rgx, rnorm = gr.residual_terms(pred, abar, x, m, meas.target, _full_weight(meas), pool)
    e_go, e_gx = rel_l2(go.cpu(), rgo), (rel_l2(gx.cpu(), rgx) if pred != "sample" else float(gx.abs().max()))
    e_n = float(((n2.cpu().double().sqrt() - rnorm).abs() / rnorm).max())
    print(f"{pred} pool {pool} weight {weight_kind} target batch {target_batch}: c_m g {e_go:.2e}, c_x g {e_gx:.2e}, |r| {e_n:.2e}")
    assert e_go <= 1e-5 and e_gx <= 1e-5 and e_n <= 1e-5
    go2, gx2, n22 = torch.empty_like(go), torch.empty_like(gx), torch.empty_like(n2)      # the same inputs give the same bits
    _lib.check(L.ldm_op_guidance_residual(*args, go2.data_ptr(), gx2.data_ptr(), n22.data_ptr(), B, 4, *DIMS, s))
    assert torch.equal(go, go2) and torch.equal(gx, gx2) and torch.equal(n2, n22)
    # update: x - zeta_b (gx + dx) with a random dx standing for J^T(c_m g)
    dx = torch.randn(x.shape, generator=torch.Generator().manual_seed(2))
    for normalize in (1, 0):
        prev = xd.clone()
        _lib.check(L.ldm_op_guidance_update(prev.data_ptr(), gx.data_ptr(), dx.to(cuda).data_ptr(), n2.data_ptr(), 0.7, normalize, B,
                                            x[0].numel(), s))
        ref = gr.update(x, gx.cpu().double() + dx.double(), n2.cpu().double().sqrt(), 0.7, bool(normalize))
        e = rel_l2(prev.cpu(), ref)
        print(f"    update normalize={normalize}: {e:.2e}")
        assert e <= 1e-5


# ------------------------------------------------------------------------------------------------ fused step, teacher-forced
def _fused_chain_setup(cuda, model, sch, meas, B, seed):
    x, cond = _inputs(B)
    sampler = sch.device_sampler(seed)
    tbuf = torch.empty((B,), dtype=torch.float32, device=cuda)
    sampler.reset(tbuf)
    state = meas.device_state(x.shape, cuda, len(sch.timesteps))
    return x, cond.to(cuda).contiguous(), sampler, tbuf, state


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
def test_fused_step_matches_the_host_composition_teacher_forced(cuda, kind, pred, precision):
    """Host composition: the module's own forward under autograd (its input VJP), the reference's arithmetic, scheduler.step.  The
    fused step's input is always the host chain's x_t."""
    B, pool = 2, 2
    model = _model(cuda, precision)
    other = _model(cuda, "fp32" if precision == "bf16" else "bf16")
    sch = _scheduler(kind, pred)
    meas = _measurement(pool, "fractional", 1, scale=0.5)
    x, cond, sampler, tbuf, state = _fused_chain_setup(cuda, model, sch, meas, B, seed=7)
    w_full = _full_weight(meas)
    image = torch.empty_like(x, device=cuda)
    ref_norms = []
    for k, t in enumerate(sch.timesteps.tolist()):
        abar = float(sch.alphas_cumprod[int(t)])
        image.copy_(x)
        model.denoise_step_measured(image, tbuf, sampler, state, cond=cond)
        # host composition on the same x_t
        tt = torch.full((B,), float(t), device=cuda)
        xg = x.to(cuda).requires_grad_(True)
        with torch.enable_grad():
            m = model(x=xg, timesteps=tt, cond=cond)
        assert m.requires_grad
        _, _, go, gx, norm = gr.residual_terms(pred, abar, x, m.detach().cpu(), meas.target, w_full, pool)
        ref_norms.append(norm)
        dx, = torch.autograd.grad(m, xg, go.float().to(cuda))
        z = sampler.noise(k, x.shape, cuda) if kind == "ddpm" else None
        with torch.no_grad():
            prev = sch.step(m.detach(), t, x.to(cuda), **({"noise": z} if z is not None else {}))[0]
            m_other = other(x=x.to(cuda), timesteps=tt, cond=cond)
        x_next = gr.update(prev.cpu(), gx + dx.cpu().double(), norm, 0.5, True)
        err = rel_l2(image.cpu(), x_next)
        floor = rel_l2(m.detach().cpu(), m_other.cpu())
        if precision == "fp32":
            print(f"{kind} {pred} fp32 step {k} (t={t}): fused vs host {err:.2e} (gate 1e-3)")
            assert err <= 1e-3, (k, err)
        else:
            print(f"{kind} {pred} bf16 step {k} (t={t}): fused vs host {err:.2e} = {err / floor:.3f} x forward floor {floor:.2e}")
            assert err <= 1.5 * floor + 2e-3, (k, err, floor)
        x = x_next.float()
    torch.cuda.synchronize()
    # the device table [n_steps][B]: every row against that step's fp64 reference norm (of the host forward's m, which is the fused
    # forward's bit for bit in both modes: the same plan on the same x_t)
    table, want = state[1]["norm_table"].cpu().double(), torch.stack(ref_norms)
    assert table.shape == want.shape == (4, B)
    e_tab = float(((table - want).abs() / want).max())
    print(f"{kind} {pred} {precision}: norm table vs reference, worst entry {e_tab:.2e} (gate 1e-5)")
    assert e_tab <= 1e-5


def test_fused_chain_matches_the_cpu_oracle_teacher_forced_fp32(cuda):
    """End to end against the CPU oracle: oracle forward, oracle autograd for J^T, the reference update, 4 DDIM steps (epsilon)."""
    from oracle import unet as ou
    from oracle.schedulers import OracleDDIM
    B, pool = 1, 2
    model = _model(cuda, "fp32")
    sch = _scheduler("ddim", "epsilon")
    osch = OracleDDIM(**cfgs.SCHED)
    osch.set_timesteps(4)
    meas = _measurement(pool, "fractional", 1, B=B, scale=0.5)
    x, cond, sampler, tbuf, state = _fused_chain_setup(cuda, model, sch, meas, B, seed=1)
    w_full = _full_weight(meas)
    image = torch.empty_like(x, device=cuda)
    assert sch.timesteps.tolist() == osch.timesteps.tolist()
    for k, t in enumerate(osch.timesteps.tolist()):
        abar = float(osch.alphas_cumprod[int(t)])
        image.copy_(x)
        model.denoise_step_measured(image, tbuf, sampler, state, cond=cond)
        xg = x.clone().requires_grad_(True)
        m = ou.unet_forward(_sd(), CFG, torch.cat([xg, cond.cpu()], dim=1), torch.tensor([float(t)] * B))
        _, _, go, gx, norm = gr.residual_terms("epsilon", abar, x, m.detach(), meas.target, w_full, pool)
        dx, = torch.autograd.grad(m, xg, go.float())
        prev, _ = osch.step(m.detach(), t, x)
        x_next = gr.update(prev, gx + dx.double(), norm, 0.5, True)
        err = rel_l2(image.cpu(), x_next)
        print(f"oracle chain step {k} (t={t}): fused fp32 mode vs oracle {err:.2e} (gate 1e-3)")
        assert err <= 1e-3, (k, err)
        x = x_next.float()


# ------------------------------------------------------------------------------------------------ chains through the inferer
def _sample(cuda, meas, kind="ddim", pred="epsilon", fused_seed=3, precision="bf16", B=2, **kw):
    from ldm3d.inferer import LatentDiffusionInferer
    sch = _scheduler(kind, pred)
    x, cond = _inputs(B)
    return LatentDiffusionInferer(sch).sample(x.to(cuda), None, _model(cuda, precision), conditioning=cond.to(cuda), mode="concat",
                                              fused_seed=fused_seed, measurement=meas, **kw)


def test_all_zero_weight_equals_scale_zero_and_is_finite(cuda):
    """|r| = 0: zeta = scale / 1e-12 multiplies an exactly zero gradient."""
    from ldm3d.guidance import ConsistencyGuidance
    target = torch.randn((1, 4, 4, 4, 4), generator=torch.Generator().manual_seed(0))
    a = _sample(cuda, ConsistencyGuidance(target, torch.zeros(1), pool=2, scale=1.0))
    b = _sample(cuda, ConsistencyGuidance(target, torch.zeros(1), pool=2, scale=0.0))
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_same_seed_gives_the_same_bits(cuda, kind):
    m1, m2 = _measurement(2, "fractional", 1), _measurement(2, "fractional", 1)
    a, b = _sample(cuda, m1, kind=kind), _sample(cuda, m2, kind=kind)
    assert torch.equal(a, b) and torch.equal(m1.norms, m2.norms)
    assert m1.norms.shape == (4, 2) and bool((m1.norms > 0).all())
    if kind == "ddpm":
        assert not torch.equal(a, _sample(cuda, _measurement(2, "fractional", 1), kind=kind, fused_seed=4))


def test_fused_and_host_driven_chains_agree_and_guidance_pulls_towards_the_target(cuda):
    """The host-driven loop (forward under autograd + scheduler.step) and the fused one start from the same x_T: the first residual norm
    agrees, both chains are finite, and the guided chain ends closer to the target than the unguided one."""
    from ldm3d.inferer import LatentDiffusionInferer
    mf, mh = _measurement(2, "fractional", 1, scale=0.5), _measurement(2, "fractional", 1, scale=0.5)
    fused = _sample(cuda, mf, precision="fp32")
    sch = _scheduler("ddim", "epsilon")
    x, cond = _inputs(2)
    host = LatentDiffusionInferer(sch).sample(x.to(cuda), None, _model(cuda, "fp32"), conditioning=cond.to(cuda), mode="concat", measurement=mh)
    plain = LatentDiffusionInferer(sch).sample(x.to(cuda), None, _model(cuda, "fp32"), conditioning=cond.to(cuda), mode="concat")
    assert torch.isfinite(fused).all() and torch.isfinite(host).all()
    assert mh.norms.shape == mf.norms.shape == (4, 2)
    e0 = float(((mh.norms[0] - mf.norms[0]).abs() / mf.norms[0]).max())
    print(f"first-step |r|: host {mh.norms[0].tolist()} fused {mf.norms[0].tolist()} ({e0:.2e}); final latents fused vs host {rel_l2(fused, host):.2e}")
    assert e0 <= 1e-4
    w = _full_weight(mf)
    res = lambda z: float((w * (torch.nn.functional.avg_pool3d(z.cpu(), 2) - mf.target)).norm())
    print(f"final weighted residual: unguided {res(plain):.3f}, guided {res(fused):.3f}")
    assert res(fused) < res(plain)


def test_callers_tensors_are_unchanged(cuda):
    from ldm3d.inferer import LatentDiffusionInferer
    meas = _measurement(2, "fractional", 1)
    t0, w0 = meas.target.clone(), meas.weight.clone()
    x, cond = _inputs(2)
    xd = x.to(cuda)
    LatentDiffusionInferer(_scheduler("ddpm", "epsilon")).sample(xd, None, _model(cuda, "bf16"), conditioning=cond.to(cuda), mode="concat",
                                                                fused_seed=1, measurement=meas)
    assert torch.equal(xd.cpu(), x) and torch.equal(meas.target, t0) and torch.equal(meas.weight, w0)


def test_warm_start_runs_guided(cuda):
    meas = _measurement(2, "none", 1)
    x, _ = _inputs(2)
    out = _sample(cuda, meas, init_latent=x[:1].to(cuda) * 0.5, start_step=2)
    assert torch.isfinite(out).all()
    assert bool((meas.norms[:2] == 0).all()) and bool((meas.norms[2:] > 0).all())      # rows 0, 1 were never stepped


def test_warm_start_without_input_noise_takes_its_shape_from_init_latent(cuda):
    from ldm3d.inferer import LatentDiffusionInferer
    meas = _measurement(2, "none", 1)
    x, cond = _inputs(2)
    out = LatentDiffusionInferer(_scheduler("ddim", "epsilon")).sample(None, None, _model(cuda, "bf16"), conditioning=cond.to(cuda), mode="concat",
                                                                      fused_seed=5, init_latent=x[:1].to(cuda) * 0.5, start_step=1, measurement=meas)
    assert out.shape == x.shape and torch.isfinite(out).all() and bool((meas.norms[1:] > 0).all())


def test_every_refusal_raises_before_anything_is_launched(cuda):
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.schedulers import DPMSolverMultistepScheduler, PNDMScheduler, RFlowScheduler
    meas = _measurement(2, "none", 1)
    model = _model(cuda, "bf16")
    x, cond = _inputs(1)
    xd, cd = x.to(cuda), cond.to(cuda)
    serial = getattr(model, "_train_serial", 0)
    for cls in (PNDMScheduler, DPMSolverMultistepScheduler, RFlowScheduler):
        sch = cls(num_train_timesteps=1000)
        sch.set_timesteps(4)
        for seed in (None, 1):
            with pytest.raises(NotImplementedError, match=cls.__name__):
                LatentDiffusionInferer(sch).sample(xd, None, model, conditioning=cd, mode="concat", fused_seed=seed, measurement=meas)
    inf = LatentDiffusionInferer(_scheduler("ddim", "epsilon"))
    with pytest.raises(NotImplementedError, match="cfg"):
        inf.sample(xd, None, model, conditioning=cd, mode="concat", fused_seed=1, cfg=2.0, measurement=meas)
    with pytest.raises(NotImplementedError, match="inpainting"):
        inf.sample(xd, None, model, conditioning=cd, mode="concat", fused_seed=1, inpaint_latent=xd, keep_mask=torch.ones(DIMS), measurement=meas)
    with pytest.raises(NotImplementedError, match="sliding windows"):
        inf.sample_sliding_window(xd, None, model, roi_size=(8, 8, 8), conditioning=cd, fused_seed=1, measurement=meas)
    with pytest.raises(NotImplementedError, match="ensembles"):
        inf.sample_ensemble(2, (4, *DIMS), None, model, conditioning=cd, measurement=meas)
    with pytest.raises(NotImplementedError, match="sample_concurrent"):
        inf.sample_concurrent([xd], None, [model], conditionings=[cd], mode="concat", measurement=meas)
    assert getattr(model, "_train_serial", 0) == serial and meas.norms is None          # no training forward ran
    # the C entry itself: a multistep sampler is refused before the forward
    from ldm3d import _lib
    sch = PNDMScheduler(num_train_timesteps=1000)
    sch.set_timesteps(4)
    sampler = sch.device_sampler(0)
    tbuf = torch.zeros((1,), device=cuda)
    with pytest.raises(_lib.LdmError, match="DDPM or DDIM"):
        model.denoise_step_measured(xd.clone(), tbuf, sampler, meas.device_state(xd.shape, cuda, 4), cond=cd)
    # ... and so is a DDIM sampler whose timesteps ascend (DDIM inversion)
    inv = _scheduler("ddim", "epsilon").inversion_sampler()
    assert inv.n_steps > 1 and inv.timesteps[0] < inv.timesteps[-1]
    with pytest.raises(_lib.LdmError, match="ascend"):
        model.denoise_step_measured(xd.clone(), tbuf, inv, meas.device_state(xd.shape, cuda, inv.n_steps), cond=cd)
    assert getattr(model, "_train_serial", 0) == serial
