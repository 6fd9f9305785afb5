"""Image-space measurement-guided sampling on the GPU (-m gpu): the fused step (ldm_unet_denoise_step_measured_image) against
tests/image_guidance_ref.py on the CPU oracle (autograd through the oracle's UNet and decoder), the fused chain against the host-driven
one through LatentDiffusionInferer.sample, the residual norms' table, the chain's pull towards the measured image, and every refusal.

VAE_TINY has 8 latent channels and 2 image channels, so the UNets here take and return 8: a one-level UNet on latents (2, 4, 3) (image
(8, 16, 12); no downsample, so the odd W is allowed) and UNET_TINY's three levels, concat-conditioned, on (4, 4, 4) (image 16^3).  Gain-0.5
seeded weights, scale 0.2.  Gates, those of test_gpu_guided_sampling.py: the guided x_{t-1} in fp32 mode <= 1e-3 against the fp32 oracle;
in bf16 mode <= 1.5 x floor + 2e-3, the floor being the bf16-emulating oracle's own distance from the fp32 oracle on the same step.  The
step's gradient c_x dz / sf + J^T(c_m dz / sf) (left in the step's scratch) is printed next to it: x_{t-1} at a small scale is dominated
by the scheduler's step, the gradient is not.
"""
import pytest
import torch

import cfgs
import image_guidance_ref as ir
from util import rel_l2

pytestmark = pytest.mark.gpu

UNET_ONE = dict(spatial_dims=3, in_channels=8, out_channels=8, channels=[64], attention_levels=[True], num_head_channels=64,
                num_res_blocks=1, norm_num_groups=32)
UNET_COND = dict(cfgs.UNET_TINY, in_channels=16, out_channels=8)
CASES = {"one": (UNET_ONE, (2, 4, 3), 0), "cond": (UNET_COND, (4, 4, 4), 8)}
VCFG = cfgs.VAE_TINY
SF = 0.9
PREDS = ("epsilon", "sample", "v_prediction")
_MODELS = {}


def _sds(case):
    from oracle import autoencoder as oa
    from oracle import unet as ou
    if ("sd", case) not in _MODELS:
        _MODELS[("sd", case)] = ou.init_state_dict(ou.unet_param_shapes(CASES[case][0]), 3, gain=0.5)
    if "vsd" not in _MODELS:
        _MODELS["vsd"] = ou.init_state_dict(oa.ae_param_shapes(VCFG), 5, gain=0.5)
    return _MODELS[("sd", case)], _MODELS["vsd"]


def _models(cuda, case, precision):
    """(UNet, AutoencoderKL) per case and precision mode, shared by the tests (weights never change)."""
    from ldm3d.networks import AutoencoderKL, DiffusionModelUNet
    key = (case, precision)
    if key not in _MODELS:
        sd, vsd = _sds(case)
        u, v = DiffusionModelUNet(**CASES[case][0]), AutoencoderKL(**VCFG)
        u.load_state_dict(sd)
        v.load_state_dict(vsd)
        u, v = u.to(cuda).eval(), v.to(cuda).eval()
        if precision == "fp32":
            u.set_precision("fp32")
            v.set_precision("fp32")
        _MODELS[key] = (u, v)
    return _MODELS[key]


def _scheduler(kind, pred, steps=4):
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler
    sch = (DDIMScheduler if kind == "ddim" else DDPMScheduler)(**cfgs.SCHED, prediction_type=pred)
    sch.set_timesteps(steps)
    return sch


def _inputs(case, B, seed=11):
    _, dims, cc = CASES[case]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 8, *dims), generator=g)
    cond = torch.randn((B, cc, *dims), generator=g) if cc else None
    return x, cond


def _measurement(case, pool, B=2, target_batch=1, weighted=True, seed=5, **kw):
    from ldm3d.guidance import ImageConsistencyGuidance
    dims = tuple(4 * v // pool for v in CASES[case][1])
    g = torch.Generator().manual_seed(seed)
    target = torch.randn((target_batch, 2, *dims), generator=g) * 0.5
    weight = torch.rand((target_batch, 2, *dims), generator=g) if weighted else None
    return ImageConsistencyGuidance(target, weight, pool=pool, **kw)


def _oracle_step(case, pred, abar, t, x, cond, meas, step, bf, scale):
    from oracle import autoencoder as oa
    from oracle import unet as ou
    sd, vsd = _sds(case)
    B = x.shape[0]
    tt = torch.tensor([float(t)] * B)
    unet = lambda xg: ou.unet_forward(sd, CASES[case][0], xg if cond is None else torch.cat([xg, cond], dim=1), tt, emulate_bf16=bf)
    decode = lambda z: oa.decode(vsd, VCFG, z, emulate_bf16=bf)
    return ir.guided_step(pred, abar, x, unet, decode, step, meas.target, meas.weight, meas.pool, SF, scale, True)


# ------------------------------------------------------------------------------------------------ one fused step against the oracle
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("kind,case", [("ddim", "one"), ("ddpm", "cond"), ("ddpm", "one"), ("ddim", "cond")])
def test_fused_step_matches_the_reference_on_the_oracle(cuda, kind, case, pred, precision):
    B, pool, scale = 2, 2, 0.2
    unet, vae = _models(cuda, case, precision)
    sch = _scheduler(kind, pred)
    meas = _measurement(case, pool, scale=scale)
    x, cond = _inputs(case, B)
    cd = None if cond is None else cond.to(cuda).contiguous()
    sampler = sch.device_sampler(7)
    tbuf = torch.empty((B,), dtype=torch.float32, device=cuda)
    sampler.reset(tbuf)
    state = meas.device_state(x.shape, cuda, len(sch.timesteps), autoencoder=vae, scale_factor=SF)
    t = int(sch.timesteps[0])
    abar = float(sch.alphas_cumprod[t])
    image = x.to(cuda).clone()
    unet.denoise_step_measured(image, tbuf, sampler, state, cond=cd, autoencoder=vae)
    torch.cuda.synchronize()
    z = sampler.noise(0, x.shape, cuda) if kind == "ddpm" else None
    step = lambda m: sch.step(m.float().to(cuda), t, x.to(cuda), **({"noise": z} if z is not None else {}))[0].cpu()
    ref, norm, _, grad = _oracle_step(case, pred, abar, t, x, cond, meas, step, False, scale)
    bufs = state[1]
    got_grad = (bufs["gx"] + bufs["dx"]).cpu()
    err, e_grad = rel_l2(image.cpu(), ref), rel_l2(got_grad, grad)
    e_norm = float(((bufs["norm_table"][0].cpu().double() - norm).abs() / norm).max())
    assert torch.isfinite(image).all() and bool((bufs["norm_table"][1:] == 0).all())
    if precision == "fp32":
        print(f"{kind} {case} {pred} fp32 (t={t}): x_(t-1) vs oracle {err:.2e} (gate 1e-3); gradient {e_grad:.2e}, |r| {e_norm:.2e}")
        assert err <= 1e-3, err
    else:
        ref_bf, _, _, grad_bf = _oracle_step(case, pred, abar, t, x, cond, meas, step, True, scale)
        floor, gfloor = rel_l2(ref_bf, ref), rel_l2(grad_bf, grad)
        print(f"{kind} {case} {pred} bf16 (t={t}): x_(t-1) vs oracle {err:.2e} = {err / floor:.3f} x floor {floor:.2e}; "
              f"gradient {e_grad:.2e} at floor {gfloor:.2e}, |r| {e_norm:.2e}")
        assert err <= 1.5 * floor + 2e-3, (err, floor)


# ------------------------------------------------------------------------------------------------ chains through the inferer
def _sample(cuda, case, meas, kind="ddim", pred="epsilon", fused_seed=3, precision="fp32", B=2, steps=3, **kw):
    from ldm3d.inferer import LatentDiffusionInferer
    unet, vae = _models(cuda, case, precision)
    x, cond = _inputs(case, B)
    ckw = {} if cond is None else dict(conditioning=cond.to(cuda), mode="concat")
    return LatentDiffusionInferer(_scheduler(kind, pred, steps), scale_factor=SF).sample(x.to(cuda), vae, unet, fused_seed=fused_seed,
                                                                                        measurement=meas, **ckw, **kw)


@pytest.mark.parametrize("case", ["one", "cond"])
def test_fused_and_host_driven_chains_agree(cuda, case):
    """3 DDIM steps in fp32 mode from the same x_T: the host-driven loop differentiates through the module's forward and through
    AutoencoderKL.decode with torch autograd.  The first residual norm agrees to 1e-4 (the latent test's comparison and tolerance), and
    the device table equals the host path's per-step norms to 1e-5."""
    mf, mh = _measurement(case, 2, scale=0.2), _measurement(case, 2, scale=0.2)
    fused = _sample(cuda, case, mf)
    host = _sample(cuda, case, mh, fused_seed=None)
    assert torch.isfinite(fused).all() and torch.isfinite(host).all()
    assert mh.norms.shape == mf.norms.shape == (3, 2) and bool((mf.norms > 0).all())
    e0 = float(((mh.norms[0] - mf.norms[0]).abs() / mf.norms[0]).max())
    e_tab = float(((mh.norms - mf.norms).abs() / mh.norms).max())
    print(f"{case}: first-step |r| host {mh.norms[0].tolist()} fused {mf.norms[0].tolist()} ({e0:.2e}); table worst entry {e_tab:.2e}; "
          f"decoded volumes fused vs host {rel_l2(fused, host):.2e}")
    assert e0 <= 1e-4
    assert e_tab <= 1e-5
    assert mf.record(1)["space"] == "image" and mf.record(1)["residual_norm_last"] == float(mf.norms[-1, 1])


def test_guided_chain_ends_closer_to_the_measured_image(cuda):
    """pool = 2, 4 DDIM steps from the same seed: the decoded volume of the guided chain has a smaller weighted pooled residual than the
    unguided chain's; the same seed gives the same bits; the caller's tensors are untouched."""
    from ldm3d.inferer import LatentDiffusionInferer
    case = "cond"
    meas, again = _measurement(case, 2, scale=0.5), _measurement(case, 2, scale=0.5)
    t0, w0 = meas.target.clone(), meas.weight.clone()
    guided = _sample(cuda, case, meas, steps=4)
    assert torch.equal(guided, _sample(cuda, case, again, steps=4)) and torch.equal(meas.norms, again.norms)
    assert torch.equal(meas.target, t0) and torch.equal(meas.weight, w0)
    unet, vae = _models(cuda, case, "fp32")
    x, cond = _inputs(case, 2)
    plain = LatentDiffusionInferer(_scheduler("ddim", "epsilon", 4), scale_factor=SF).sample(x.to(cuda), vae, unet, conditioning=cond.to(cuda),
                                                                                           mode="concat", fused_seed=3)
    res = lambda v: float(ir.residual(v.cpu(), meas.target, meas.weight, 2).norm())
    print(f"final weighted image residual: unguided {res(plain):.4f}, guided {res(guided):.4f}; per-step |r| {meas.norms.tolist()}")
    assert res(guided) < res(plain)


def test_bf16_chain_with_warm_start_runs(cuda):
    meas = _measurement("one", 4, weighted=False, target_batch=2)
    x, _ = _inputs("one", 2)
    out = _sample(cuda, "one", meas, kind="ddpm", precision="bf16", steps=4, init_latent=x[:1].to(cuda) * 0.5, start_step=2)
    assert out.shape == (2, 2, 8, 16, 12) and torch.isfinite(out).all()
    assert bool((meas.norms[:2] == 0).all()) and bool((meas.norms[2:] > 0).all())


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_raises_before_anything_is_launched(cuda):
    from ldm3d import _lib
    from ldm3d.guidance import ImageConsistencyGuidance
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.networks import AutoencoderKL
    from ldm3d.schedulers import DPMSolverMultistepScheduler, PNDMScheduler, RFlowScheduler
    case = "cond"
    unet, vae = _models(cuda, case, "bf16")
    meas = _measurement(case, 2)
    x, cond = _inputs(case, 1)
    xd, cd = x.to(cuda), cond.to(cuda)
    serial, dserial = getattr(unet, "_train_serial", 0), getattr(vae, "_dec_serial", 0)
    for cls in (PNDMScheduler, DPMSolverMultistepScheduler, RFlowScheduler):
        sch = cls(num_train_timesteps=1000)
        sch.set_timesteps(4)
        for seed in (None, 1):
            with pytest.raises(NotImplementedError, match=cls.__name__):
                LatentDiffusionInferer(sch).sample(xd, vae, unet, conditioning=cd, mode="concat", fused_seed=seed, measurement=meas)
    inf = LatentDiffusionInferer(_scheduler("ddim", "epsilon"), scale_factor=SF)
    kw = dict(conditioning=cd, mode="concat", fused_seed=1, measurement=meas)
    with pytest.raises(NotImplementedError, match="cfg"):
        inf.sample(xd, vae, unet, cfg=2.0, **kw)
    with pytest.raises(NotImplementedError, match="inpainting"):
        inf.sample(xd, vae, unet, inpaint_latent=xd, keep_mask=torch.ones(4, 4, 4), **kw)
    with pytest.raises(NotImplementedError, match="sliding windows"):
        inf.sample_sliding_window(xd, vae, unet, roi_size=(4, 4, 4), conditioning=cd, fused_seed=1, measurement=meas)
    with pytest.raises(NotImplementedError, match="ensembles"):
        inf.sample_ensemble(2, (8, 4, 4, 4), vae, unet, conditioning=cd, measurement=meas)
    with pytest.raises(NotImplementedError, match="sample_concurrent"):
        inf.sample_concurrent([xd], vae, [unet], conditionings=[cd], mode="concat", measurement=meas)
    with pytest.raises(ValueError, match="autoencoder_model"):
        inf.sample(xd, None, unet, **kw)
    other = AutoencoderKL(**dict(VCFG, latent_channels=4)).to(cuda).eval()             # a VAE whose latent channels differ
    with pytest.raises(ValueError, match="latent_channels"):
        inf.sample(xd, other, unet, **kw)
    with pytest.raises(ValueError, match="target must be"):                            # a latent-shaped target is not an image-shaped one
        inf.sample(xd, vae, unet, **dict(kw, measurement=ImageConsistencyGuidance(torch.zeros(1, 8, 2, 2, 2), pool=2)))
    assert getattr(unet, "_train_serial", 0) == serial and getattr(vae, "_dec_serial", 0) == dserial and meas.norms is None
    # the C entry itself
    state = meas.device_state(xd.shape, cuda, 4, autoencoder=vae, scale_factor=SF)
    tbuf = torch.zeros((1,), device=cuda)
    pndm = PNDMScheduler(num_train_timesteps=1000)
    pndm.set_timesteps(4)
    with pytest.raises(_lib.LdmError, match="DDPM or DDIM"):
        unet.denoise_step_measured(xd.clone(), tbuf, pndm.device_sampler(0), state, cond=cd, autoencoder=vae)
    inv = _scheduler("ddim", "epsilon").inversion_sampler()
    with pytest.raises(_lib.LdmError, match="ascend"):
        unet.denoise_step_measured(xd.clone(), tbuf, inv, state, cond=cd, autoencoder=vae)
    sampler = _scheduler("ddim", "epsilon").device_sampler(0)
    sampler.reset(tbuf)
    with pytest.raises(_lib.LdmError, match="latent_channels"):
        unet.denoise_step_measured(xd.clone(), tbuf, sampler, state, cond=cd, autoencoder=other)
    with pytest.raises(_lib.LdmError, match="AutoencoderKL"):
        unet.denoise_step_measured(xd.clone(), tbuf, sampler, state, cond=cd, autoencoder=unet)
    with pytest.raises(_lib.LdmError, match="go together"):
        unet.denoise_step_measured(xd.clone(), tbuf, sampler, state, cond=cd)
    state[0].pool = 3                                                                  # does not divide the image dims
    with pytest.raises(_lib.LdmError, match="pool"):
        unet.denoise_step_measured(xd.clone(), tbuf, sampler, state, cond=cd, autoencoder=vae)
    torch.cuda.synchronize()
    assert bool((state[1]["norm_table"] == 0).all()) and getattr(unet, "_train_serial", 0) == serial
