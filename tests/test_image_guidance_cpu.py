"""Image-space measurement guidance without a GPU: known answers of the fp64 reference (tests/image_guidance_ref.py), argument
validation of ImageConsistencyGuidance, the refusal table, the command line of `inference.py --data-consistency-image`, the new symbols,
and the decoder's data-only plan as a host-side object."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import cfgs
import image_guidance_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ldm_vae_decode_grad_workspace_bytes", "ldm_vae_decode_grad_forward", "ldm_vae_decode_grad_backward",
               "ldm_unet_denoise_step_measured_image", "ldm_image_residual_scratch_bytes", "ldm_op_guidance_x0", "ldm_op_image_residual",
               "ldm_op_guidance_chain")


# ------------------------------------------------------------------------------------------------ the reference's known answers
@pytest.mark.parametrize("pool", [1, 2, 3])
def test_pool_and_its_transpose_are_adjoint(pool):
    """<P u, v> = <u, P^T v>."""
    g = torch.Generator().manual_seed(pool)
    u = torch.randn((2, 3, 2 * pool, 3 * pool, 4 * pool), generator=g, dtype=torch.float64)
    v = torch.randn((2, 3, 2, 3, 4), generator=g, dtype=torch.float64)
    lhs, rhs = float((ir.pool(u, pool) * v).sum()), float((u * ir.pool_t(v, pool)).sum())
    assert lhs == pytest.approx(rhs, rel=1e-12)
    assert float(ir.pool(torch.ones_like(u), pool).min()) == pytest.approx(1.0) and ir.pool(u, pool).shape == v.shape


@pytest.mark.parametrize("pool,tb,wk", [(1, 2, "none"), (2, 1, "frac"), (3, 2, "frac"), (2, 2, "one")])
def test_g_img_is_autograds_gradient_of_the_loss(pool, tb, wk):
    g = torch.Generator().manual_seed(7 + pool)
    y_hat = torch.randn((2, 2, 2 * pool, 2 * pool, 3 * pool), generator=g, dtype=torch.float64)
    target = torch.randn((tb, 2, 2, 2, 3), generator=g, dtype=torch.float64)
    weight = {"none": None, "frac": torch.rand((tb, 2, 2, 2, 3), generator=g, dtype=torch.float64),
              "one": torch.rand((1, 2, 2, 2, 3), generator=g, dtype=torch.float64)}[wk]
    yg = y_hat.clone().requires_grad_(True)
    w = 1.0 if weight is None else weight
    loss = 0.5 * (w * ((F.avg_pool3d(yg, pool) if pool > 1 else yg) - target)).pow(2).sum()
    want, = torch.autograd.grad(loss, yg)
    got, n2 = ir.image_terms(y_hat, target, weight, pool)
    assert float((got - want).norm() / want.norm()) <= 1e-12
    assert torch.allclose(ir.loss(y_hat, target, weight, pool), 0.5 * n2, rtol=1e-14)
    assert float(n2.sum()) == pytest.approx(2.0 * float(loss.detach()), rel=1e-12)


@pytest.mark.parametrize("pred", ["epsilon", "sample", "v_prediction"])
def test_guided_step_equals_the_chained_formulae(pred):
    """guided_step (autograd end to end) == c_x dz / sf + J^T(c_m dz / sf) assembled from image_terms, chain and two explicit VJPs."""
    g = torch.Generator().manual_seed(3)
    k1 = torch.randn((2, 2, 3, 3, 3), generator=g, dtype=torch.float64) * 0.3
    k2 = torch.randn((1, 2, 3, 3, 3), generator=g, dtype=torch.float64) * 0.3
    unet = lambda t: torch.tanh(F.conv3d(t, k1, padding=1))
    decode = lambda z: F.conv3d(F.interpolate(z, scale_factor=2, mode="nearest"), k2, padding=1)
    x = torch.randn((2, 2, 2, 2, 3), generator=g, dtype=torch.float64)
    target = torch.randn((1, 1, 2, 2, 3), generator=g, dtype=torch.float64)
    weight = torch.rand((1, 1, 2, 2, 3), generator=g, dtype=torch.float64)
    abar, sf, pool = 0.41, 0.8, 2
    got, norm, m, grad = ir.guided_step(pred, abar, x, unet, decode, lambda m: x, target, weight, pool, sf, 0.5, True)
    xg = x.clone().requires_grad_(True)
    mg = unet(xg)
    zg = ir.z0(pred, abar, x, m, sf).requires_grad_(True)
    yh = decode(zg)
    g_img, n2 = ir.image_terms(yh.detach(), target, weight, pool)
    dz, = torch.autograd.grad(yh, zg, g_img)
    go, gx = ir.chain(pred, abar, dz, sf)
    dx, = torch.autograd.grad(mg, xg, go)
    want = x - ir.zeta(n2.sqrt(), 0.5, True).reshape(-1, 1, 1, 1, 1) * (gx + dx)
    assert float((got - want).norm() / want.norm()) <= 1e-12 and torch.allclose(norm, n2.sqrt(), rtol=1e-12)
    assert float((grad - (gx + dx)).norm() / grad.norm()) <= 1e-12


# ------------------------------------------------------------------------------------------------ the Python surface
class _Ae:
    latent_channels, out_channels, factor = 8, 2, 4


def test_image_guidance_shares_the_latent_measurements_code(built_lib):
    from ldm3d.guidance import ConsistencyGuidance, ImageConsistencyGuidance
    assert issubclass(ImageConsistencyGuidance, ConsistencyGuidance)
    for name in ("__init__", "check", "device_tensors", "zeta", "residual", "pooled", "_correction"):
        assert getattr(ImageConsistencyGuidance, name) is getattr(ConsistencyGuidance, name), name
    m = ImageConsistencyGuidance(torch.zeros(1, 2, 4, 8, 6), pool=2, scale=0.25, normalize=False)
    assert m.space == "image" and ConsistencyGuidance(torch.zeros(1, 1, 1, 1, 1)).space == "latent"
    assert m.measured_shape((3, 8, 2, 4, 3), _Ae) == (3, 2, 8, 16, 12)
    m.check(m.measured_shape((3, 8, 2, 4, 3), _Ae))
    m.norms = torch.tensor([[4.0], [1.0]])
    rec = m.record(0)
    assert rec["space"] == "image" and (rec["residual_norm_first"], rec["residual_norm_last"], rec["pool"]) == (4.0, 1.0, 2)
    assert "space" not in ConsistencyGuidance(torch.zeros(1, 1, 1, 1, 1)).record(0)


def test_argument_validation(built_lib):
    from ldm3d.guidance import ImageConsistencyGuidance as G
    t = torch.zeros(1, 2, 4, 8, 6)
    with pytest.raises(ValueError, match="autoencoder_model"):
        G(t, pool=2).measured_shape((1, 8, 2, 4, 3), None)
    with pytest.raises(ValueError, match="latent_channels"):
        G(t, pool=2).measured_shape((1, 4, 2, 4, 3), _Ae)
    with pytest.raises(ValueError, match="divide the image dims"):
        G(torch.zeros(1, 2, 2, 5, 4), pool=3).check((1, 2, 8, 16, 12))
    with pytest.raises(ValueError, match="target must be"):
        G(t, pool=2).check((1, 2, 8, 16, 16))
    with pytest.raises(ValueError, match="target must be"):
        G(torch.zeros(1, 1, 4, 8, 6), pool=2).check((1, 2, 8, 16, 12))          # the image's channels, not the latent's
    with pytest.raises(ValueError, match="target must be"):
        G(torch.zeros(3, 2, 4, 8, 6), pool=2).check((2, 2, 8, 16, 12))
    with pytest.raises(ValueError, match=">= 0"):
        G(t, weight=torch.tensor([-1.0]))
    with pytest.raises(ValueError, match="broadcastable"):
        G(t, weight=torch.ones(5, 4, 4))
    with pytest.raises(ValueError, match="pool"):
        G(t, pool=0)
    with pytest.raises(ValueError, match="target must be"):
        G(torch.zeros(2, 4, 8, 6))


def test_refusal_table_is_the_latent_measurements(built_lib):
    """check_measurable is reused as is: the same schedulers and combinations are refused by name."""
    from ldm3d import guidance
    from ldm3d.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, PNDMScheduler, RFlowScheduler
    for cls in (PNDMScheduler, DPMSolverMultistepScheduler, RFlowScheduler):
        with pytest.raises(NotImplementedError, match=cls.__name__):
            guidance.check_measurable(cls(num_train_timesteps=1000))
    ddim = DDIMScheduler(**cfgs.SCHED)
    guidance.check_measurable(ddim)
    for kw, word in ((dict(cfg=2.0), "cfg"), (dict(inpaint=True), "inpainting"), (dict(windows=True), "sliding windows"),
                     (dict(ensemble=True), "ensembles"), (dict(concurrent=True), "sample_concurrent")):
        with pytest.raises(NotImplementedError, match=word):
            guidance.check_measurable(ddim, **kw)


def test_inferer_refuses_before_it_touches_a_model(built_lib):
    """No GPU and no model needed: every refusal happens before the first launch."""
    from ldm3d.guidance import ImageConsistencyGuidance
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.schedulers import DDIMScheduler, PNDMScheduler
    meas = ImageConsistencyGuidance(torch.zeros(1, 2, 4, 8, 6), pool=2)
    x, cond = torch.zeros(1, 8, 2, 4, 3), torch.zeros(1, 8, 2, 4, 3)
    sch = DDIMScheduler(**cfgs.SCHED)
    sch.set_timesteps(4)
    inf = LatentDiffusionInferer(sch)
    with pytest.raises(ValueError, match="autoencoder_model"):
        inf.sample(x, None, object(), conditioning=cond, mode="concat", fused_seed=1, measurement=meas)
    with pytest.raises(ValueError, match="latent_channels"):
        inf.sample(torch.zeros(1, 4, 2, 4, 3), _Ae, object(), conditioning=cond[:, :4], mode="concat", fused_seed=1, measurement=meas)
    with pytest.raises(NotImplementedError, match="cfg"):
        inf.sample(x, _Ae, object(), conditioning=cond, mode="concat", fused_seed=1, cfg=2.0, measurement=meas)
    with pytest.raises(NotImplementedError, match="inpainting"):
        inf.sample(x, _Ae, object(), conditioning=cond, mode="concat", inpaint_latent=x, keep_mask=torch.ones(2, 4, 3), measurement=meas)
    with pytest.raises(NotImplementedError, match="sliding windows"):
        inf.sample_sliding_window(x, _Ae, object(), roi_size=(2, 2, 2), conditioning=cond, fused_seed=1, measurement=meas)
    with pytest.raises(NotImplementedError, match="ensembles"):
        inf.sample_ensemble(2, (8, 2, 4, 3), _Ae, object(), conditioning=cond, measurement=meas)
    with pytest.raises(NotImplementedError, match="sample_concurrent"):
        inf.sample_concurrent([x], _Ae, [object()], conditionings=[cond], mode="concat", measurement=meas)
    pndm = PNDMScheduler(num_train_timesteps=1000)
    pndm.set_timesteps(4)
    with pytest.raises(NotImplementedError, match="PNDMScheduler"):
        LatentDiffusionInferer(pndm).sample(x, _Ae, object(), conditioning=cond, mode="concat", fused_seed=1, measurement=meas)
    assert meas.norms is None


def test_encoder_side_refusals_stay(built_lib):
    """The decoder became differentiable w.r.t. its latent; the encoder did not become differentiable w.r.t. the image."""
    import inspect
    from ldm3d.networks import AutoencoderKL
    src = inspect.getsource(AutoencoderKL._encode) + inspect.getsource(AutoencoderKL.forward)
    assert src.count("NotImplementedError") == 2
    assert "NotImplementedError" not in inspect.getsource(AutoencoderKL.decode)
    assert "no gradient" in AutoencoderKL.decode.__doc__


# ------------------------------------------------------------------------------------------------ inference.py
def _parse(monkeypatch, *extra):
    import inference
    monkeypatch.setattr(sys, "argv", ["inference.py", "-e", os.path.join(ROOT, "config", "environment_synthetic.json"),
                                      "-c", os.path.join(ROOT, "config", "config_synthetic_train.json"), "--steps", "4", *extra])
    return inference.parse_cli()


def test_inference_cli_flag_parses(built_lib, monkeypatch):
    ns = _parse(monkeypatch, "--condition", "p.npz", "--data-consistency-image", "4", "--dc-scale", "0.5", "--dc-no-normalize",
                "--sampler", "ddim", "--metrics")
    assert ns.data_consistency_image == 4 and ns.data_consistency == 0 and ns.dc_scale == 0.5 and ns.dc_no_normalize
    assert _parse(monkeypatch, "--condition", "p.npz").data_consistency_image == 0
    import inference
    assert "--data-consistency-image" in inference.__doc__ and "is not built" not in inference.__doc__


@pytest.mark.parametrize("extra,word", [
    (["--data-consistency-image", "2"], "--condition"),
    (["--data-consistency-image", "-1", "--condition", "p.npz"], "K >= 1"),
    (["--data-consistency-image", "2", "--data-consistency", "2", "--condition", "p.npz"], "exclusive"),
    (["--data-consistency-image", "2", "--condition", "p.npz", "--sampler", "pndm"], "pndm"),
    (["--data-consistency-image", "2", "--condition", "p.npz", "--sampler", "dpm"], "dpm"),
    (["--data-consistency-image", "2", "--condition", "p.npz", "--sampler", "rflow"], "rflow"),
    (["--data-consistency-image", "2", "--condition", "p.npz", "--cfg", "2.0"], "--cfg"),
    (["--data-consistency-image", "2", "--condition", "p.npz", "--sliding-window"], "--sliding-window"),
    (["--data-consistency-image", "2", "--condition", "p.npz", "--chains", "2"], "--chains"),
    (["--data-consistency-image", "2", "--condition", "p.npz", "--likelihood"], "--likelihood"),
    (["--condition", "p.npz", "--dc-scale", "0.5"], "--data-consistency-image"),
])
def test_inference_cli_refusals(built_lib, monkeypatch, capsys, extra, word):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        _parse(monkeypatch, *extra)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ the library, host side
def test_new_symbols_are_exported_and_bound(built_lib):
    from ldm3d import _lib
    for n in NEW_SYMBOLS:
        assert hasattr(built_lib, n), n
        assert n in _lib.SIGNATURES, n
    fields = [f for f, _ in _lib.ImageMeasurement._fields_]
    assert fields == ["target", "target_batch", "weight", "weight_batch", "pool", "scale", "normalize", "inv_scale_factor", "z0", "recon",
                      "dz", "grad_out", "gx", "dx", "norm2", "norm_table", "partials", "vae_workspace", "vae_workspace_bytes"]


def test_scratch_size_is_a_function_of_the_shape(built_lib):
    """One double per (sample, chunk): linear in B, 0 for a refused shape."""
    from ldm3d import _lib
    L = _lib.lib()
    for C, D, H, W, pool in ((2, 6, 12, 9, 3), (1, 8, 8, 20, 4), (1, 5, 7, 11, 1), (1, 96, 96, 96, 4), (1, 144, 176, 112, 4), (1, 96, 96, 96, 1)):
        one = L.ldm_image_residual_scratch_bytes(1, C, D, H, W, pool)
        assert one >= 8 and one % 8 == 0 and L.ldm_image_residual_scratch_bytes(3, C, D, H, W, pool) == 3 * one
        print((C, D, H, W, pool), "chunks per sample:", one // 8)
    assert L.ldm_image_residual_scratch_bytes(1, 1, 96, 96, 96, 4) // 8 >= 256          # many workgroups per sample at the headline image
    assert L.ldm_image_residual_scratch_bytes(1, 1, 8, 8, 9, 2) == 0
    assert L.ldm_image_residual_scratch_bytes(0, 1, 8, 8, 8, 2) == 0
    assert L.ldm_image_residual_scratch_bytes(1, 1, 8, 8, 8, 0) == 0


@pytest.mark.parametrize("name", ["VAE_TINY", "VAE_TINY_ATTN", "VAE_FULL"])
def test_decoder_gradient_plan_is_data_only(built_lib, name):
    """Host-side plans: "dec_x" exists per shape, runs fewer launches than the training plan (no encoder, no column sums, weight
    gradients or exports) and more than the inference decode (it has a backward); the other plans' launch counts are what they were
    before "dec_x" was built on the same handle."""
    from ldm3d import _lib
    from ldm3d.networks import AutoencoderKL
    L = _lib.lib()
    cfg = getattr(cfgs, name)
    m, fresh = AutoencoderKL(**cfg), AutoencoderKL(**cfg)
    d = (2, 4, 3) if name == "VAE_TINY" else (4, 4, 4)
    img = tuple(4 * v for v in d)
    n_x = L.ldm_model_plan_launches(m._h, b"dec_x", 1, *d)
    n_dec = L.ldm_model_plan_launches(m._h, b"dec", 1, *d)
    n_train = L.ldm_model_plan_launches(m._h, b"train", 1, *img)
    print(name, dict(dec_x=n_x, dec=n_dec, train=n_train))
    assert n_dec < n_x < n_train
    assert (n_dec, n_train) == (L.ldm_model_plan_launches(fresh._h, b"dec", 1, *d), L.ldm_model_plan_launches(fresh._h, b"train", 1, *img))
    assert L.ldm_vae_decode_grad_workspace_bytes(m._h, 1, *d) > 0
    assert L.ldm_vae_decode_grad_workspace_bytes(m._h, 1, *d) < L.ldm_vae_train_workspace_bytes(m._h, 1, *img)
    from ldm3d.networks import DiffusionModelUNet
    u = DiffusionModelUNet(**cfgs.UNET_TINY)
    assert L.ldm_vae_decode_grad_workspace_bytes(u._h, 1, *d) == 0 and b"AutoencoderKL" in L.ldm_last_error()
