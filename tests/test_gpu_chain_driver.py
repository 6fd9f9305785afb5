"""The branches of the inferer's chains that no other GPU test pins (-m gpu): guided DDIM inversion, full latent and windowed, fused and
host-driven; the intermediates of a fused chain, plain and inpainting; and the host-driven windowed inpainting chain against the fused
one.  The first two compare the inferer with the hand-driven calls it stands for, bit for bit; the last is gated like the other
host-against-fused comparisons."""
import functools

import pytest
import torch

import cfgs
from util import rel_l2

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _unet(tame=False):
    """tame: the output projection scaled by 0.1 and fp32 arithmetic, as tests/test_gpu_sliding.py compares a host-driven loop with the
    device sampler (a random-weight bf16 UNet multiplies a last-bit difference from step to step)"""
    from ldm3d.networks import DiffusionModelUNet
    from oracle import unet as ou
    m = DiffusionModelUNet(**cfgs.UNET_TINY_COND)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfgs.UNET_TINY_COND), 1))
    if tame:
        with torch.no_grad():
            for name, p in m.named_parameters():
                if name.startswith("out.2.conv."):
                    p.mul_(0.1)
    m = m.to(torch.device("cuda:0")).eval()
    if tame:
        m.set_precision("fp32")
    return m


def _ddim(n):
    from ldm3d.schedulers import DDIMScheduler
    sch = DDIMScheduler(**cfgs.SCHED)
    sch.set_timesteps(n)
    return sch


def _count(m, name):
    calls, fn = [], getattr(m, name)

    def counted(*a, **kw):
        calls.append(1)
        return fn(*a, **kw)
    setattr(m, name, counted)
    return calls, lambda: delattr(m, name)


class _Latent:
    """Stands where the autoencoder stands and decodes nothing: the chain's latents come back as they are."""

    @staticmethod
    def decode_stage_2_outputs(z):
        return z


def test_guided_inversion_full_windowed_and_host_driven(cuda):
    """invert(cfg=...): the fused loop == the host-driven one; on a grid of one window invert(roi_size, cfg) == invert(cfg); on two
    windows it is the hand-driven guided windowed step on the inversion sampler (tbuf of 2 x sw_batch_size entries).  n_steps calls each."""
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.sliding import WindowGrid
    m, sch = _unet(), _ddim(10)
    inf = LatentDiffusionInferer(sch)
    g = torch.Generator(device=cuda).manual_seed(41)
    z = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g) * 0.5
    cond = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g)
    with torch.no_grad():
        host = inf.invert(z, m, conditioning=cond, n_steps=4, cfg=2.0, fused=False)
        plain = inf.invert(z, m, conditioning=cond, n_steps=4)
        for name, kw in (("denoise_step", {}), ("denoise_step_windows", dict(roi_size=(8, 8, 8)))):
            calls, undo = _count(m, name)
            try:
                got = inf.invert(z, m, conditioning=cond, n_steps=4, cfg=2.0, **kw)
            finally:
                undo()
            assert len(calls) == 4 and torch.equal(got, host), (name, rel_l2(got, host))
        assert torch.isfinite(host).all() and not torch.equal(host, plain) and not torch.equal(host, z)
        shape = (1, 4, 8, 8, 13)
        z2 = torch.randn(shape, device=cuda, generator=g) * 0.5
        c2 = torch.randn(shape, device=cuda, generator=g)
        grid = WindowGrid(shape[2:], (8, 8, 8))
        assert grid.n_windows == 2
        smp, tbuf, x = sch.inversion_sampler(4), torch.empty((2,), device=cuda), z2.clone()
        smp.reset(tbuf)
        for _ in range(4):
            m.denoise_step_windows(x, tbuf, smp, grid, cond_windows=grid.gather(c2), sw_batch_size=1, guidance=2.0, guidance_fill=-1.0)
        got = inf.invert(z2, m, conditioning=c2, n_steps=4, cfg=2.0, roi_size=(8, 8, 8), sw_batch_size=1)
    assert torch.equal(got, x) and torch.isfinite(x).all() and not torch.equal(x, z2)


def test_fused_chain_keeps_its_intermediates(cuda):
    """sample(save_intermediates=True, fused_seed=...): one intermediate per call made AT a timestep divisible by intermediate_steps,
    each the latent that call left (a copy: the fused chain updates one image in place), over the scheduler's timesteps for a plain chain
    and over the repaint sampler's rows for an inpainting one."""
    from ldm3d.inferer import LatentDiffusionInferer
    m, sch = _unet(), _ddim(6)
    inf = LatentDiffusionInferer(sch, scale_factor=2.0)
    assert sch.timesteps.tolist() == [830, 664, 498, 332, 166, 0]
    g = torch.Generator(device=cuda).manual_seed(43)
    noise = torch.randn((2, 4, 8, 8, 8), device=cuda, generator=g)
    cond = torch.randn((2, 4, 8, 8, 8), device=cuda, generator=g)
    known = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g) * 0.5
    keep = (torch.rand((8, 8, 8), device=cuda, generator=g) < 0.5).float()
    with torch.no_grad():
        for inpaint in (False, True):
            kw = dict(inpaint_latent=known, keep_mask=keep, jump_length=2, n_resample=2) if inpaint else {}
            smp = sch.repaint_sampler(known, keep, 2, 2, 5) if inpaint else sch.device_sampler(5)
            assert len(smp.timesteps) == (10 if inpaint else 6)
            tbuf, x, want = torch.empty((2,), device=cuda), noise.clone(), []
            smp.reset(tbuf)
            for t in smp.timesteps:
                m.denoise_step(x, tbuf, smp, cond=cond)
                if t % 332 == 0:
                    want.append(x / 2.0)
            out, inter = inf.sample(noise, _Latent(), m, conditioning=cond, mode="concat", fused_seed=5, save_intermediates=True,
                                    intermediate_steps=332, **kw)
            assert len(inter) == len(want) == sum(t % 332 == 0 for t in smp.timesteps) >= 3
            assert torch.equal(out, x / 2.0) and all(torch.equal(a, b) for a, b in zip(inter, want))
            assert torch.equal(inter[-1], out) and not torch.equal(inter[0], inter[1])


@pytest.mark.parametrize("kind", ["ddpm", "flow"])
def test_host_driven_windowed_inpainting_agrees_with_the_fused_one(cuda, kind):
    """sample_sliding_window(inpaint_latent, keep_mask) host-driven (gather, forward per chunk, blend, the scheduler's step, repaint_merge)
    on a RepaintSampler's own draws against the fused windowed chain of the same seed: latent 13 x 14 x 17 in 12 windows of 8^3, 5 per
    call, 6 timesteps with jump_length = n_resample = 2, 10 UNet calls.  DDPM draws step noise on every row but the last; rectified flow
    takes ``next_timestep`` from the row's level, which a jump sets back.  The gate is tests/test_gpu_repaint.py's for the full latent:
    1e-5 rel-L2, the project's gate for a host-driven against a fused chain, or twice the yardstick were that above 5e-6; the yardstick
    is the plain windowed 6-step DDIM chain, host-driven against fused, on the same model.  Over the whole latent and over the
    regenerated region alone (the last merge restores the kept region whatever the steps did)."""
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.schedulers import DDPMScheduler, RFlowScheduler
    m = _unet(True)
    g = torch.Generator(device=cuda).manual_seed(47)
    shape = (1, 4, 13, 14, 17)
    noise = torch.randn(shape, device=cuda, generator=g)
    known = torch.randn(shape, device=cuda, generator=g) * 0.5
    cond = torch.randn(shape, device=cuda, generator=g)
    keep = torch.ones(shape[2:], device=cuda)
    keep[3:11, 5:9, 6:15] = 0.0                              # the region crosses window seams
    if kind == "ddpm":
        sch = DDPMScheduler(**dict(cfgs.SCHED, num_train_timesteps=6))
    else:
        sch = RFlowScheduler(num_train_timesteps=1000)
        sch.set_timesteps(6)
    inf = LatentDiffusionInferer(sch)
    sw = dict(sw_batch_size=5, conditioning=cond)
    with torch.no_grad():
        plain = LatentDiffusionInferer(_ddim(6))
        yard = rel_l2(plain.sample_sliding_window(noise, None, m, (8, 8, 8), **sw),
                      plain.sample_sliding_window(noise, None, m, (8, 8, 8), fused_seed=9, **sw))
        rs = sch.repaint_sampler(known, keep, 2, 2, seed=9)
        draw = {"step": rs.noise, "known": rs.noise_known, "jump": rs.noise_jump}
        calls, undo = _count(m, "forward")
        try:
            host = inf.sample_sliding_window(noise, None, m, (8, 8, 8), inpaint_latent=known, keep_mask=keep, jump_length=2, n_resample=2,
                                             inpaint_noise=lambda stream, k: draw[stream](k, shape, cuda), **sw)
        finally:
            undo()
        fused = inf.sample_sliding_window(noise, None, m, (8, 8, 8), fused_seed=9, inpaint_latent=known, keep_mask=keep, jump_length=2,
                                          n_resample=2, **sw)
        other = inf.sample_sliding_window(noise, None, m, (8, 8, 8), fused_seed=10, inpaint_latent=known, keep_mask=keep, jump_length=2,
                                          n_resample=2, **sw)
    kp = (keep != 0).expand(shape)
    err, err_new = rel_l2(host, fused), rel_l2(host[~kp], fused[~kp])
    gate = 1e-5 if yard <= 5e-6 else 2.0 * yard
    print(f"{kind}: plain windowed 6-step DDIM host vs fused {yard:.2e}; windowed repaint host vs fused (10 calls) {err:.2e}, regenerated "
          f"region {err_new:.2e} (gate {gate:.2e}); another seed differs by {rel_l2(other[~kp], fused[~kp]):.2e}")
    assert rs.n_calls == 10 and len(calls) == 10 * 3 and torch.isfinite(host).all()          # 12 windows, 5 per call: 3 forwards per step
    assert err <= gate and err_new <= gate
    assert torch.equal(host[kp], known.expand(shape)[kp]) and torch.equal(fused[kp], known[kp])
    assert rel_l2(other[~kp], fused[~kp]) > 100 * gate       # the draws matter in the regenerated region: the gate can tell chains apart
