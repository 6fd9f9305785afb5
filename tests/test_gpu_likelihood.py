"""LatentDiffusionInferer.get_likelihood on the GPU (-m gpu): the term kernel against the fp64 restatement of MONAI's get_likelihood
(tests/likelihood_ref.py), gated by the error of the same restatement evaluated in fp32; determinism and batch independence of the
reduction; the device-resident loop against the host-driven loop bit for bit; the model-level loop teacher-forced through the
reference; the inferer's surface, the nearest-resize op and the CLI.

Sizes per sample: 1 element, 1003 (ragged last quad) and 4 * 256 * 1024 + 5 (256 workgroups per sample, every thread wraps, then a tail)."""
import functools
import json
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cfgs
import likelihood_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SIZES = [1, 1003, 4 * 256 * 1024 + 5]
PREDS = ["epsilon", "sample", "v_prediction"]
VARS = ["fixed_small", "fixed_large"]
BIN = 1.0 / 255.0
HI = 27.64                                     # -log(1e-12) = 27.631


def _tab(pred="epsilon", vt="fixed_small"):
    return lr.Tables(**cfgs.SCHED, variance_type=vt, prediction_type=pred)


@functools.lru_cache(maxsize=None)
def _inputs(n, t, pred, B=1):
    """(x0, z, m, x_t) fp32 [B, n] on the CPU: x0 = clamp(0.6 randn, +-1.05) (both saturated branches at about 5 % each), m random for
    the large t and the truth + 0.05 randn for t in {1, 0}; x_t is noised in fp32 here and handed to the op and to the reference alike."""
    g = torch.Generator().manual_seed(1000 + n % 997)
    x0 = torch.clamp(0.6 * torch.randn((B, n), generator=g), -1.05, 1.05)
    z = torch.randn((B, n), generator=g)
    r = torch.randn((B, n), generator=g)
    a = _tab().alphas_cumprod[t]
    sa, sb = a ** 0.5, (1 - a) ** 0.5
    x_t = sa * x0 + sb * z
    if t > 1:
        m = r
    else:
        truth = z if pred == "epsilon" else x0 if pred == "sample" else sa * z - sb * x0
        m = truth + 0.05 * r
    return x0, z, m, x_t


@functools.lru_cache(maxsize=None)
def _ref(n, t, pred, vt, B=1):
    """The fp64 map (with its parts) and the fp32 MONAI-order map of the same inputs, computed once per case."""
    x0, _, m, x_t = _inputs(n, t, pred, B)
    kl64, parts = lr.term_map(_tab(pred, vt), t, x0, x_t, m, BIN, torch.float64, parts=True)
    kl32 = lr.term_map(_tab(pred, vt), t, x0, x_t, m, BIN, torch.float32)
    return kl64, kl32, parts


@functools.lru_cache(maxsize=None)
def _lik(pred, vt):
    from ldm3d.schedulers import DDPMScheduler, DeviceLikelihood
    return DeviceLikelihood(DDPMScheduler(**cfgs.SCHED, variance_type=vt, prediction_type=pred), seed=11, bin_width=BIN)


def _op(dev, n, t, pred, vt, B=1, rows=None):
    """The host-driven term op on the case's inputs (or on the batch rows ``rows`` of them) -> (map, per-sample mean, total) on the CPU."""
    x0, _, m, x_t = (v.to(dev) if rows is None else v[rows].contiguous().to(dev) for v in _inputs(n, t, pred, B))
    lik = _lik(pred, vt)
    kmap, term = torch.empty_like(x0), torch.empty((x0.shape[0],), device=dev)
    total = torch.full((x0.shape[0],), 0.5, device=dev)
    lik.term(x0, x_t, m, lik.timesteps.index(t), total, kl_map=kmap, term_out=term)
    return kmap.cpu(), term.cpu(), total.cpu()


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("vt", VARS)
@pytest.mark.parametrize("pred", PREDS)
def test_term_above_t0_matches_fp64(cuda, pred, vt, n):
    """t in {999, 500, 37, 1}: the map's rel-L2 and the per-sample mean's relative error against fp64 are at most 2 x the same error of
    the fp32 MONAI-order restatement on the same inputs + 1e-6 (the scheduler gate as a floor; 2 x: an FMA evaluation reorders roundings
    of the same magnitude).  The kernel evaluates c0 (x0 - x0_hat), without MONAI's cancellation of the two means, and sits far below."""
    for t in (999, 500, 37, 1):
        kl64, kl32, _ = _ref(n, t, pred, vt)
        kmap, term, total = _op(cuda, n, t, pred, vt)
        mean64 = kl64.mean(dim=1)
        e_map, y_map = _rel(kmap, kl64), _rel(kl32, kl64)
        e_mean = float(((term.double() - mean64).abs() / mean64.clamp_min(1e-300)).max())
        y_mean = float(((kl32.mean(dim=1).double() - mean64).abs() / mean64.clamp_min(1e-300)).max())
        print(f"likelihood term {pred} {vt} n={n} t={t}: map rel-L2 {e_map:.3e} (fp32 restatement {y_map:.3e}), "
              f"mean rel {e_mean:.3e} (fp32 restatement {y_mean:.3e})")
        assert torch.isfinite(kmap).all() and float(kmap.min()) >= 0.0
        assert e_map <= 2.0 * y_map + 1e-6, (t, e_map, y_map)
        assert e_mean <= 2.0 * y_mean + 1e-6, (t, e_mean, y_mean)
        assert torch.equal(total, term + 0.5)                     # total[b] += the mean, in fp32


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pred", PREDS)
def test_decoder_term_fixed_large_matches_fp64(cuda, pred, n):
    """t = 0, fixed_large: per element where the reference probability exp(-kl64) >= 1e-3 (below it fp32 loses 1 - cdf and P - M in the
    tails, as MONAI's fp32 does; at most 5 % of the elements), |kl - kl64| <= 2 x the fp32 restatement's max abs error on those elements;
    elsewhere finite in [0, 27.64]."""
    kl64, kl32, _ = _ref(n, 0, pred, "fixed_large")
    kmap, term, _ = _op(cuda, n, 0, pred, "fixed_large")
    keep = torch.exp(-kl64) >= 1e-3
    share = 1.0 - float(keep.double().mean())
    err = float((kmap.double() - kl64)[keep].abs().max()) if keep.any() else 0.0
    yard = float((kl32.double() - kl64)[keep].abs().max()) if keep.any() else 0.0
    print(f"likelihood decoder term {pred} fixed_large n={n}: excluded {100 * share:.2f} %, max abs err {err:.3e} (fp32 restatement {yard:.3e})")
    assert share <= 0.05, share
    assert torch.isfinite(kmap).all() and float(kmap.min()) >= 0.0 and float(kmap.max()) <= HI
    assert err <= 2.0 * yard, (err, yard)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pred", PREDS)
def test_decoder_term_fixed_small_is_the_step_function(cuda, pred, n):
    """t = 0, fixed_small (var = 1e-20): the map is 0 or -log(1e-12).  Elements whose fp64 cx lies >= 1e-5 from both bin edges agree with
    the reference to 1e-3; at most 1 % are closer (there the side of the edge is decided by fp32 rounding)."""
    kl64, kl32, parts = _ref(n, 0, pred, "fixed_small")
    kmap, _, _ = _op(cuda, n, 0, pred, "fixed_small")
    cx = parts["cx"]
    keep = ((cx - BIN / 2).abs() >= 1e-5) & ((cx + BIN / 2).abs() >= 1e-5)
    share = 1.0 - float(keep.double().mean())
    err = float((kmap.double() - kl64)[keep].abs().max()) if keep.any() else 0.0
    yard = float((kl32.double() - kl64)[keep].abs().max()) if keep.any() else 0.0
    print(f"likelihood decoder term {pred} fixed_small n={n}: excluded {100 * share:.2f} %, max abs err {err:.3e} (fp32 restatement {yard:.3e}), "
          f"{int((kmap > 1).sum())} of {kmap.numel()} outside their bin")
    assert share <= 0.01, share
    assert torch.isfinite(kmap).all() and float(kmap.min()) >= 0.0 and float(kmap.max()) <= HI
    assert err <= 1e-3, err


@pytest.mark.parametrize("n", [1003, 40007])
@pytest.mark.parametrize("t,vt", [(500, "fixed_small"), (0, "fixed_large")])
def test_reduction_is_deterministic_and_batch_independent(cuda, t, vt, n):
    """Two runs of one call give the same bits; slot b of a B = 3 call equals the B = 1 call on that sample, map and mean (n = 40007: ten
    workgroups per sample)."""
    a, b = _op(cuda, n, t, "epsilon", vt, B=3), _op(cuda, n, t, "epsilon", vt, B=3)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    for s in range(3):
        one = _op(cuda, n, t, "epsilon", vt, B=3, rows=slice(s, s + 1))
        assert torch.equal(one[0][0], a[0][s]) and torch.equal(one[1][0], a[1][s]), s


@pytest.mark.parametrize("n", [1, 1003, 40008])
def test_philox_noise_and_noising(cuda, n):
    """z is a function of (seed, per_sample, sample, element), not of B; the reset's x_t is row 0's host-driven noising of that z, and
    the noising rounds both products, then the sum."""
    from ldm3d.schedulers import DDPMScheduler, DeviceLikelihood
    lik = _lik("epsilon", "fixed_small")
    z3, z2 = lik.noise((3, n), cuda), lik.noise((2, n), cuda)
    assert torch.equal(z3[:2], z2) and torch.equal(z3, lik.noise((3, n), cuda))
    assert n == 1 or not torch.equal(z3[0], z3[1])
    other = DeviceLikelihood(DDPMScheduler(**cfgs.SCHED), seed=12, bin_width=BIN)
    assert not torch.equal(other.noise((3, n), cuda), z3)
    if n > 1000:
        assert abs(float(z3.mean())) < 0.05 and abs(float(z3.var()) - 1.0) < 0.05
    x0 = _inputs(n, 500, "epsilon", 3)[0].to(cuda)
    x_t, tbuf, total = torch.empty_like(x0), torch.empty((3,), device=cuda), torch.ones((3,), device=cuda)
    lik.reset(x0, x_t, tbuf, total)
    assert torch.equal(x_t, lik.noisy(x0, z3, 0)) and tbuf.tolist() == [999.0] * 3 and total.tolist() == [0.0] * 3
    k = lik.timesteps.index(500)
    sa, sb = (torch.tensor(lik.rows[k][j], dtype=torch.float32) for j in (0, 1))
    assert torch.equal(lik.noisy(x0, z3, k).cpu(), sa * x0.cpu() + sb * z3.cpu())


# ---- model level -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _unet(cond, precision):
    from ldm3d.networks import DiffusionModelUNet
    from oracle import unet as ou
    cfg = cfgs.UNET_TINY_COND if cond else cfgs.UNET_TINY
    m = DiffusionModelUNet(**cfg)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfg), 5))
    m = m.to(torch.device("cuda:0")).eval()
    m.set_precision(precision)
    return m


def _latents(B, cond, dev):
    g = torch.Generator().manual_seed(77)
    x0 = torch.clamp(0.6 * torch.randn((B, 4, 8, 8, 8), generator=g), -1.05, 1.05).to(dev)
    c = torch.randn((B, 4, 8, 8, 8), generator=g).to(dev) if cond else None
    return x0, c


def _sched(pred, vt):
    from ldm3d.schedulers import DDPMScheduler
    sch = DDPMScheduler(**cfgs.SCHED, variance_type=vt, prediction_type=pred)
    sch.set_timesteps(5)
    assert sch.timesteps.tolist() == [800, 600, 400, 200, 0]
    return sch


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("cond,pred,vt", [(False, "epsilon", "fixed_small"), (True, "v_prediction", "fixed_large")], ids=["uncond", "cond"])
def test_device_loop_equals_host_driven_loop(cuda, cond, pred, vt, B, precision, graph):
    """get_likelihood(fused_seed=s) == get_likelihood(noise=DeviceLikelihood(s).noise(...)): total, the per-timestep terms and every map,
    bit for bit, with graph replay on and off; another seed gives another number."""
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.schedulers import DeviceLikelihood
    unet = _unet(cond, precision)
    unet.enable_graph_replay(graph)
    try:
        sch = _sched(pred, vt)
        inf = LatentDiffusionInferer(sch)
        x0, c = _latents(B, cond, cuda)
        kw = dict(conditioning=c, mode="concat") if cond else {}
        common = dict(save_intermediates=True, return_terms=True, verbose=False, **kw)
        total_d, maps_d, terms_d = inf.get_likelihood(x0, None, unet, fused_seed=5, **common)
        z = DeviceLikelihood(sch, seed=5).noise(x0.shape, cuda)
        total_h, maps_h, terms_h = inf.get_likelihood(x0, None, unet, noise=z, **common)
        assert torch.isfinite(total_d).all() and total_d.shape == (B,) and terms_d.shape == (5, B) and len(maps_d) == len(maps_h) == 5
        assert torch.equal(terms_d, terms_h), (terms_d, terms_h)
        assert torch.equal(total_d, total_h)
        assert all(torch.equal(a, b) for a, b in zip(maps_d, maps_h))
        acc = torch.zeros_like(total_d)
        for k in range(5):
            acc += terms_d[k]
        assert torch.equal(acc, total_d)                           # total = the fp32 running sum of the terms
        again = inf.get_likelihood(x0, None, unet, fused_seed=5, verbose=False, **kw)
        assert torch.equal(again, total_d)
        assert not torch.equal(inf.get_likelihood(x0, None, unet, fused_seed=6, verbose=False, **kw), total_d)
    finally:
        unet.enable_graph_replay(False)


def test_graph_replay_key_holds_the_likelihood_pointers(cuda):
    """A recorded likelihood step bakes kl_map, terms and total in by value, so they are part of the replay key: with graph replay on,
    the loop with kl_map=None, with a kl_map tensor and with a second terms tensor each equals the eager loop bit for bit and writes
    the tensors passed on THAT call; a poisoned tensor of an earlier call stays poisoned."""
    from ldm3d.schedulers import DDPMScheduler, DeviceLikelihood
    unet = _unet(False, "bf16")
    sch = DDPMScheduler(**cfgs.SCHED)
    sch.set_timesteps(4)
    lik = DeviceLikelihood(sch, seed=9)
    n, poison = lik.n_steps, -7.0
    x0, _ = _latents(2, False, cuda)
    x_t, tbuf, total = torch.empty_like(x0), torch.empty((2,), device=cuda), torch.empty((2,), device=cuda)

    def loop(kl_map, terms):
        lik.reset(x0, x_t, tbuf, total)
        for _ in range(n):
            unet.likelihood_step(x0, x_t, tbuf, lik, total, kl_map=kl_map, terms=terms)
        return total.clone()
    want_terms, want_map = torch.zeros((n, 2), device=cuda), torch.empty_like(x0)
    want_total = loop(want_map, want_terms)
    assert torch.isfinite(want_total).all() and torch.isfinite(want_map).all() and bool((want_terms != 0).all())
    terms1, terms2, kmap = (torch.full_like(want_terms, poison), torch.full_like(want_terms, poison), torch.full_like(x0, poison))
    unet.enable_graph_replay(True)
    try:
        # 1. no map: every step of a loop has the same key, so one loop sees, captures and replays it
        assert torch.equal(loop(None, terms1), want_total) and torch.equal(terms1, want_terms)
        assert bool((kmap == poison).all())
        # 2. a map: another key, or the replay of 1. would leave the map unwritten
        terms1.fill_(poison)
        assert torch.equal(loop(kmap, terms1), want_total) and torch.equal(terms1, want_terms) and torch.equal(kmap, want_map)
        # 3. a second terms tensor: another key, or the replay of 2. would write the first one
        terms1.fill_(poison), kmap.fill_(poison)
        assert torch.equal(loop(kmap, terms2), want_total) and torch.equal(terms2, want_terms) and torch.equal(kmap, want_map)
        assert bool((terms1 == poison).all())
        # 1. again, now replaying from the first step on: the map of 2. and 3. is not touched
        terms2.fill_(poison), kmap.fill_(poison)
        assert torch.equal(loop(None, terms1), want_total) and torch.equal(terms1, want_terms)
        assert bool((kmap == poison).all()) and bool((terms2 == poison).all())
    finally:
        unet.enable_graph_replay(False)


@pytest.mark.parametrize("pred,vt", [("epsilon", "fixed_large"), ("v_prediction", "fixed_small"), ("sample", "fixed_large")])
def test_model_level_loop_teacher_forced(cuda, pred, vt):
    """The host-driven loop with every step's model output captured and fed to the fp64 reference: each t > 0 term within gate 1 of the
    reference's, the t = 0 map within the per-element gates (2 / 3) and its mean within what those allow, the total within their sum."""
    from ldm3d.schedulers import DeviceLikelihood
    unet = _unet(False, "bf16")
    sch = _sched(pred, vt)
    tab = _tab(pred, vt)
    x0, _ = _latents(2, False, cuda)
    lik = DeviceLikelihood(sch, seed=3, bin_width=BIN)
    z = lik.noise(x0.shape, cuda)
    total, tbuf = torch.zeros((2,), device=cuda), torch.empty((2,), device=cuda)
    terms, kmap = torch.zeros((5, 2), device=cuda), torch.empty_like(x0)
    want_total, slack_total = torch.zeros((2,), dtype=torch.float64), torch.zeros((2,), dtype=torch.float64)
    for k, t in enumerate(lik.timesteps):
        x_t = lik.noisy(x0, z, k)
        tbuf.fill_(float(t))
        with torch.no_grad():
            m = unet(x=x_t, timesteps=tbuf).clone()
        lik.term(x0, x_t, m, k, total, kl_map=kmap, term_out=terms[k])
        args = (x0.cpu().reshape(2, -1), x_t.cpu().reshape(2, -1), m.cpu().reshape(2, -1), BIN)
        kl64, parts = lr.term_map(tab, t, *args, torch.float64, parts=True)
        kl32 = lr.term_map(tab, t, *args, torch.float32)
        got, got_mean, mean64 = kmap.cpu().reshape(2, -1).double(), terms[k].cpu().double(), kl64.mean(dim=1)
        if t > 0:
            y_mean = (kl32.mean(dim=1).double() - mean64).abs() / mean64
            slack = (2.0 * y_mean + 1e-6) * mean64
            assert _rel(got, kl64) <= 2.0 * _rel(kl32, kl64) + 1e-6, (t, _rel(got, kl64), _rel(kl32, kl64))
        else:
            # a random model's x0_hat is far from x0, so most elements sit in the tails: the share limits of the op tests' inputs do
            # not apply here, the per-element gates on the kept elements do
            if vt == "fixed_large":
                keep = torch.exp(-kl64) >= 1e-3
                bound = 2.0 * float((kl32.double() - kl64)[keep].abs().max()) if keep.any() else 0.0
            else:
                cx = parts["cx"]
                keep = ((cx - BIN / 2).abs() >= 1e-5) & ((cx + BIN / 2).abs() >= 1e-5)
                bound = 1e-3
            print(f"teacher-forced {pred} {vt} t=0: {int(keep.sum())} of {keep.numel()} elements kept, per-element bound {bound:.3e}")
            assert float(got.min()) >= 0.0 and float(got.max()) <= HI
            assert not keep.any() or float((got - kl64)[keep].abs().max()) <= bound
            # the mean: kept elements within their bound, an excluded one anywhere in [0, 27.64]
            slack = (keep.double() * bound + (~keep).double() * HI).mean(dim=1) + 1e-6 * mean64
        print(f"teacher-forced {pred} {vt} t={t}: term {got_mean.tolist()} reference {mean64.tolist()} allowed {slack.tolist()}")
        assert bool(((got_mean - mean64).abs() <= slack).all()), (t, got_mean, mean64, slack)
        want_total += mean64
        slack_total += slack
    assert bool(((total.cpu().double() - want_total).abs() <= slack_total + 1e-6 * want_total).all()), (total, want_total, slack_total)


def test_inferer_surface(cuda):
    """MONAI's four call forms (return types and shapes), resampled maps of the input's spatial shape, autoencoder_model=None, and the
    NotImplementedErrors."""
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.networks import AutoencoderKL, DiffusionModelUNet
    from ldm3d.schedulers import DDIMScheduler, PNDMScheduler, RFlowScheduler
    from oracle import autoencoder as oa
    from oracle import unet as ou
    vae = AutoencoderKL(**cfgs.VAE_TINY)
    vae.load_state_dict(ou.init_state_dict(oa.ae_param_shapes(cfgs.VAE_TINY), 2))
    vae = vae.to(cuda).eval()
    ucfg = dict(cfgs.UNET_TINY, in_channels=8, out_channels=8)
    unet = DiffusionModelUNet(**ucfg)
    unet.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(ucfg), 6))
    unet = unet.to(cuda).eval()
    sch = _sched("epsilon", "fixed_large")
    inf = LatentDiffusionInferer(sch, scale_factor=0.9)
    img = torch.rand((2, 2, 32, 32, 32), generator=torch.Generator().manual_seed(4)).to(cuda)
    z = torch.randn((2, 8, 8, 8, 8), generator=torch.Generator().manual_seed(5)).to(cuda)

    def score(**kw):
        torch.manual_seed(123)                                     # encode_stage_2_inputs draws its eps with torch.randn: the same latent every call
        return inf.get_likelihood(img, vae, unet, verbose=False, noise=z, **kw)

    total = score()
    assert torch.is_tensor(total) and total.shape == (2,) and total.is_cuda and torch.isfinite(total).all() and float(total.min()) > 0
    total2, maps = score(save_intermediates=True)
    assert torch.equal(total2, total) and len(maps) == 5 and all(m.shape == (2, 8, 8, 8, 8) and not m.is_cuda for m in maps)
    mean_of_maps = sum(m.double().reshape(2, -1).mean(dim=1) for m in maps)
    assert torch.allclose(mean_of_maps, total.cpu().double(), rtol=1e-5)
    total3, big = score(save_intermediates=True, resample_latent_likelihoods=True, resample_interpolation_mode="nearest")
    assert torch.equal(total3, total) and all(m.shape == (2, 8, 32, 32, 32) for m in big)
    assert all(torch.equal(b, F.interpolate(m, size=(32, 32, 32), mode="nearest")) for b, m in zip(big, maps))
    assert inf.get_likelihood(img, vae, unet).shape == (2,)        # the defaults: torch.randn_like noise, verbose
    # mode="concat" conditioning on the latent itself (autoencoder_model=None)
    cu = _unet(True, "bf16")
    x0, c = _latents(2, True, cuda)
    tc = LatentDiffusionInferer(sch).get_likelihood(x0, None, cu, conditioning=c, mode="concat", verbose=False, fused_seed=1)
    assert tc.shape == (2,) and torch.isfinite(tc).all()
    with pytest.raises(NotImplementedError):
        LatentDiffusionInferer(sch).get_likelihood(x0, None, cu, conditioning=c, mode="crossattn", verbose=False)
    for other in (DDIMScheduler(**cfgs.SCHED), PNDMScheduler(**cfgs.SCHED), RFlowScheduler()):
        with pytest.raises(NotImplementedError):
            inf.get_likelihood(img, vae, unet, scheduler=other, verbose=False)
    with pytest.raises(NotImplementedError):
        inf.get_likelihood(img, vae, unet, verbose=False, resample_latent_likelihoods=True, resample_interpolation_mode="trilinear")
    with pytest.raises(ValueError):
        inf.get_likelihood(img, vae, unet, verbose=False, resample_latent_likelihoods=True, resample_interpolation_mode="bicubic")


def test_c_level_refusals_launch_nothing(cuda):
    import ctypes as C
    from ldm3d import _lib
    from ldm3d.schedulers import LIK_ROW, DeviceLikelihood
    L = _lib.lib()
    sch = _sched("epsilon", "fixed_small")
    rows = torch.tensor(sch.likelihood_rows(), dtype=torch.float32)
    h = C.c_void_p()
    assert L.ldm_likelihood_create(rows.data_ptr(), 5, 3, 1, 0, BIN, C.byref(h)) == -1 and not h.value          # unknown pred
    assert L.ldm_likelihood_create(rows.data_ptr(), 5, 0, 1, 0, 0.0, C.byref(h)) == -1 and not h.value          # bin_width <= 0
    assert L.ldm_likelihood_create(None, 5, 0, 1, 0, BIN, C.byref(h)) == -1 and L.ldm_likelihood_create(rows.data_ptr(), 0, 0, 1, 0, BIN, C.byref(h)) == -1
    lik = DeviceLikelihood(sch, seed=1, bin_width=BIN)
    x0, _ = _latents(2, False, cuda)
    x_t, m = torch.randn_like(x0), torch.randn_like(x0)
    total, kmap = torch.full((2,), 7.0, device=cuda), torch.full_like(x0, -3.0)
    ws = lik.scratch(x0)
    row = (C.c_float * LIK_ROW)(*lik.rows[0])
    s = _lib.current_stream()
    per = x0[0].numel()
    term = lambda a, b, c, r, pred, bw, B: L.ldm_likelihood_term(a, b, c, r, pred, 1, bw, kmap.data_ptr(), None, total.data_ptr(), B, per,
                                                                 ws.data_ptr(), ws.numel() * 8, s)
    p = (x0.data_ptr(), x_t.data_ptr(), m.data_ptr())
    assert term(None, p[1], p[2], row, 0, BIN, 2) == -1 and term(p[0], None, p[2], row, 0, BIN, 2) == -1 and term(p[0], p[1], None, row, 0, BIN, 2) == -1
    assert term(*p, None, 0, BIN, 2) == -1 and term(*p, row, 0, BIN, 0) == -1 and term(*p, row, 7, BIN, 2) == -1 and term(*p, row, 0, -1.0, 2) == -1
    assert L.ldm_likelihood_term(*p, row, 0, 1, BIN, None, None, total.data_ptr(), 2, per, ws.data_ptr(), 8, s) == -5      # scratch too small
    assert L.ldm_likelihood_noisy(None, x_t.data_ptr(), row, x_t.data_ptr(), 2, per, s) == -1
    assert L.ldm_likelihood_noise(lik._h, None, 2, per, s) == -1 and L.ldm_likelihood_noise(lik._h, x_t.data_ptr(), 0, per, s) == -1
    assert L.ldm_op_resize_nearest(None, kmap.data_ptr(), 1, 1, 2, 2, 2, 4, 4, 4, s) == -1
    assert L.ldm_op_resize_nearest(x0.data_ptr(), kmap.data_ptr(), 1, 1, 2, 2, 2, 0, 4, 4, s) == -1
    torch.cuda.synchronize()
    assert total.tolist() == [7.0, 7.0] and bool((kmap == -3.0).all())
    # a step before the first reset and a step past the last row
    unet = _unet(False, "bf16")
    tbuf = torch.empty((2,), device=cuda)
    with pytest.raises(_lib.LdmError, match="past the last row"):
        unet.likelihood_step(x0, x_t, tbuf, lik, total, kl_map=kmap)
    lik.reset(x0, x_t, tbuf, total)
    for _ in range(5):
        unet.likelihood_step(x0, x_t, tbuf, lik, total)
    done, xt_done = total.clone(), x_t.clone()
    with pytest.raises(_lib.LdmError, match="past the last row"):
        unet.likelihood_step(x0, x_t, tbuf, lik, total, kl_map=kmap)
    torch.cuda.synchronize()
    assert torch.equal(total, done) and torch.equal(x_t, xt_done) and bool((kmap == -3.0).all()) and tbuf.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("src,dst", [((2, 3, 5), (8, 12, 20)), ((3, 4, 5), (7, 9, 11)), ((2, 3, 4), (8, 12, 16))])
def test_resize_nearest_matches_torch(cuda, src, dst):
    from ldm3d.inferer import resize_nearest
    x = torch.randn((2, 3) + src, generator=torch.Generator().manual_seed(9))
    assert torch.equal(resize_nearest(x.to(cuda), dst).cpu(), F.interpolate(x, size=dst, mode="nearest"))


def test_inference_cli_likelihood(tmp_path):
    from ldm3d.data import write_synthetic_pairs
    pair = write_synthetic_pairs(str(tmp_path / "pairs"), 1, (100, 104, 118))[0]
    env = {"npz_dir": str(tmp_path / "pairs"), "model_dir": str(tmp_path / "ckpt"), "output_dir": str(tmp_path / "out"),
           "tfevent_path": str(tmp_path / "tfevent"), "resume_ckpt": False, "seed": 7}
    env_file = str(tmp_path / "environment.json")
    with open(env_file, "w") as fh:
        json.dump(env, fh)
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-e", env_file, "-c", os.path.join(ROOT, "config", "config_synthetic_train.json"),
           "--random-init", "--likelihood", "--steps", "4", "--condition", pair, "--likelihood-map", "-n", "2"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    recs = [json.loads(l) for l in open(tmp_path / "out" / "likelihood.jsonl")]
    assert len(recs) == 2 and [rec["seed"] for rec in recs] == [7, 8]          # the environment file's seed + the draw's index
    for rec in recs:
        assert math.isfinite(rec["nll_nats_per_dim"]) and rec["nll_nats_per_dim"] > 0 and math.isfinite(rec["t0_term"])
        assert rec["bits_per_dim"] == rec["nll_nats_per_dim"] / math.log(2.0)
        assert rec["timesteps"] == 4 and rec["latent_shape"][1:] == [24, 24, 24]
        raw = open(tmp_path / "out" / rec["map"], "rb").read()
        assert struct.unpack_from("<8h", raw, 40)[:5] == (4, 96, 96, 96, 1)              # the crop's shape (+ the trailing axis of every volume written)
        vol = np.frombuffer(raw, dtype="<f4", offset=352)
        assert vol.size == 96 ** 3 and np.isfinite(vol).all() and vol.min() >= 0.0 and vol.max() > 0.0
    assert recs[0]["nll_nats_per_dim"] != recs[1]["nll_nats_per_dim"]
