"""RFlowScheduler (rectified flow) on the GPU (-m gpu): the host-driven step against the fp64 restatement (tests/rflow_ref.py), the device
sampler against the host-driven step bit for bit, the closed-form straight path, the noising / target kernel, the one-launch timestep
draw, the cached latent batch, graph replay, sliding windows, the trainer, argument errors and the two command lines.

Sizes: 1 element, 1003 (ragged last quad) and 4 * 256 * 1024 + 5 (every thread of the 1024-block grid wraps once, then a tail)."""
import ctypes as C
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cfgs
from rflow_ref import RFlowRef, timestep_uniform, ulp32
from util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
BAD_ARG = -1                                                            # LDM_ERR_BAD_ARG, include/ldm3d.h
SIZES = [1, 1003, 4 * 256 * 1024 + 5]
T = 1000
NUMEL = 24 * 20 * 28                                                    # the volume size the transformed schedules see
SCHEDULES = {"discrete": dict(), "transformed": dict(use_discrete_timesteps=False, use_timestep_transform=True, transform_scale=1.3)}


def _pair(schedule, n_steps):
    from ldm3d.schedulers import RFlowScheduler
    sch, ref = RFlowScheduler(**SCHEDULES[schedule]), RFlowRef(**SCHEDULES[schedule])
    sch.set_timesteps(n_steps, input_img_size_numel=NUMEL)
    ref.set_timesteps(n_steps, input_img_size_numel=NUMEL)
    assert sch.timesteps.double().tolist() == ref.timesteps.tolist()
    return sch, ref


def _next(ts, k):
    return ts[k + 1] if k + 1 < len(ts) else 0


@functools.lru_cache(maxsize=None)
def _chain(schedule, n):
    """One N = 10 chain with random model outputs, computed once per case and shared: the outputs, the free-running host-driven chain
    (prev and x0_hat of every step), the fp64 reference chain, and the per-step errors of the step fed from the reference's state."""
    dev = torch.device("cuda:0")
    sch, ref = _pair(schedule, 10)
    g = torch.Generator(device=dev).manual_seed(2000 + n % 997)
    x_init = torch.randn((n,), device=dev, generator=g)
    ts = sch.timesteps.tolist()
    ms, xs, x0s, err_prev, err_x0 = [], [], [], [], []
    x, xr = x_init, x_init.double().cpu()
    for k, t in enumerate(ts):
        m = torch.randn((n,), device=dev, generator=g)
        ms.append(m)
        got_prev, got_x0 = sch.step(m, t, xr.float().to(dev), next_timestep=_next(ts, k))
        x, x0 = sch.step(m, t, x, next_timestep=_next(ts, k))
        xs.append(x)
        x0s.append(x0)
        xr_next, x0r = ref.step(m.double().cpu(), t, xr, next_timestep=_next(ts, k))
        err_prev.append(rel_l2(got_prev, xr_next))
        err_x0.append(rel_l2(got_x0, x0r))
        xr = xr_next
    return dict(sch=sch, ts=ts, x_init=x_init, ms=ms, xs=xs, x0s=x0s, ref_end=xr, err_prev=err_prev, err_x0=err_x0)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_host_driven_step_matches_fp64(cuda, schedule, n):
    """Every step, from the reference's state: prev and x0_hat at rel-L2 <= 1e-6 (the project's scheduler gate).  The end-of-chain error of
    the chain that runs on its own fp32 state is reported, not gated."""
    c = _chain(schedule, n)
    end = rel_l2(c["xs"][-1], c["ref_end"])
    print(f"rflow {schedule} n={n}: max per-step rel-L2 prev {max(c['err_prev']):.3e}, x0_hat {max(c['err_x0']):.3e}, end of chain {end:.3e}")
    assert len(c["err_prev"]) == 10
    assert max(c["err_prev"]) <= 1e-6 and max(c["err_x0"]) <= 1e-6, (c["err_prev"], c["err_x0"])
    assert torch.isfinite(c["xs"][-1]).all()
    if n > 1:                                                      # without next_timestep: dt = 1 / num_inference_steps
        sch, m, x = c["sch"], c["ms"][0], c["x_init"]
        got, _ = sch.step(m, c["ts"][3], x)
        assert rel_l2(got, x.double().cpu() + 0.1 * m.double().cpu()) <= 1e-6


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_fused_sampler_equals_host_driven_bitwise(cuda, schedule, n):
    c = _chain(schedule, n)
    sch, ts = c["sch"], c["ts"]
    smp = sch.device_sampler()
    assert smp.n_steps == len(ts) and smp.kind == 3 and smp.state_numel(n) == 0
    x = c["x_init"].clone()
    x0 = torch.full_like(x, float("nan"))
    tbuf = torch.full((2,), -1.0, device=cuda)
    smp.reset(tbuf)
    assert tbuf.tolist() == [float(ts[0])] * 2
    for k, m in enumerate(c["ms"]):
        keep = m.clone()
        smp.step(m, x, tbuf, x0_out=x0)
        assert torch.equal(x, c["xs"][k]), (k, rel_l2(x, c["xs"][k]))
        assert torch.equal(x0, c["x0s"][k]), (k, rel_l2(x0, c["x0s"][k]))
        assert tbuf.tolist() == [float(ts[min(k + 1, len(ts) - 1)])] * 2, k
        assert torch.equal(m, keep)
    x0.fill_(7.0)
    smp.step(c["ms"][0], x, tbuf, x0_out=x0)                      # beyond the end: nothing moves
    assert torch.equal(x, c["xs"][-1]) and tbuf.tolist() == [float(ts[-1])] * 2 and bool((x0 == 7.0).all())
    smp.reset(tbuf)                                                # a rewound chain reproduces the first, without x0_out too
    x.copy_(c["x_init"])
    for m in c["ms"]:
        smp.step(m, x, tbuf)
    assert torch.equal(x, c["xs"][-1])


@pytest.mark.parametrize("n_steps", [1, 7, 30])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_closed_form_straight_path(cuda, schedule, n_steps):
    """The model output is the constant v = x* - noise and the chain starts at x = noise with t_0 = T: the dt sum to 1, so the chain ends
    at x*.  Bound per element, nothing measured: each of the N steps is one fused multiply-add whose result lies between noise and x*
    (|.| <= |noise| + |v|) and is rounded once (2^-24 relative), and the N fp32 dt carry at most 2^-24 of |v| in total: together below
    N * 2^-23 * (|noise| + |v|).  v and noise are the fp32 data; x* = noise + v is formed in fp64, where that sum is exact."""
    n = 1003
    sch, ref = _pair(schedule, n_steps)
    assert ref.timesteps[0].item() == float(T)
    g = torch.Generator().manual_seed(17)
    noise, v = torch.randn((n,), generator=g), torch.randn((n,), generator=g)
    x_star = noise.double() + v.double()
    x = noise.clone().to(cuda)
    vm = v.to(cuda)
    smp = sch.device_sampler()
    tbuf = torch.empty((1,), device=cuda)
    smp.reset(tbuf)
    for _ in range(n_steps):
        smp.step(vm, x, tbuf)
    err = (x.double().cpu() - x_star).abs()
    bound = n_steps * 2.0 ** -23 * (noise.double().abs() + v.double().abs())
    print(f"rflow closed form {schedule} N={n_steps}: max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())


def _noise_target(x0, noise, a, b, noisy=True):
    from ldm3d import _lib
    B = x0.shape[0]
    ny = torch.full_like(x0, 7.0) if noisy else None
    tg = torch.full_like(x0, 7.0)
    rc = _lib.lib().ldm_rflow_noise_target(_lib.ptr(x0), _lib.ptr(noise), _lib.ptr(a), _lib.ptr(b), _lib.ptr(ny), _lib.ptr(tg), B,
                                           x0.numel() // B, _lib.current_stream())
    return rc, ny, tg


@pytest.mark.parametrize("per_sample", SIZES)
def test_noise_and_target_kernel(cuda, per_sample):
    """B = 3 at t = 0, 500, T.  noisy is bit-equal to torch's fp32 a x0 + b noise (both products rounded, then the sum), which is how
    ldm_add_noise rounds launches of at most 2^20 elements: compared with ldm_add_noise itself at the sizes below that, and through
    RFlowScheduler.add_noise / add_noise_and_target; target is bit-equal to fp32 x0 - noise; both within 1e-6 of fp64."""
    from ldm3d.schedulers import RFlowScheduler
    sch, ref = RFlowScheduler(), RFlowRef()
    g = torch.Generator(device=cuda).manual_seed(per_sample % 991)
    x0 = torch.randn((3, per_sample), device=cuda, generator=g)
    noise = torch.randn((3, per_sample), device=cuda, generator=g)
    ts = torch.tensor([0, 500, T], device=cuda)
    a, b = sch._noising_coefs(ts, cuda)
    assert a.tolist() == [1.0, 0.5, 0.0] and b.tolist() == [0.0, 0.5, 1.0]
    rc, noisy, target = _noise_target(x0, noise, a, b)
    assert rc == 0
    assert torch.equal(noisy, a[:, None] * x0 + b[:, None] * noise)
    assert torch.equal(target, x0 - noise)
    assert torch.equal(noisy[0], x0[0]) and torch.equal(noisy[2], noise[2])      # t = 0: the data; t = T: the noise
    rc, none, t2 = _noise_target(x0, noise, a, b, noisy=False)                   # noisy may be NULL
    assert rc == 0 and none is None and torch.equal(t2, target)
    for name, got, want in (("noisy", noisy, ref.add_noise(x0, noise, ts)), ("target", target, ref.target(x0, noise))):
        err, bound = float((got.double() - want).abs().max()), 1e-6 * float(want.abs().max())
        print(f"per_sample {per_sample} {name}: max abs err {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    n2, t3 = sch.add_noise_and_target(original_samples=x0, noise=noise, timesteps=ts)
    assert torch.equal(n2, noisy) and torch.equal(t3, target)
    if 3 * per_sample <= 1 << 20:
        from ldm3d import _lib
        chain = torch.empty_like(x0)
        _lib.check(_lib.lib().ldm_add_noise(x0.data_ptr(), noise.data_ptr(), a.data_ptr(), b.data_ptr(), chain.data_ptr(), 3, per_sample,
                                            _lib.current_stream()))
        assert torch.equal(noisy, chain) and torch.equal(sch.add_noise(original_samples=x0, noise=noise, timesteps=ts), chain)
    # unaligned rows of a multiple-of-four sample (the scalar path) and aligned ones (the float4 path) agree
    if per_sample == 1003:
        xa, na = x0[:, :1000].contiguous(), noise[:, :1000].contiguous()
        rc, ny, tg = _noise_target(xa, na, a, b)
        assert rc == 0 and torch.equal(ny, noisy[:, :1000]) and torch.equal(tg, target[:, :1000])


def _timesteps(draw=None, idx=None, B=None, method="uniform", loc=0.0, scale=1.0, discrete=False, ratio=0.0, seed=0, step=0, outs=None,
               Tn=T, null=None):
    """One ldm_rflow_timesteps call -> (status, t, one_minus_tau, tau)."""
    from ldm3d import _lib
    from ldm3d.schedulers import SAMPLE_METHODS
    dev = torch.device("cuda:0")
    nb = B if B is not None else (draw.numel() if draw is not None else len(idx))
    if outs is None:
        outs = [torch.empty((max(nb, 1),), device=dev) for _ in range(3)]
    ptrs = [None if null == k else o.data_ptr() for k, o in enumerate(outs)]
    ids = None if idx is None else (C.c_int * max(len(idx), 1))(*idx)
    rc = _lib.lib().ldm_rflow_timesteps(ids, nb, Tn, SAMPLE_METHODS.get(method, method), loc, scale, int(discrete), ratio, _lib.ptr(draw),
                                        seed, step, ptrs[0], ptrs[1], ptrs[2], _lib.current_stream())
    return rc, outs[0], outs[1], outs[2]


def _batched(draws, **kw):
    """ldm_rflow_timesteps over 4096 explicit draws in batches of 64 -> (t, one_minus_tau, tau) [4096]."""
    out = [[], [], []]
    for lo in range(0, draws.numel(), 64):
        rc, t, omt, tau = _timesteps(draw=draws[lo:lo + 64].contiguous(), **kw)
        assert rc == 0
        for o, v in zip(out, (t, omt, tau)):
            o.append(v)
    return tuple(torch.cat(o) for o in out)


def _close_ulps(got, want, ulps=1):
    """|got - want| <= ulps fp32 ulp of want, element-wise."""
    got, want = got.double().cpu(), want.double().cpu()
    spacing = torch.tensor([ulp32(w) for w in want.tolist()], dtype=torch.float64)
    return bool(((got - want).abs() <= ulps * spacing).all())


def test_timesteps_from_explicit_uniform_draws(cuda):
    """4096 draws.  Continuous: t equals torch's fp32 u * T (one correctly rounded multiply either way), tau is within 1 ulp of torch's
    t / T (torch multiplies by the rounded reciprocal), one_minus_tau is exactly the fp32 1 - tau of the kernel's own tau and hence within
    2^-23 of torch's (tau < 1 moves by at most 2^-24 and each subtraction rounds by at most 2^-25).  Discrete: floor(fp32(u T)) exactly."""
    u = torch.rand((4096,), device=cuda, generator=torch.Generator(device=cuda).manual_seed(31))
    t, omt, tau = _batched(u)
    t_ref = u * float(T)
    tau_ref = t_ref / float(T)
    assert torch.equal(t, t_ref)
    assert _close_ulps(tau, tau_ref)
    assert torch.equal(omt, 1.0 - tau)
    assert float((omt.double() - (1.0 - tau_ref).double()).abs().max()) <= 2.0 ** -23
    assert bool((t >= 0).all()) and bool((t < T).all())
    td, omtd, taud = _batched(u, discrete=True)
    assert torch.equal(td, torch.floor(t_ref))
    assert _close_ulps(taud, td / float(T)) and torch.equal(omtd, 1.0 - taud)
    # the transform, on the continuous and on the floored timesteps: 1e-6 relative to fp64
    for discrete in (False, True):
        kw = dict(use_discrete_timesteps=discrete, use_timestep_transform=True, transform_scale=1.3)
        ref = RFlowRef(**kw)
        tt, omtt, taut = _batched(u, discrete=discrete, ratio=ref.ratio(NUMEL))
        want = ref.transform(torch.floor(t_ref.double()) if discrete else t_ref.double(), NUMEL).cpu()
        err = (tt.double().cpu() - want).abs()
        print(f"transform (discrete {discrete}): max rel err {float((err / want.clamp_min(1e-30)).max()):.3e}")
        assert bool((err <= 1e-6 * want).all())
        assert _close_ulps(taut, tt / float(T)) and torch.equal(omtt, 1.0 - taut)


def test_timesteps_from_explicit_normal_draws(cuda):
    """Logit-normal, 4096 draws, loc 0.3, scale 1.7.  Continuous: |t - fp64| <= 4 * 2^-23 * T.  Discrete: floor(fp64) wherever the fp64
    value's fractional part lies in [1e-3, 1 - 1e-3], never off by more than 1 elsewhere; the excluded draws are at most 1 % of all (a cap:
    the band is 0.2 % wide; checked here on the fp64 reference alone)."""
    n = torch.randn((4096,), device=cuda, generator=torch.Generator(device=cuda).manual_seed(47))
    kw = dict(sample_method="logit-normal", loc=0.3, scale=1.7)
    cont = RFlowRef(use_discrete_timesteps=False, **kw).sample_timesteps(n.cpu())
    frac = cont - torch.floor(cont)
    clear = (frac >= 1e-3) & (frac <= 1 - 1e-3)
    assert float((~clear).float().mean()) <= 0.01
    t, omt, tau = _batched(n, method="logit-normal", loc=0.3, scale=1.7)
    err = float((t.double().cpu() - cont).abs().max())
    print(f"logit-normal continuous: max |dt| {err:.3e} (bound {4 * 2.0 ** -23 * T:.3e})")
    assert err <= 4 * 2.0 ** -23 * T
    assert _close_ulps(tau, t / float(T)) and torch.equal(omt, 1.0 - tau)
    td, omtd, taud = _batched(n, method="logit-normal", loc=0.3, scale=1.7, discrete=True)
    want = RFlowRef(use_discrete_timesteps=True, **kw).sample_timesteps(n.cpu())
    got = td.double().cpu()
    assert torch.equal(got[clear], want[clear])
    assert float((got - want).abs().max()) <= 1.0
    assert bool((td >= 0).all()) and bool((td < T).all()) and torch.equal(td, torch.floor(td))
    assert _close_ulps(taud, td / float(T)) and torch.equal(omtd, 1.0 - taud)


def test_device_draws_depend_on_seed_step_and_dataset_index_only(cuda):
    seed, step = 0x123456789ABCDEF, 5
    idx = [5, 9, 200, 0, 63]
    for method in ("uniform", "logit-normal"):
        kw = dict(method=method, seed=seed, step=step)
        rc, t, omt, tau = _timesteps(idx=idx, **kw)
        assert rc == 0 and bool(torch.isfinite(t).all()) and bool((t >= 0).all()) and bool((t < T).all())
        assert _close_ulps(tau, t / float(T)) and torch.equal(omt, 1.0 - tau)
        if method == "uniform":                                    # the documented key layout, restated on the host
            want = [float(np.float32(timestep_uniform(seed, step, i)) * np.float32(T)) for i in idx]
            assert t.tolist() == want
        rc, t2, _, _ = _timesteps(idx=idx[::-1], **kw)               # another slot
        assert rc == 0 and torch.equal(t2, t.flip(0))
        for slot, i in enumerate(idx):                             # a batch of one
            rc, t1, _, _ = _timesteps(idx=[i], **kw)
            assert rc == 0 and float(t1[0]) == float(t[slot])
        big = list(range(64))                                      # the largest batch; idx NULL means the batch slots
        rc, t64, _, _ = _timesteps(idx=big, **kw)
        rc2, tslots, _, _ = _timesteps(B=64, **kw)
        assert rc == 0 and rc2 == 0 and torch.equal(t64, tslots)
        assert float(t64[5]) == float(t[0]) and float(t64[9]) == float(t[1]) and float(t64[63]) == float(t[4])
        assert len(set(t64.tolist())) >= 60                        # different indices: different draws
        for other in (dict(kw, step=6), dict(kw, seed=seed + 1), dict(kw, seed=seed ^ (1 << 40))):
            rc, d, _, _ = _timesteps(idx=big, **other)
            assert rc == 0 and float((d != t64).float().mean()) > 0.9


def _latent_batch_first_draws(seed, step, n_idx):
    """The first element of the three latent-batch streams (e_label, e_image, noise) for dataset indices 0 .. n_idx - 1: [3, n_idx]."""
    from ldm3d import _lib
    dev = torch.device("cuda:0")
    cache = tuple(torch.zeros((n_idx, 4), device=dev) for _ in range(4))
    ones = torch.ones(n_idx, device=dev)
    outs = [torch.empty((n_idx, 4), device=dev) for _ in range(3)]
    draws = torch.empty((3, n_idx, 4), device=dev)
    _lib.check(_lib.lib().ldm_latent_batch(cache[0].data_ptr(), cache[1].data_ptr(), cache[2].data_ptr(), cache[3].data_ptr(), n_idx, 4,
                                           (C.c_int * n_idx)(*range(n_idx)), n_idx, ones.data_ptr(), ones.data_ptr(), 1.0, 0, None, None, None,
                                           seed, step, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), draws.data_ptr(),
                                           _lib.current_stream()))
    return draws[:, :, 0].contiguous()


def test_device_draw_statistics_and_stream_separation(cuda):
    """2^16 draws (1024 steps x 64 indices).  Uniform: u = t / T has mean 1/2 and variance 1/12; the five-sigma bounds of the sample mean
    (sigma = sqrt(1/12 / n)) and of the sample variance (sigma = sqrt((1/80 - 1/144) / n), from the fourth central moment 1/80).
    Logit-normal (loc 0, scale 1): n = logit(t / T) recovered in fp64 is standard normal: |mean| < 5 / sqrt(n), |var - 1| < 5 sqrt(2 / n),
    the bounds tests/test_gpu_latent_batch.py uses.  And the stream is its own: the timestep a latent-batch draw of the same key would
    give is not the timestep drawn."""
    steps, per = 1024, 64
    us, ns = [], []
    for step in range(steps):
        rc, t, _, _ = _timesteps(B=per, seed=2024, step=step)
        rc2, tn, _, _ = _timesteps(B=per, method="logit-normal", seed=2024, step=step)
        assert rc == 0 and rc2 == 0
        us.append(t)
        ns.append(tn)
    n = steps * per
    u = torch.cat(us).double() / T
    mean, var = float(u.mean()), float(u.var(unbiased=False))
    b_mean, b_var = 5 * math.sqrt(1 / 12 / n), 5 * math.sqrt((1 / 80 - 1 / 144) / n)
    print(f"uniform: mean - 1/2 {mean - 0.5:+.5f} (bound {b_mean:.5f}), var - 1/12 {var - 1 / 12:+.6f} (bound {b_var:.6f})")
    assert abs(mean - 0.5) < b_mean and abs(var - 1 / 12) < b_var
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
    tau = torch.cat(ns).double() / T
    assert float(tau.min()) > 0.0 and float(tau.max()) < 1.0
    z = torch.log(tau) - torch.log1p(-tau)
    mean, var = float(z.mean()), float(z.var(unbiased=False))
    print(f"logit-normal: mean {mean:+.5f} (bound {5 / math.sqrt(n):.5f}), var - 1 {var - 1:+.5f} (bound {5 * math.sqrt(2 / n):.5f})")
    assert abs(mean) < 5 / math.sqrt(n) and abs(var - 1) < 5 * math.sqrt(2 / n)
    first = _latent_batch_first_draws(2024, 3, per)                # [3, 64] normals of the key (seed 2024, step 3, idx)
    rc, mine, _, _ = _timesteps(B=per, method="logit-normal", seed=2024, step=3)
    assert rc == 0
    for s in range(3):
        rc, theirs, _, _ = _timesteps(draw=first[s].contiguous(), method="logit-normal")
        assert rc == 0 and float((theirs != mine).float().mean()) > 0.95, s


def _heads(ml, eps):
    """ldm_op_vae_heads on ONE sample: ml [2L, ...] (mu | log_var), eps [L, ...] or None -> (mu, sigma, z = mu + sigma * eps)."""
    from ldm3d import _lib
    Lc = ml.shape[0] // 2
    mu, sg, z = (torch.empty((Lc,) + tuple(ml.shape[1:]), device=ml.device) for _ in range(3))
    _lib.check(_lib.lib().ldm_op_vae_heads(ml.data_ptr(), _lib.ptr(eps), mu.data_ptr(), sg.data_ptr(), z.data_ptr(), 1, Lc, ml[0].numel(),
                                           _lib.current_stream()))
    return mu, sg, z


@pytest.mark.parametrize("scale", [1.0, 0.7311])
def test_latent_cache_batch_equals_the_chain_bit_for_bit(cuda, scale):
    """LatentCache.batch with an RFlowScheduler and explicit draws at the 3 x 3 x 5 x 7 cache shape of tests/test_gpu_latent_batch.py (315
    elements per sample: no multiple of 4) against encode (ldm_op_vae_heads per sample) -> torch's multiply by the scale factor ->
    add_noise_and_target: noisy, the unscaled condition and target = z - noise; with explicit timesteps, with the coefficients of
    sample_timesteps, and with device draws replayed."""
    from ldm3d.latents import LatentCache
    from ldm3d.schedulers import RFlowScheduler
    shape = (3, 3, 5, 7)
    g = torch.Generator(device=cuda).manual_seed(sum(shape))
    ml_l = torch.randn((3, 6) + shape[1:], device=cuda, generator=g) * 1.5
    ml_i = torch.randn((3, 6) + shape[1:], device=cuda, generator=g) * 1.5
    mu_l, sg_l = (torch.stack(t) for t in zip(*[_heads(ml_l[n].contiguous(), None)[:2] for n in range(3)]))
    mu_i, sg_i = (torch.stack(t) for t in zip(*[_heads(ml_i[n].contiguous(), None)[:2] for n in range(3)]))
    e_l, e_i, nz = (torch.randn((3,) + shape, device=cuda, generator=g) for _ in range(3))
    cache = LatentCache(mu_l, sg_l, mu_i, sg_i)
    idx = [2, 0, 2]
    z = torch.stack([_heads(ml_l[n].contiguous(), e_l[b].contiguous())[2] for b, n in enumerate(idx)])
    want_cond = torch.stack([_heads(ml_i[n].contiguous(), e_i[b].contiguous())[2] for b, n in enumerate(idx)])
    if scale != 1.0:
        z = z * scale
    sch = RFlowScheduler(sample_method="logit-normal")
    drawn = sch.sample_timesteps(z, idx=idx, seed=9, step=2)
    assert drawn.shape == (3,) and float(drawn[0]) == float(drawn[2]) != float(drawn[1])       # keyed by the dataset index
    for ts in (torch.tensor([0, T, 417], device=cuda), drawn):
        want_noisy, want_target = sch.add_noise_and_target(original_samples=z, noise=nz, timesteps=ts)
        assert torch.equal(want_target, z - nz)
        noisy, cond, target = cache.batch(idx, sch, ts, scale, eps_label=e_l, eps_image=e_i, noise=nz)
        assert torch.equal(noisy, want_noisy), float((noisy - want_noisy).abs().max())
        assert torch.equal(cond, want_cond) and torch.equal(target, want_target)
    explicit = sch._noising_coefs(drawn.clone(), cuda)             # the same timesteps as a tensor of the caller's: t / T and 1 - t / T
    assert torch.equal(explicit[1], sch._drawn[2]) and torch.equal(explicit[0], sch._drawn[1])
    noisy, cond, target, draws = cache.batch(idx, sch, drawn, scale, seed=77, step=4, return_draws=True)
    n2, c2, t2 = cache.batch(idx, sch, drawn, scale, eps_label=draws[0], eps_image=draws[1], noise=draws[2])
    assert torch.equal(n2, noisy) and torch.equal(c2, cond) and torch.equal(t2, target) and bool(torch.isfinite(noisy).all())


def _unet(cfg, cuda, seed=1):
    from ldm3d.networks import DiffusionModelUNet
    from oracle import unet as ou
    m = DiffusionModelUNet(**cfg)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfg), seed))
    return m.to(cuda).eval()


def _flow6(**kw):
    from ldm3d.schedulers import RFlowScheduler
    sch = RFlowScheduler(**kw)
    sch.set_timesteps(6, input_img_size_numel=NUMEL)
    return sch


def test_graph_replay_equals_eager_and_the_table_equals_the_computed_embedding(cuda):
    """ldm_unet_denoise_step with a flow sampler: eager and replayed chains are bit-equal, finite and away from the start; and the chain
    whose time embedding comes from the table keyed by the sampler's (fractional) timesteps equals the chain that computes it from tbuf
    (UNet forward + ldm_sampler_step) bit for bit, the gate tests/test_gpu_sampler.py holds the table to."""
    m = _unet(cfgs.UNET_TINY, cuda)
    for sch in (_flow6(), _flow6(**SCHEDULES["transformed"])):
        x0 = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=torch.Generator(device=cuda).manual_seed(2))
        x, tbuf = torch.empty_like(x0), torch.empty((1,), device=cuda)
        ts = sch.timesteps.tolist()

        def chain(smp, fused=True):
            x.copy_(x0)
            smp.reset(tbuf)
            for k in range(len(ts)):
                assert tbuf.tolist() == [float(ts[k])]
                if fused:
                    m.denoise_step(x, tbuf, smp)
                else:
                    smp.step(m(x=x, timesteps=tbuf), x, tbuf)
            return x.clone()
        with torch.no_grad():
            m.enable_graph_replay(False)
            eager = chain(sch.device_sampler())
            assert torch.isfinite(eager).all() and not torch.equal(eager, x0)
            unfused = chain(sch.device_sampler(), fused=False)
            assert torch.equal(unfused, eager)
            m.enable_graph_replay(True)
            smp = sch.device_sampler()
            first = chain(smp)
            second = chain(smp)                                    # the replayed graph on a rewound counter
            third = chain(smp)
            m.enable_graph_replay(False)
            assert torch.equal(first, eager) and torch.equal(second, eager) and torch.equal(third, eager)


def test_sliding_window_equals_the_unfused_path(cuda):
    """sample_sliding_window on a latent larger than the window, device sampler, against gather -> UNet per window -> ldm_window_blend ->
    ldm_rflow_step (RFlowScheduler.step with the next timestep) bit for bit; the inferer's own host loop too, and one window == sample."""
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.sliding import WindowGrid
    m = _unet(cfgs.UNET_TINY, cuda)
    sch = _flow6()
    inf = LatentDiffusionInferer(sch)
    noise = torch.randn((1, 4, 8, 8, 12), device=cuda, generator=torch.Generator(device=cuda).manual_seed(4))
    grid = WindowGrid((8, 8, 12), 8)
    assert grid.n_windows == 2
    ts = sch.timesteps.tolist()
    with torch.no_grad():
        fused = inf.sample_sliding_window(noise, None, m, (8, 8, 8), sw_batch_size=2, fused_seed=0)
        x = noise
        for k, t in enumerate(ts):
            tb = torch.full((2,), float(t), device=cuda)
            out_w = m(x=grid.gather(x), timesteps=tb, context=None).clone()
            x, _ = sch.step(grid.blend(out_w), t, x, next_timestep=_next(ts, k))
        assert torch.equal(fused, x), rel_l2(fused, x)
        assert torch.isfinite(fused).all() and not torch.equal(fused, noise)
        host = inf.sample_sliding_window(noise, None, m, (8, 8, 8), sw_batch_size=2)
        assert torch.equal(host, x)
        one = noise[..., :8].contiguous()
        a = inf.sample_sliding_window(one, None, m, (8, 8, 8), fused_seed=0)
        b = inf.sample(one, None, m, fused_seed=0)
        c = inf.sample(one, None, m)                               # the host-driven loop of sample: a flow chain draws nothing
        assert torch.equal(a, b) and torch.equal(b, c)


VCFG = dict(cfgs.VAE_TINY, in_channels=1, out_channels=1, latent_channels=4)     # 4 latent channels: UNET_TINY_COND takes 4 + 4
PATCH, LATENT = (16, 16, 16), (4, 4, 4, 4)


class _Pairs:
    randcrop, scale_on_host = False, True

    def __init__(self):
        g = torch.Generator().manual_seed(21)
        self.items = [{"image": torch.rand((1,) + PATCH, generator=g), "label": torch.rand((1,) + PATCH, generator=g)} for _ in range(3)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


@pytest.fixture(scope="module")
def world(cuda):
    from ldm3d.latents import LatentCache
    from ldm3d.networks import AutoencoderKL
    from oracle import autoencoder as oa, unet as ou
    vae = AutoencoderKL(**VCFG)
    vae.load_state_dict(ou.init_state_dict(oa.ae_param_shapes(VCFG), 2))
    vae = vae.to(cuda).eval()
    pairs = _Pairs()
    return vae, pairs, LatentCache.build(vae, pairs, cuda)


def _trainer(cuda, vae, scale=0.7311, **kw):
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.networks import DiffusionModelUNet
    from ldm3d.schedulers import RFlowScheduler
    from ldm3d.trainer import DiffusionTrainer
    from oracle import unet as ou
    unet = DiffusionModelUNet(**cfgs.UNET_TINY_COND)
    unet.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfgs.UNET_TINY_COND), 3, gain=0.5))
    return DiffusionTrainer(unet.to(cuda), vae, LatentDiffusionInferer(RFlowScheduler(**kw), scale_factor=scale), lr=1e-4)


def _manual_step(tr, noisy, cond, target, ts):
    """What a training step does after its inputs exist: UNet, mse_loss, backward, clip + Adam."""
    from ldm3d.optim import mse_loss
    tr.unet.train()
    tr.optimizer.zero_grad(set_to_none=True)
    loss = mse_loss(tr.unet(x=noisy, timesteps=ts, context=None, cond=cond), target)
    loss.backward()
    tr.optimizer.step()
    return loss.detach()


def test_trainer_uncached(cuda, world):
    """Two train_steps with explicit noise and timesteps: the loss is optim.mse_loss(unet(noisy), target) with noisy and target from the
    scheduler on the same inputs (a second trainer walks the same two steps by hand), finite, and the parameters move; then a step whose
    timesteps the scheduler draws."""
    vae, pairs, _ = world
    tr, by_hand = _trainer(cuda, vae), _trainer(cuda, vae)
    sch = by_hand.inferer.scheduler
    p0 = tr.unet.flat_params.clone()
    images = torch.stack([pairs[0]["image"], pairs[2]["image"]]).to(cuda)
    labels = torch.stack([pairs[0]["label"], pairs[2]["label"]]).to(cuda)
    g = torch.Generator().manual_seed(3)
    for k, ts in enumerate(([0, 613], [T, 250])):
        noise = torch.randn((2,) + LATENT, generator=g).to(cuda)
        ts = torch.tensor(ts, device=cuda)
        torch.manual_seed(11 + k)
        loss, skipped = tr.train_step(images, labels, noise=noise, timesteps=ts)
        torch.manual_seed(11 + k)
        with torch.no_grad():
            cond = vae.encode_stage_2_inputs(images)
            z = vae.encode_stage_2_inputs(labels) * by_hand.inferer.scale_factor
        noisy, target = sch.add_noise_and_target(original_samples=z, noise=noise, timesteps=ts)
        assert torch.equal(target, z - noise)
        want = _manual_step(by_hand, noisy, cond, target, ts)
        assert not bool(skipped) and bool(torch.isfinite(loss)) and float(loss) == float(want) and float(loss) > 0
        assert torch.equal(tr.unet.flat_params, by_hand.unet.flat_params)
    assert not torch.equal(tr.unet.flat_params, p0)
    loss, skipped = tr.train_step(images, labels)                  # timesteps from RFlowScheduler.sample_timesteps
    assert not bool(skipped) and bool(torch.isfinite(loss)) and tr.timestep_draws == 1
    drawn = tr.inferer.scheduler._drawn[0]
    assert drawn.shape == (2,) and bool((drawn >= 0).all()) and bool((drawn < T).all()) and torch.equal(drawn, torch.floor(drawn))
    for kw in (dict(), dict(sample_method="logit-normal", loc=-0.5, scale=2.0), dict(use_discrete_timesteps=False),
               dict(use_timestep_transform=True, base_img_size_numel=8)):
        from ldm3d.schedulers import RFlowScheduler
        s = RFlowScheduler(**kw)
        t = torch.cat([s.sample_timesteps(torch.empty((64,) + LATENT, device=cuda), seed=1, step=k) for k in range(8)])
        assert bool((t >= 0).all()) and bool((t < T).all()) and float(t.std()) > 0, kw


def test_trainer_cached(cuda, world):
    """train_step_cached on the same terms: explicit draws and timesteps against LatentCache.batch -> UNet -> mse_loss by hand for two
    steps; then device draws: timesteps, latent draws and noise keyed by (cache_seed, cached_steps) and the dataset indices repeat under
    one seed and leave under another, and validate_cached is finite."""
    vae, _, cache = world
    tr, by_hand = _trainer(cuda, vae), _trainer(cuda, vae)
    sch = by_hand.inferer.scheduler
    p0 = tr.unet.flat_params.clone()
    g = torch.Generator(device=cuda).manual_seed(8)
    for idx, ts in (([2, 0], [0, 613]), ([1, 1], [T, 250])):
        e_l, e_i, noise = (torch.randn((2,) + LATENT, device=cuda, generator=g) for _ in range(3))
        ts = torch.tensor(ts, device=cuda)
        loss, skipped = tr.train_step_cached(cache, idx, noise=noise, timesteps=ts, eps_label=e_l, eps_image=e_i)
        noisy, cond, target = cache.batch(idx, sch, ts, by_hand.inferer.scale_factor, eps_label=e_l, eps_image=e_i, noise=noise)
        want = _manual_step(by_hand, noisy, cond, target, ts)
        assert not bool(skipped) and bool(torch.isfinite(loss)) and float(loss) == float(want) and float(loss) > 0
        assert torch.equal(tr.unet.flat_params, by_hand.unet.flat_params)
    assert tr.cached_steps == 2 and not torch.equal(tr.unet.flat_params, p0)
    runs = []
    for seed in (3, 3, 4):
        t2 = _trainer(cuda, vae, sample_method="logit-normal")
        t2.cache_seed = seed
        losses, drawn = [], []
        for idx in ([0, 1], [2, 1]):
            loss, skipped = t2.train_step_cached(cache, idx)
            assert not bool(skipped)
            losses.append(float(loss))
            drawn.append(t2.inferer.scheduler._drawn[0].tolist())
            assert all(0 <= t < T and t == math.floor(t) for t in drawn[-1])
        assert all(x == x and x > 0 for x in losses)
        runs.append((losses, drawn, t2))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and torch.equal(runs[0][2].unet.flat_params, runs[1][2].unet.flat_params)
    assert runs[0][0] != runs[2][0] and runs[0][1] != runs[2][1]
    val = runs[0][2].validate_cached(cache, [[0, 1], [2]])
    assert val == val and 0 < val < float("inf") and runs[0][2].cached_val_steps == 2


def test_argument_errors_launch_nothing(cuda):
    """Outputs pre-filled with a sentinel and checked after the refused call."""
    from ldm3d import _lib
    L = _lib.lib()
    u = torch.rand((64,), device=cuda)

    def refused(**kw):
        outs = [torch.full((64,), 7.0, device=cuda) for _ in range(3)]
        rc = _timesteps(outs=outs, **kw)[0]
        torch.cuda.synchronize()
        return rc == BAD_ARG and all(bool((o == 7.0).all()) for o in outs)
    assert refused(draw=u, B=0) and refused(draw=u, B=65) and refused(idx=[0] * 65)
    assert refused(draw=u, method=2) and refused(draw=u, method=-1)
    assert refused(draw=u, method="logit-normal", scale=0.0) and refused(draw=u, method="logit-normal", scale=-1.0)
    assert refused(draw=u, Tn=0) and refused(draw=u, ratio=-1.0)
    for k in range(3):
        assert refused(draw=u, null=k)
    rc, t, _, _ = _timesteps(draw=u, scale=0.0)                    # uniform ignores scale; the largest batch is accepted
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(t, u * float(T))
    # a flow sampler draws nothing and keeps no state
    sch = _flow6()
    smp = sch.device_sampler()
    out = torch.full((1003,), 7.0, device=cuda)
    assert L.ldm_sampler_noise(smp._h, 0, out.data_ptr(), out.numel(), _lib.current_stream()) == BAD_ARG
    with pytest.raises(_lib.LdmError):
        smp.noise(0, (8,), cuda)
    state = torch.full((6 * 1003,), 7.0, device=cuda)
    assert L.ldm_sampler_bind_state(smp._h, state.data_ptr(), state.numel() * 4, 1003) == BAD_ARG
    with pytest.raises(_lib.LdmError):
        smp.bind_state(state, 1003)
    # a NULL tensor in ldm_rflow_noise_target, and in ldm_rflow_step
    g = torch.Generator(device=cuda).manual_seed(6)
    x0, nz = torch.randn((3, 1003), device=cuda, generator=g), torch.randn((3, 1003), device=cuda, generator=g)
    a, b = sch._noising_coefs(torch.tensor([0, 500, T], device=cuda), cuda)
    for miss in range(5):
        args = [x0, nz, a, b, None]
        args[miss] = None
        ny, tg = torch.full_like(x0, 7.0), torch.full_like(x0, 7.0)
        rc = L.ldm_rflow_noise_target(_lib.ptr(args[0]), _lib.ptr(args[1]), _lib.ptr(args[2]), _lib.ptr(args[3]), ny.data_ptr(),
                                      None if miss == 4 else tg.data_ptr(), 3, 1003, _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == BAD_ARG and bool((ny == 7.0).all()) and bool((tg == 7.0).all()), miss
    row = (C.c_float * 8)(0.1, 0.5, 0, 0, 0, 500.0, 0, 0)
    prev = torch.full((1003,), 7.0, device=cuda)
    for args in ((None, x0[0], prev), (x0[0], None, prev)):
        assert L.ldm_rflow_step(_lib.ptr(args[0]), _lib.ptr(args[1]), prev.data_ptr(), None, 1003, row, _lib.current_stream()) == BAD_ARG
    assert L.ldm_rflow_step(x0[0].data_ptr(), nz[0].data_ptr(), prev.data_ptr(), None, 1003, None, _lib.current_stream()) == BAD_ARG
    handle = C.c_void_p()
    assert L.ldm_sampler_create_rflow(None, 6, C.byref(handle)) == BAD_ARG and not handle.value
    torch.cuda.synchronize()
    assert bool((prev == 7.0).all()) and bool((out == 7.0).all()) and bool((state == 7.0).all())
    # nothing advanced the counter: the first real step is step 0
    tbuf = torch.empty((1,), device=cuda)
    smp.reset(tbuf)
    ts = sch.timesteps.tolist()
    want, _ = sch.step(nz[0], ts[0], x0[0], next_timestep=ts[1])
    x = x0[0].clone()
    smp.step(nz[0].contiguous(), x, tbuf)
    assert torch.equal(x, want) and tbuf.tolist() == [float(ts[1])]


def _env(tmp_path, **extra):
    env = {"data_base_dir": str(tmp_path / "data"), "npz_dir": str(tmp_path / "pairs"), "val_fraction": 0.25, "model_dir": str(tmp_path / "ckpt"),
           "tfevent_path": str(tmp_path / "tfevent"), "output_dir": str(tmp_path / "out"), "resume_ckpt": False, "seed": 0, **extra}
    env_file = str(tmp_path / "environment.json")
    with open(env_file, "w") as fh:
        json.dump(env, fh)
    return env_file


def test_inference_cli_samples_with_rflow(tmp_path):
    """inference.py --sampler rflow --steps 6 on the synthetic 24^3 config with the flow section: one finite volume."""
    cfg = json.load(open(os.path.join(ROOT, "config", "config_synthetic_24.json")))
    cfg["NoiseScheduler"] = dict(cfg["NoiseScheduler"], scheduler="rflow")
    cfg_file = str(tmp_path / "config_rflow_24.json")
    json.dump(cfg, open(cfg_file, "w"))
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-e", _env(tmp_path), "-c", cfg_file, "-n", "1", "--random-init",
           "--sampler", "rflow", "--steps", "6"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    vols = sorted((tmp_path / "out").glob("*.nii"))
    assert len(vols) == 1
    data = np.fromfile(vols[0], dtype=np.float32, offset=352)
    assert data.size == 96 ** 3 and np.isfinite(data).all() and float(data.std()) > 0.0


def test_train_cli_trains_a_flow_model_from_the_cache(tmp_path):
    """train_diffusion.py -c config/config_synthetic_rflow.json --synthetic 4 --max-steps 3 --cache-latents --sample-steps 4: it finishes,
    writes its checkpoints, the losses are finite and the periodic sample takes 4 Euler steps."""
    cmd = [sys.executable, os.path.join(ROOT, "train_diffusion.py"), "-e", _env(tmp_path), "-c",
           os.path.join(ROOT, "config", "config_synthetic_rflow.json"), "--random-init", "--synthetic", "4", "--max-steps", "3",
           "--cache-latents", "--sample-steps", "4"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    for name in ("diffusion_unet.pt", "diffusion_unet_last.pt", "diffusion_train_state.pt", "scale_factor.json"):
        assert os.path.exists(tmp_path / "ckpt" / name), name
    assert "NaN loss" not in log and "conditional sample (4 steps" in log, log[-3000:]
    rows = [json.loads(line) for line in open(tmp_path / "tfevent" / "diffusion" / "scalars.jsonl")]
    losses = [x["value"] for x in rows if x["tag"] == "train_diffusion_loss_iter"]
    vals = [x["value"] for x in rows if x["tag"] == "val_diffusion_loss"]
    assert len(losses) == 3 and all(v == v and 0 < v < float("inf") for v in losses + vals) and len(vals) >= 1
