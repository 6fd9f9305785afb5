"""Warm-start sampling on the GPU (-m gpu): the start kernel against float64, its device draws, the seek, reversed_step and the fused
inversion, the inferer end to end (full latent, sliding window, ensemble, guidance), the refusals and the command line."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import cfgs
import warm_start_ref as ref
from util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NAN = float("nan")


def _scheduler(kind, n=10, pred="epsilon", clip=True):
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler, RFlowScheduler
    if kind == "ddpm":
        return DDPMScheduler(**dict(cfgs.SCHED, num_train_timesteps=n), prediction_type=pred, clip_sample=clip)
    if kind == "flow":
        sch = RFlowScheduler(num_train_timesteps=1000)
    else:
        sch = DDIMScheduler(**cfgs.SCHED, prediction_type=pred, clip_sample=clip)
    sch.set_timesteps(n)
    return sch


def _rows32(sch):
    """the sampler's rows as the device holds them: rounded to fp32 once"""
    from ldm3d.schedulers import _sampler_rows
    return torch.tensor(_sampler_rows(sch, 0.0)[1], dtype=torch.float32).double().tolist()


def _unet(cfg, cuda, tame=False):
    """tame: the output projection scaled by 0.1 and fp32 arithmetic, as tests/test_gpu_sliding.py compares a host-driven DDIM loop with
    the device sampler (a random-weight UNet otherwise multiplies a last-bit difference from step to step)"""
    from ldm3d.networks import DiffusionModelUNet
    from oracle import unet as ou
    m = DiffusionModelUNet(**cfg)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfg), 1))
    if tame:
        with torch.no_grad():
            for name, p in m.named_parameters():
                if name.startswith("out.2.conv."):
                    p.mul_(0.1)
    m = m.to(cuda).eval()
    if tame:
        m.set_precision("fp32")
    return m


@functools.lru_cache(maxsize=None)
def _cond_unet(tame):
    return _unet(cfgs.UNET_TINY_COND, torch.device("cuda:0"), tame)


# ---- the start kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("per", [1, 3, 4, 5, 1025])
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "flow"])
def test_start_matches_float64(cuda, kind, per, B):
    """x = a z0 + s e against float64 on the fp32 row values, every element within the bound of the kernel's two roundings (three for
    flow); the quad tail (1, 3, 5), exactly one quad, one block and one element; one latent broadcast and one per member; the first,
    a middle and the last row; explicit noise; the output NaN-filled before the launch."""
    n = 1000 if kind == "ddpm" else 10
    sch = _scheduler(kind, n)
    smp = sch.device_sampler(seed=3)
    rows = _rows32(sch)
    g = torch.Generator(device=cuda).manual_seed(per * 7 + B)
    for zb in sorted({1, B}):
        z0 = torch.randn((zb, per), device=cuda, generator=g)
        eps = torch.randn((B, per), device=cuda, generator=g)
        for k0 in (0, n // 2, n - 1):
            out = torch.full((B, per), NAN, device=cuda)
            got = smp.start(z0, k0, B, noise=eps, out=out)
            assert got is out and torch.isfinite(out).all()
            r = rows[k0]
            a, s = (1.0 - r[1], r[1]) if kind == "flow" else (r[6], r[1])
            want = ref.noised_start(z0, eps, a, s)
            err = (out.double().cpu() - want).abs()
            gate = ref.start_gate(z0, eps, a, s, kind == "flow")
            worst = float((err / gate.clamp_min(1e-300)).max())
            print(f"{kind} per={per} B={B} z0_batch={zb} k0={k0}: max err / gate {worst:.3f}")
            assert bool((err <= gate).all()), (kind, per, B, zb, k0, worst)
        if zb == B:                                          # in place on z0: allowed when every member has its own latent
            want = smp.start(z0, n // 2, B, noise=eps)
            assert smp.start(z0, n // 2, B, noise=eps, out=z0) is z0 and torch.equal(z0, want)


def test_start_coefficients_are_the_rows_of_the_timestep(cuda):
    """the rows the kernel reads are the schedule's own: sqrt(abar_t), sqrt(1 - abar_t) of timesteps[k0] from the float64 table"""
    sch = _scheduler("ddim", 10)
    smp = sch.device_sampler(seed=0)
    ac = ref.alphas_cumprod(**cfgs.SCHED)
    one, zero = torch.ones((1, 4), device=cuda), torch.zeros((1, 4), device=cuda)
    for k0, t in enumerate(int(t) for t in sch.timesteps.tolist()):
        a = float(smp.start(one, k0, 1, noise=zero)[0, 0])
        s = float(smp.start(zero, k0, 1, noise=one)[0, 0])
        assert abs(a - ac[t] ** 0.5) <= 1e-6 and abs(s - (1 - ac[t]) ** 0.5) <= 1e-6 * max(1.0, 1 / (1 - ac[t]) ** 0.5), (k0, t, a, s)


def test_device_draws(cuda):
    """start(noise=None) is start(noise=start_noise(member)) bit for bit; a member's draw does not depend on the chunk it runs in; the
    draws are standard normal and uncorrelated with the step noise of the same seed (five-sigma bounds over N = 4 * 16^3 draws)."""
    sch = _scheduler("ddpm", 1000)
    smp = sch.device_sampler(seed=1234)
    g = torch.Generator(device=cuda).manual_seed(1)
    for shape in ((4, 3, 3, 3), (4, 8, 8, 8)):               # 108 elements per member: whole quads; 27 per channel: scalar path when odd
        z0 = torch.randn((1,) + shape, device=cuda, generator=g)
        first, B = 5, 3
        drawn = smp.start(z0, 400, B, first_member=first)
        e = torch.stack([smp.start_noise(first + j, shape, cuda) for j in range(B)])
        assert torch.equal(drawn, smp.start(z0, 400, B, noise=e))
        for j in range(B):                                   # chunking independence
            assert torch.equal(drawn[j], smp.start(z0, 400, 1, first_member=first + j)[0]), j
        assert not torch.equal(e[0], e[1])
        assert not torch.equal(e[0], smp.start_noise(first, shape, cuda, seed=1235))
        assert torch.equal(e[0], sch.device_sampler(seed=1234).start_noise(first, shape, cuda))
    odd = smp.start_noise(2, (5,), cuda)                     # the quad tail of the draw itself
    assert torch.equal(odd[:4], smp.start_noise(2, (4,), cuda)) and torch.isfinite(odd).all()
    shape = (4, 16, 16, 16)
    N = 4 * 16 ** 3
    d = smp.start_noise(0, shape, cuda).double().cpu().reshape(-1)
    step0 = smp.noise(0, shape, cuda).double().cpu().reshape(-1)
    mean, var = float(d.mean()), float(d.var(unbiased=False))
    corr = float(torch.corrcoef(torch.stack([d, step0]))[0, 1])
    print(f"start draws: mean {mean:.4f} (gate {5 / N ** 0.5:.4f}), var - 1 {var - 1:.4f} (gate {5 * (2 / N) ** 0.5:.4f}), corr with step 0 {corr:.4f}")
    assert abs(mean) <= 5 / N ** 0.5 and abs(var - 1.0) <= 5 * (2.0 / N) ** 0.5 and abs(corr) <= 5 / N ** 0.5


# ---- seek ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "flow"])
def test_seek_publishes_the_timestep_to_every_entry(cuda, kind):
    sch = _scheduler(kind, 10)
    smp = sch.device_sampler(seed=1)
    ts = sch.timesteps.tolist()
    for entries in (3, 6):                                   # B, and the 2 B of a guided step
        tbuf = torch.full((entries,), NAN, device=cuda)
        for k0 in (0, 4, 9):
            chain = smp.chain
            smp.seek(k0, tbuf)
            assert tbuf.tolist() == [float(ts[k0])] * entries and smp.chain != chain


def test_a_warm_ddpm_chain_takes_the_full_chains_steps(cuda):
    """The full chain's steps k0 ... from the full chain's x at k0, on the recorded model outputs: bit for bit, which needs step k of the
    warm chain to draw step k's z (the Philox step index is the row index, not the number of steps taken)."""
    n, k0 = 12, 5
    sch = _scheduler("ddpm", n)
    g = torch.Generator(device=cuda).manual_seed(4)
    shape = (2, 4, 3, 5, 7)
    eps = [torch.randn(shape, device=cuda, generator=g) for _ in range(n)]
    full = sch.device_sampler(seed=77)
    tbuf = torch.empty((2,), device=cuda)
    full.reset(tbuf)
    x, xs, tb = torch.randn(shape, device=cuda, generator=g), [], []
    for k in range(n):
        xs.append(x.clone())
        full.step(eps[k], x, tbuf)
        tb.append(tbuf.tolist())
    xs.append(x.clone())
    warm = sch.device_sampler(seed=77)
    tbuf2 = torch.empty((2,), device=cuda)
    warm.seek(k0, tbuf2)
    y = xs[k0].clone()
    for k in range(k0, n):
        warm.step(eps[k], y, tbuf2)
        assert torch.equal(y, xs[k + 1]) and tbuf2.tolist() == tb[k], k
    restart = sch.device_sampler(seed=77)                    # negative control: from row 0 the same inputs give another x (other z, other row)
    restart.reset(tbuf2)
    y = xs[k0].clone()
    restart.step(eps[k0], y, tbuf2)
    assert not torch.equal(y, xs[k0 + 1])


# ---- reversed_step and the inversion ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("pred", ["epsilon", "sample", "v_prediction"])
def test_reversed_step_matches_float64(cuda, pred, clip):
    """the gate of tests/test_gpu_prediction_types.py on ldm_scheduler_step (the same kernel function), float64 on the fp32 row"""
    sch = _scheduler("ddim", 10, pred, clip)
    g = torch.Generator(device=cuda).manual_seed(11)
    for t in (0, 500, 900):                                  # 900: the next timestep lies beyond the table (abar = 0)
        x = torch.randn((2, 4, 3, 5, 7), device=cuda, generator=g)
        m = torch.randn((2, 4, 3, 5, 7), device=cuda, generator=g)
        post, x0 = sch.reversed_step(m, t, x)
        r = torch.tensor(sch._inversion_row(t), dtype=torch.float32).double().tolist()
        want, want_x0 = ref.reversed_step(pred, (r[6], r[1], r[2], r[3]), m.double().cpu(), x.double().cpu(), clip)
        print(f"{pred} clip={clip} t={t}: post {rel_l2(post, want):.2e}, x0 {rel_l2(x0, want_x0):.2e}")
        assert rel_l2(post, want) <= 1e-6 and rel_l2(x0, want_x0) <= 1e-6, t
        if clip:
            assert float(x0.abs().max()) <= 1.0
    ac = ref.alphas_cumprod(**cfgs.SCHED)                    # and the rows are the float64 table's: one step against it, loosely
    want, _ = ref.reversed_step(pred, ref.coefs(ac[500], ac[600]), m.double().cpu(), x.double().cpu(), clip)
    assert rel_l2(sch.reversed_step(m, 500, x)[0], want) <= 1e-5


def test_fused_inversion_equals_the_host_driven_one(cuda):
    """invert(fused=True) (denoise_step on the inversion sampler, eager and as a replayed graph) == invert(fused=False) (forward +
    reversed_step from the host), bit for bit; four steps, so that the graph is recorded and replayed."""
    from ldm3d.inferer import LatentDiffusionInferer
    m = _unet(cfgs.UNET_TINY, cuda)
    sch = _scheduler("ddim", 10)
    inf = LatentDiffusionInferer(sch)
    z = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=torch.Generator(device=cuda).manual_seed(2))
    with torch.no_grad():
        host = inf.invert(z, m, n_steps=4, fused=False)
        assert torch.isfinite(host).all() and not torch.equal(host, z)
        for graph in (False, True):
            m.enable_graph_replay(graph)
            got = inf.invert(z, m, n_steps=4, fused=True)
            m.enable_graph_replay(False)
            assert torch.equal(got, host), (graph, rel_l2(got, host))
        smp = sch.inversion_sampler(4)
        assert smp.timesteps == [0, 100, 200, 300] and smp.n_steps == 4


def test_windowed_inversion_equals_its_pieces(cuda):
    """invert(roi_size=...) on a latent of two windows: the windowed device step on the inversion rows == gather -> forward per window
    -> blend -> reversed_step from the host, bit for bit, eager and replayed (the rows go through denoise_step_windows as they are)."""
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.sliding import WindowGrid
    m = _cond_unet(False)
    sch = _scheduler("ddim", 10)
    inf = LatentDiffusionInferer(sch)
    g = torch.Generator(device=cuda).manual_seed(12)
    shape = (1, 4, 8, 8, 13)
    z = torch.randn(shape, device=cuda, generator=g) * 0.5
    cond = torch.randn(shape, device=cuda, generator=g)
    grid = WindowGrid(shape[2:], (8, 8, 8))
    assert grid.n_windows == 2
    with torch.no_grad():
        cw = grid.gather(cond)
        x = z.clone()
        for t in sch.inversion_timesteps(4):
            xw = grid.gather(x)
            eps_w = torch.stack([m(x=xw[w:w + 1], timesteps=torch.full((1,), float(t), device=cuda), cond=cw[w:w + 1])[0].clone() for w in range(2)])
            x, _ = sch.reversed_step(grid.blend(eps_w), t, x)
        for graph in (False, True):
            m.enable_graph_replay(graph)
            got = inf.invert(z, m, conditioning=cond, n_steps=4, roi_size=(8, 8, 8), sw_batch_size=1)
            m.enable_graph_replay(False)
            assert torch.equal(got, x), (graph, rel_l2(got, x))
        with pytest.raises(ValueError):
            inf.invert(z, m, conditioning=cond, n_steps=4, roi_size=(8, 8, 8), fused=False)
    assert torch.isfinite(x).all() and not torch.equal(x, z)


# ---- the inferer, end to end -----------------------------------------------------------------------------------------------------
def _count(m, name):
    """wrap m.<name> with a call counter -> (the list the calls are appended to, undo)"""
    calls, fn = [], getattr(m, name)

    def counted(*a, **kw):
        calls.append(1)
        return fn(*a, **kw)
    setattr(m, name, counted)
    return calls, lambda: delattr(m, name)


@pytest.mark.parametrize("cfg", [None, 2.0])
@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_sample_equals_seek_start_and_hand_driven_steps(cuda, kind, cfg):
    """sample(init_latent, start_step=k0, fused_seed) == seek + start + n - k0 denoise_step calls, bit for bit, eager and replayed; it
    makes exactly n - k0 UNet calls.  One latent broadcast to B = 2 members, the start drawn on the device; cfg: tbuf has 2 B entries."""
    from ldm3d.inferer import LatentDiffusionInferer
    m = _cond_unet(False)
    n, k0, B = 8, 3, 2
    sch = _scheduler(kind, n)
    inf = LatentDiffusionInferer(sch)
    g = torch.Generator(device=cuda).manual_seed(6)
    z0 = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g) * 0.5
    cond = torch.randn((B, 4, 8, 8, 8), device=cuda, generator=g)
    kw = {} if cfg is None else dict(guidance=cfg, guidance_fill=-1.0)
    with torch.no_grad():
        smp = sch.device_sampler(9)
        tbuf = torch.full((B if cfg is None else 2 * B,), NAN, device=cuda)
        smp.seek(k0, tbuf)
        assert tbuf.tolist() == [float(sch.timesteps[k0])] * tbuf.numel()
        x = smp.start(z0, k0, B, 9)
        assert not torch.equal(x[0], x[1])
        for _ in range(n - k0):
            m.denoise_step(x, tbuf, smp, cond=cond, **kw)
        for graph in (False, True):
            m.enable_graph_replay(graph)
            calls, undo = _count(m, "denoise_step")
            try:
                got = inf.sample(None, None, m, conditioning=cond, mode="concat", fused_seed=9, init_latent=z0, start_step=k0, cfg=cfg)
            finally:
                undo()
                m.enable_graph_replay(False)
            assert len(calls) == n - k0
            assert torch.equal(got, x), (kind, cfg, graph, rel_l2(got, x))
        full = inf.sample(torch.randn((B, 4, 8, 8, 8), device=cuda, generator=g), None, m, conditioning=cond, mode="concat", fused_seed=9, cfg=cfg)
        assert torch.isfinite(x).all() and not torch.equal(full, x)
        # the start already at timesteps[k0] (what invert returns): no noise is added, the same steps follow
        inv = inf.sample(None, None, m, conditioning=cond, mode="concat", fused_seed=9, init_latent=smp.start(z0, k0, B, 9), start_step=k0,
                         init_inverted=True, cfg=cfg)
        assert torch.equal(inv, x)


def test_host_driven_warm_chain_agrees_with_the_fused_one(cuda):
    """DDIM, eta = 0, the same explicit start noise: the host loop (add_noise, then forward + DDIMScheduler.step) against the device
    sampler, at the gate of the existing fused-vs-host tests (the two noising kernels may round the start differently in the last bit,
    hence the tame fp32 model of tests/test_gpu_sliding.py); n - k0 forwards."""
    from ldm3d.inferer import LatentDiffusionInferer
    m = _cond_unet(True)
    n, k0, B = 6, 2, 2
    sch = _scheduler("ddim", n)
    inf = LatentDiffusionInferer(sch)
    g = torch.Generator(device=cuda).manual_seed(8)
    z0 = torch.randn((B, 4, 8, 8, 8), device=cuda, generator=g) * 0.5
    noise = torch.randn((B, 4, 8, 8, 8), device=cuda, generator=g)
    cond = torch.randn((B, 4, 8, 8, 8), device=cuda, generator=g)
    with torch.no_grad():
        calls, undo = _count(m, "forward")
        try:
            host = inf.sample(noise, None, m, conditioning=cond, mode="concat", init_latent=z0, start_step=k0)
        finally:
            undo()
        fused = inf.sample(noise, None, m, conditioning=cond, mode="concat", init_latent=z0, start_step=k0, fused_seed=1)
        with pytest.raises(ValueError):
            inf.sample(None, None, m, conditioning=cond, mode="concat", init_latent=z0, start_step=k0)      # the host loop draws nothing itself
    print(f"host vs fused warm chain: {rel_l2(fused, host):.2e}")
    assert len(calls) == n - k0 and torch.isfinite(host).all()
    assert rel_l2(fused, host) <= 1e-5


def test_sliding_window_warm_start(cuda):
    """The whole latent is noised once, then the windowed steps: sample_sliding_window(init_latent, start_step, fused_seed) == seek +
    start + n - k0 denoise_step_windows calls bit for bit, and agrees with the unfused windowed loop as tests/test_gpu_sliding.py
    compares the two (DDIM, tame fp32 model, 1e-5)."""
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.sliding import WindowGrid
    m = _cond_unet(True)
    n, k0 = 5, 2
    sch = _scheduler("ddim", n)
    inf = LatentDiffusionInferer(sch)
    g = torch.Generator(device=cuda).manual_seed(9)
    shape = (1, 4, 8, 8, 13)
    z0 = torch.randn(shape, device=cuda, generator=g) * 0.5
    noise = torch.randn(shape, device=cuda, generator=g)
    cond = torch.randn(shape, device=cuda, generator=g)
    with torch.no_grad():
        host = inf.sample_sliding_window(noise, None, m, (8, 8, 8), sw_batch_size=1, conditioning=cond, init_latent=z0, start_step=k0)
        calls, undo = _count(m, "denoise_step_windows")
        try:
            fused = inf.sample_sliding_window(noise, None, m, (8, 8, 8), sw_batch_size=1, conditioning=cond, fused_seed=3, init_latent=z0,
                                              start_step=k0)
        finally:
            undo()
        grid = WindowGrid(shape[2:], (8, 8, 8))
        assert grid.n_windows == 2
        smp = sch.device_sampler(3)
        tbuf = torch.empty((1,), device=cuda)
        smp.seek(k0, tbuf)
        x = smp.start(z0, k0, 1, 3, noise=noise)
        cw = grid.gather(cond)
        for _ in range(n - k0):
            m.denoise_step_windows(x, tbuf, smp, grid, cond_windows=cw, sw_batch_size=1)
        drawn = inf.sample_sliding_window(None, None, m, (8, 8, 8), sw_batch_size=1, conditioning=cond, fused_seed=3, init_latent=z0, start_step=k0)
    print(f"windowed host vs fused warm chain: {rel_l2(fused, host):.2e}")
    assert len(calls) == n - k0 and torch.equal(fused, x)
    assert rel_l2(fused, host) <= 1e-5
    assert torch.isfinite(drawn).all() and not torch.equal(drawn, fused)      # input_noise=None: the start drawn on the device


def test_ensemble_of_warm_members_is_the_same_under_any_chunking(cuda):
    """Four warm members of a deterministic sampler (DDIM, eta = 0) run 1, 2 and 4 at a time: every member starts from the draw keyed
    by its global index, so the mean moves only by the UNet's batch dependence (fp32 summation order: the 5e-5 of
    tests/test_gpu_sliding.py's chunking test); the latent itself stands for the decoded volume (no autoencoder)."""
    from ldm3d.inferer import LatentDiffusionInferer
    m = _cond_unet(True)
    sch = _scheduler("ddim", 4)
    inf = LatentDiffusionInferer(sch)
    g = torch.Generator(device=cuda).manual_seed(10)
    z0 = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g) * 0.5
    cond = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g)
    res = {}
    with torch.no_grad():
        for mb in (1, 2, 4):
            calls, undo = _count(m, "denoise_step")
            try:
                res[mb] = inf.sample_ensemble(4, (4, 8, 8, 8), None, m, conditioning=cond, member_batch=mb, seed=21, init_latent=z0, start_step=1,
                                              keep_members=4)
            finally:
                undo()
            assert len(calls) == 3 * (4 // mb) and res[mb].count == 4
        cold = inf.sample_ensemble(4, (4, 8, 8, 8), None, m, conditioning=cond, member_batch=2, seed=21)
    for mb in (2, 4):
        em, es = rel_l2(res[mb].mean, res[1].mean), rel_l2(res[mb].members, res[1].members)
        print(f"member_batch {mb} vs 1: mean {em:.2e}, members {es:.2e}")
        assert em <= 5e-5 and es <= 5e-5
    assert float(res[1].std.max()) > 0 and not torch.equal(res[1].members[0], res[1].members[1])
    assert not torch.equal(cold.mean, res[2].mean)           # without init_latent nothing changed: the host-drawn pure-noise starts


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(cuda, built_lib):
    from ldm3d import _lib
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.schedulers import PNDMScheduler
    L = built_lib
    ddim = _scheduler("ddim", 10)
    smp = ddim.device_sampler(seed=1)
    pndm = PNDMScheduler(skip_prk_steps=True, **cfgs.SCHED)
    pndm.set_timesteps(10)
    psmp = pndm.device_sampler()
    B, per = 3, 20
    tbuf = torch.full((B,), -7.0, device=cuda)
    z0 = torch.ones((B, per), device=cuda)
    x = torch.full((B, per), NAN, device=cuda)
    e = torch.ones((B, per), device=cuda)
    s = _lib.current_stream()
    BAD = -1
    assert L.ldm_sampler_seek(psmp._h, 1, tbuf.data_ptr(), B, s) == BAD                  # PNDM: from its first row only
    assert b"PNDM" in L.ldm_last_error()
    assert L.ldm_sampler_start(psmp._h, 0, z0.data_ptr(), B, e.data_ptr(), x.data_ptr(), B, per, 0, 0, s) == BAD
    for k0 in (-1, 10):
        assert L.ldm_sampler_seek(smp._h, k0, tbuf.data_ptr(), B, s) == BAD
        assert L.ldm_sampler_start(smp._h, k0, z0.data_ptr(), B, e.data_ptr(), x.data_ptr(), B, per, 0, 0, s) == BAD
    assert L.ldm_sampler_start(smp._h, 2, z0.data_ptr(), 2, e.data_ptr(), x.data_ptr(), B, per, 0, 0, s) == BAD      # z0_batch not in {1, B}
    assert L.ldm_sampler_start(smp._h, 2, x.data_ptr(), 1, e.data_ptr(), x.data_ptr(), B, per, 0, 0, s) == BAD       # in place on a broadcast latent
    assert L.ldm_sampler_start(smp._h, 2, z0.data_ptr(), B, x.data_ptr(), x.data_ptr(), B, per, 0, 0, s) == BAD      # in place on the noise
    assert L.ldm_sampler_seek(None, 2, tbuf.data_ptr(), B, s) == BAD and L.ldm_sampler_seek(smp._h, 2, None, B, s) == BAD
    assert L.ldm_sampler_seek(smp._h, 2, tbuf.data_ptr(), 0, s) == BAD
    assert L.ldm_sampler_start(None, 2, z0.data_ptr(), B, e.data_ptr(), x.data_ptr(), B, per, 0, 0, s) == BAD
    assert L.ldm_sampler_start(smp._h, 2, None, B, e.data_ptr(), x.data_ptr(), B, per, 0, 0, s) == BAD
    assert L.ldm_sampler_start(smp._h, 2, z0.data_ptr(), B, e.data_ptr(), None, B, per, 0, 0, s) == BAD
    assert L.ldm_sampler_start(smp._h, 2, z0.data_ptr(), B, e.data_ptr(), x.data_ptr(), 0, per, 0, 0, s) == BAD
    assert L.ldm_sampler_start(smp._h, 2, z0.data_ptr(), B, e.data_ptr(), x.data_ptr(), B, 0, 0, 0, s) == BAD
    assert L.ldm_sampler_start_noise(0, 0, None, per, s) == BAD and L.ldm_sampler_start_noise(0, 0, x.data_ptr(), 0, s) == BAD
    with pytest.raises(_lib.LdmError):
        psmp.seek(3, tbuf)
    with pytest.raises(_lib.LdmError):
        psmp.start(z0, 0, B, noise=e, out=x)
    with pytest.raises(ValueError):
        ddim.inversion_sampler(eta=0.3)
    with pytest.raises(ValueError):
        LatentDiffusionInferer(ddim).invert(torch.zeros((1, 4, 8, 8, 8), device=cuda), None, eta=0.3)
    torch.cuda.synchronize()
    assert bool(torch.isnan(x).all()) and tbuf.tolist() == [-7.0] * B                     # nothing was written
    assert L.ldm_sampler_seek(psmp._h, 0, tbuf.data_ptr(), B, s) == 0                     # what is allowed still runs
    assert L.ldm_sampler_start(smp._h, 2, z0.data_ptr(), B, e.data_ptr(), x.data_ptr(), B, per, 0, 0, s) == 0
    torch.cuda.synchronize()
    assert tbuf.tolist() == [float(pndm.timesteps[0])] * B and torch.isfinite(x).all()


# ---- the command line ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invert", [False, True])
def test_inference_cli_warm_start(tmp_path, invert):
    from ldm3d.data import write_synthetic_pairs
    pair = write_synthetic_pairs(str(tmp_path / "pairs"), 1, (100, 96, 120))[0]
    env = {"npz_dir": str(tmp_path / "pairs"), "model_dir": str(tmp_path / "ckpt"), "output_dir": str(tmp_path / "out"),
           "tfevent_path": str(tmp_path / "tfevent"), "resume_ckpt": False, "seed": 0}
    env_file = str(tmp_path / "environment.json")
    with open(env_file, "w") as fh:
        json.dump(env, fh)
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-e", env_file, "-c", os.path.join(ROOT, "config", "config_synthetic_train.json"),
           "--random-init", "--steps", "10", "--condition", pair, "--init-from-condition", "--strength", "0.4"] + (["--init-invert"] if invert else [])
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = tmp_path / "out"
    vols = sorted(out.glob("synimg_*.nii"))
    assert len(vols) == 1
    import numpy as np
    data = np.fromfile(vols[0], dtype=np.float32, offset=352)
    assert data.size == 96 ** 3 and np.isfinite(data).all()
    recs = [json.loads(l) for l in open(out / "warm_start.jsonl")]
    assert len(recs) == 1
    rec = recs[0]
    assert rec["file"] == vols[0].name and rec["start_step"] == 6 and rec["unet_calls"] == 4 and rec["strength"] == 0.4
    assert rec["mode"] == ("inverted" if invert else "noised")
    assert rec.get("inversion_calls") == (3 if invert else None)


@pytest.mark.parametrize("flags", [["--sliding-window", "--init-invert", "--cfg", "2.0", "--metrics"], ["--ensemble", "2", "--sampler", "ddim"]],
                         ids=["whole-scan-inverted-guided-scored", "ensemble"])
def test_inference_cli_warm_start_composes(tmp_path, flags):
    """the flags it is valid with: the whole scan by sliding windows from a windowed inversion, guided and scored; an ensemble whose
    members start from the scan's latent.  The warm-start fields land in the run's own records."""
    from ldm3d.data import write_synthetic_pairs
    pair = write_synthetic_pairs(str(tmp_path / "pairs"), 1, (100, 96, 120))[0]
    env = {"npz_dir": str(tmp_path / "pairs"), "model_dir": str(tmp_path / "ckpt"), "output_dir": str(tmp_path / "out"),
           "tfevent_path": str(tmp_path / "tfevent"), "resume_ckpt": False, "seed": 0}
    env_file = str(tmp_path / "environment.json")
    with open(env_file, "w") as fh:
        json.dump(env, fh)
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-e", env_file, "-c", os.path.join(ROOT, "config", "config_synthetic_train.json"),
           "--random-init", "--steps", "5", "--condition", pair, "--init-from-condition", "--strength", "0.6"] + flags
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = tmp_path / "out"
    want = {"start_step": 2, "unet_calls": 3, "strength": 0.6}
    if "--ensemble" in flags:
        rec = [json.loads(l) for l in open(out / "ensemble.jsonl")][0]
        assert rec["members"] == 2 and rec["mode"] == "noised" and rec["max_std"] > 0
    else:
        rec = [json.loads(l) for l in open(out / "metrics.jsonl")][0]
        assert rec["mode"] == "inverted" and rec["inversion_calls"] == 2 and rec["shape"] == [100, 96, 120]
        assert [json.loads(l) for l in open(out / "warm_start.jsonl")][0]["file"] == rec["file"]
    assert {k: rec[k] for k in want} == want


def test_inference_cli_refuses(tmp_path, monkeypatch, capsys):
    """the refused flag combinations exit non-zero (argparse errors, raised before any device work: parsed in process)"""
    from test_warm_start_cpu import REFUSED, parse
    for argv in REFUSED:
        with pytest.raises(SystemExit) as e:
            parse(argv, tmp_path, monkeypatch)
        assert e.value.code != 0, argv
        assert "error" in capsys.readouterr().err, argv
