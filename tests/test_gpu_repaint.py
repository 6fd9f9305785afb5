"""Inpainting (RePaint) on the GPU (-m gpu): the merge against float64, the fused step against its pieces bit for bit, the degenerate
masks, the three noise streams, the inferer end to end (full latent, guidance, sliding window, ensemble), the refusals and the command
line."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import cfgs
import repaint_ref as ref
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


def _rows32(rows):
    """rows as the device holds them: rounded to fp32 once"""
    return torch.tensor(rows, dtype=torch.float32).double().tolist()


def _unet(cfg, cuda, tame=False):
    """tame: the output projection scaled by 0.1 and fp32 arithmetic (tests/test_gpu_warm_start.py's)"""
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


def _mask(shape, cuda, seed, p=0.5):
    """a 0 / 1 mask with both values wherever it has two elements"""
    g = torch.Generator(device=cuda).manual_seed(seed)
    m = (torch.rand(shape, device=cuda, generator=g) < p).float()
    if m.numel() > 1:
        m.view(-1)[0], m.view(-1)[-1] = 1.0, 0.0
    return m


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the merge -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C,DHW", [(1, 1), (3, 1), (2, 2), (1, 5), (5, 205)])
def test_merge_matches_float64(cuda, C, DHW, B):
    """ldm_repaint_merge against float64 on the fp32 coefficients, every element within the bound of the function's spelled-out roundings
    (repaint_ref.merge_gate); quad tails and quads that straddle a channel or sample boundary; one known latent broadcast and one per
    sample; the first row, a jump row and the last row of a table; explicit draws; the output NaN-filled before the launch.  Kept
    elements of the last row are the known latent's bits; elements that are neither kept nor jumped are the input's bits."""
    from ldm3d.schedulers import repaint_merge, repaint_rows
    schedule, rows = repaint_rows(_scheduler("ddim", 6), 2, 2)
    rows = _rows32(rows)
    picks = [0, next(k for k, (_, j) in enumerate(schedule) if j), len(rows) - 1]
    assert not schedule[0][1] and not schedule[-1][1] and rows[-1][8:10] == [1.0, 0.0]
    g = torch.Generator(device=cuda).manual_seed(C * 1000 + DHW * 10 + B)
    masks = [torch.zeros((DHW,), device=cuda), torch.ones((DHW,), device=cuda)] if DHW == 1 else [_mask((DHW,), cuda, DHW)]
    for keep in masks:
        for kb in sorted({1, B}):
            x = torch.randn((B, C, DHW), device=cuda, generator=g)
            known = torch.randn((kb, C, DHW), device=cuda, generator=g)
            zk = torch.randn((B, C, DHW), device=cuda, generator=g)
            zj = torch.randn((B, C, DHW), device=cuda, generator=g)
            kp = (keep != 0).expand(B, C, DHW)
            for k in picks:
                c4, jump = rows[k][8:12], schedule[k][1]
                out = torch.full((B, C, DHW), NAN, device=cuda)
                got = repaint_merge(x, known, keep, c4, jump, z_known=zk, z_jump=zj, out=out)
                assert got is out and torch.isfinite(out).all()
                want = ref.merge(x, known, keep, c4, jump, zk, zj)
                gate = ref.merge_gate(x, known, keep, c4, jump, zk, zj)
                err = (out.double().cpu() - want).abs()
                worst = float((err / gate.clamp_min(1e-300)).max()) if bool((gate > 0).any()) else 0.0
                print(f"C={C} DHW={DHW} B={B} known_batch={kb} row={k} jump={jump}: max err / gate {worst:.3f}")
                assert bool((err <= gate).all()), (C, DHW, B, kb, k, worst)
                if not jump:
                    assert torch.equal(_bits(out)[~kp], _bits(x)[~kp])
                if k == len(rows) - 1:
                    assert torch.equal(_bits(out)[kp], _bits(known.expand(B, C, DHW))[kp])
                    assert torch.equal(repaint_merge(x, known, keep, c4, False), out)      # no draw is needed where its coefficient is 0
            alias = x.clone()                                # in place on x
            assert repaint_merge(alias, known, keep, rows[picks[1]][8:12], True, z_known=zk, z_jump=zj, out=alias) is alias
            assert torch.equal(alias, repaint_merge(x, known, keep, rows[picks[1]][8:12], True, z_known=zk, z_jump=zj))


# ---- the fused step --------------------------------------------------------------------------------------------------------------
CASES = [(k, p, e) for k, e in (("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5)) for p in ("epsilon", "sample", "v_prediction")] + [("flow", "epsilon", 0.0)]


@pytest.mark.parametrize("kind,pred,eta", CASES, ids=[f"{k}-{p}-eta{e}" for k, p, e in CASES])
def test_fused_step_equals_its_pieces(cuda, kind, pred, eta):
    """sampler.step on the repaint sampler == the plain device step on the base rows (the host-driven flow step for rectified flow)
    followed by repaint_merge with the accessors' draws, bit for bit, x and x0_hat, over a whole n = 6, jump_length = 2, n_resample = 2
    table; tbuf after every row is the next row's t, the rise at a jump included; a step past the end touches nothing."""
    from ldm3d.schedulers import DeviceSampler, repaint_merge
    n = 6
    sch = _scheduler(kind, n, pred)
    shape = (2, 4, 3, 5, 7)                                  # 105 voxels: quads straddle channels and samples
    g = torch.Generator(device=cuda).manual_seed(17)
    keep = _mask(shape[2:], cuda, 3)
    rises = 0
    for kb in (1, 2):
        known = torch.randn((kb,) + shape[1:], device=cuda, generator=g)
        rs = sch.repaint_sampler(known, keep, jump_length=2, n_resample=2, seed=77, eta=eta)
        assert rs.n_calls == rs.n_steps == 10 == ref.n_calls(n, 2, 2) and rs.schedule == ref.schedule(n, 2, 2)
        rows = _rows32(rs.rows)
        ts = sch.timesteps.tolist()
        plain = None if kind == "flow" else DeviceSampler(sch, 77, eta, rows=rs.base_rows)
        tbuf, tbuf2 = torch.full((2,), NAN, device=cuda), torch.full((2,), NAN, device=cuda)
        rs.reset(tbuf)
        assert tbuf.tolist() == [float(ts[0])] * 2
        if plain is not None:
            plain.reset(tbuf2)
        x = torch.randn(shape, device=cuda, generator=g)
        for k, (level, jump) in enumerate(rs.schedule):
            eps = torch.randn(shape, device=cuda, generator=g)
            y, x0, x0b = x.clone(), torch.full(shape, NAN, device=cuda), torch.full(shape, NAN, device=cuda)
            rs.step(eps, x, tbuf, x0_out=x0)
            if plain is None:
                y, x0b = sch.step(eps, ts[level], y, next_timestep=ts[level + 1] if level + 1 < n else 0)
            else:
                plain.step(eps, y, tbuf2, x0_out=x0b)
            want = repaint_merge(y.contiguous(), rs.known, rs.keep, rs.rows[k][8:12], jump,
                                 z_known=rs.noise_known(k, shape, cuda) if rows[k][9] != 0.0 else None,
                                 z_jump=rs.noise_jump(k, shape, cuda) if jump else None)
            assert torch.equal(x, want), (kind, pred, eta, kb, k, rel_l2(x, want))
            assert torch.equal(x0, x0b), (kind, pred, eta, kb, k)
            t_next = rows[k + 1][5] if k + 1 < len(rows) else rows[k][5]
            assert tbuf.tolist() == [t_next] * 2, (k, tbuf.tolist(), t_next)
            if jump:
                assert t_next > rows[k][5]
                rises += 1
        assert torch.isfinite(x).all()
        kp = (rs.keep != 0).expand(shape)
        assert torch.equal(_bits(x)[kp], _bits(rs.known.expand(shape))[kp])      # the chain ends on the known latent where it is kept
        before, tb = x.clone(), tbuf.clone()
        rs.step(torch.randn(shape, device=cuda, generator=g), x, tbuf)            # past the end
        assert torch.equal(x, before) and torch.equal(tbuf, tb)
    assert rises == 4


def test_all_zero_mask_is_the_plain_chain(cuda):
    """nothing kept, n_resample = 1: the plain device chain of the same seed, bit for bit (the step noise of row k is step k's)"""
    n, shape = 8, (2, 4, 3, 5, 7)
    sch = _scheduler("ddpm", n)
    g = torch.Generator(device=cuda).manual_seed(5)
    rs = sch.repaint_sampler(torch.randn((1,) + shape[1:], device=cuda, generator=g), torch.zeros(shape[2:], device=cuda), seed=9)
    plain = sch.device_sampler(9)
    assert rs.n_calls == n
    ta, tb = torch.empty((2,), device=cuda), torch.empty((2,), device=cuda)
    rs.reset(ta)
    plain.reset(tb)
    x = torch.randn(shape, device=cuda, generator=g)
    y = x.clone()
    for k in range(n):
        eps = torch.randn(shape, device=cuda, generator=g)
        rs.step(eps, x, ta)
        plain.step(eps, y, tb)
        assert torch.equal(x, y) and torch.equal(ta, tb), k
    assert torch.isfinite(x).all()


def test_all_ones_mask_forgets_the_model(cuda):
    """everything kept: after every row x is a function of the known latent and the draws alone - two chains on different model outputs
    and different starts hold the same bits"""
    shape = (2, 4, 3, 5, 7)
    sch = _scheduler("ddpm", 6)
    g = torch.Generator(device=cuda).manual_seed(6)
    known = torch.randn(shape, device=cuda, generator=g)
    keep = torch.ones(shape[2:], device=cuda)
    xs = []
    for trial in range(2):
        rs = sch.repaint_sampler(known, keep, jump_length=2, n_resample=2, seed=4)
        tbuf = torch.empty((2,), device=cuda)
        rs.reset(tbuf)
        x = torch.randn(shape, device=cuda, generator=g)
        trace = []
        for k in range(rs.n_calls):
            rs.step(torch.randn(shape, device=cuda, generator=g), x, tbuf)
            trace.append(x.clone())
        xs.append(trace)
    for k, (a, b) in enumerate(zip(*xs)):
        assert torch.equal(a, b), k
    assert torch.equal(xs[0][-1], known) and not torch.equal(xs[0][0], known)


def test_draws(cuda):
    """the three streams of one seed over N = 4 * 16^3 draws: standard normal and pairwise uncorrelated (five-sigma bounds); different
    rows draw differently; the same seed, row and element repeat; the quad tail of the accessor"""
    shape = (4, 16, 16, 16)
    N = 4 * 16 ** 3
    sch = _scheduler("ddpm", 10)
    known, keep = torch.zeros((1,) + shape, device=cuda), torch.ones(shape[1:], device=cuda)
    rs = sch.repaint_sampler(known, keep, seed=1234)
    row = 3
    draws = {"step": rs.noise(row, shape, cuda), "known": rs.noise_known(row, shape, cuda), "jump": rs.noise_jump(row, shape, cuda)}
    for name, d in draws.items():
        v = d.double().cpu().reshape(-1)
        mean, var = float(v.mean()), float(v.var(unbiased=False))
        print(f"{name} draws: mean {mean:.4f} (gate {5 / N ** 0.5:.4f}), var - 1 {var - 1:.4f} (gate {5 * (2 / N) ** 0.5:.4f})")
        assert abs(mean) <= 5 / N ** 0.5 and abs(var - 1.0) <= 5 * (2.0 / N) ** 0.5, name
    names = list(draws)
    for i in range(3):
        for j in range(i + 1, 3):
            r = float(torch.corrcoef(torch.stack([draws[names[i]].double().cpu().reshape(-1), draws[names[j]].double().cpu().reshape(-1)]))[0, 1])
            print(f"corr({names[i]}, {names[j]}) = {r:.4f} (gate {5 / N ** 0.5:.4f})")
            assert abs(r) <= 5 / N ** 0.5, (names[i], names[j], r)
    again = sch.repaint_sampler(known, keep, seed=1234)
    other = sch.repaint_sampler(known, keep, seed=1235)
    for fn in ("noise_known", "noise_jump"):
        d = getattr(rs, fn)(row, shape, cuda)
        assert torch.equal(d, getattr(again, fn)(row, shape, cuda))
        assert not torch.equal(d, getattr(rs, fn)(row + 1, shape, cuda)) and not torch.equal(d, getattr(other, fn)(row, shape, cuda))
        odd = getattr(rs, fn)(row, (5,), cuda)
        assert torch.equal(odd[:4], getattr(rs, fn)(row, (4,), cuda)) and torch.equal(odd, d.reshape(-1)[:5])


# ---- the inferer -----------------------------------------------------------------------------------------------------------------
def _count(m, name):
    calls, fn = [], getattr(m, name)

    def counted(*a, **kw):
        calls.append(1)
        return fn(*a, **kw)
    setattr(m, name, counted)
    return calls, lambda: delattr(m, name)


@pytest.mark.parametrize("cfg", [None, 2.0])
def test_sample_equals_hand_driven_steps(cuda, cfg):
    """sample(inpaint_latent, keep_mask, fused_seed) == n_calls denoise_step calls on the repaint sampler, bit for bit, eager and
    replayed; the final latent is the known latent inside the mask, bit for bit, and differs from the unconstrained chain outside it.
    DDPM of 6 timesteps, jump_length 2, n_resample 2: 10 UNet calls."""
    from ldm3d.inferer import LatentDiffusionInferer
    m = _cond_unet(True)
    sch = _scheduler("ddpm", 6)
    inf = LatentDiffusionInferer(sch)
    g = torch.Generator(device=cuda).manual_seed(21)
    shape = (1, 4, 8, 8, 8)
    noise = torch.randn(shape, device=cuda, generator=g)
    known = torch.randn(shape, device=cuda, generator=g) * 0.5
    cond = torch.randn(shape, device=cuda, generator=g)
    keep = torch.ones(shape[2:], device=cuda)
    keep[2:6, 1:5, 3:8] = 0.0
    kw = {} if cfg is None else dict(guidance=cfg, guidance_fill=-1.0)
    with torch.no_grad():
        rs = sch.repaint_sampler(known, keep, 2, 2, seed=9)
        assert rs.n_calls == 10
        tbuf = torch.full((1 if cfg is None else 2,), NAN, device=cuda)
        rs.reset(tbuf)
        x = noise.clone()
        for _ in range(rs.n_calls):
            m.denoise_step(x, tbuf, rs, cond=cond, **kw)
        for graph in (False, True):
            m.enable_graph_replay(graph)
            calls, undo = _count(m, "denoise_step")
            try:
                got = inf.sample(noise, None, m, conditioning=cond, mode="concat", fused_seed=9, cfg=cfg, inpaint_latent=known,
                                 keep_mask=keep[None, None], jump_length=2, n_resample=2)
            finally:
                undo()
                m.enable_graph_replay(False)
            assert len(calls) == 10
            assert torch.equal(got, x), (cfg, graph, rel_l2(got, x))
        free = inf.sample(noise, None, m, conditioning=cond, mode="concat", fused_seed=9, cfg=cfg)
    kp = (keep != 0).expand(shape)
    assert torch.isfinite(x).all()
    assert torch.equal(_bits(x)[kp], _bits(known)[kp])
    assert not torch.equal(x[~kp], free[~kp]) and not torch.equal(x[~kp], known[~kp])


def test_rebinding_never_replays_the_old_graph(cuda):
    """graph mode: a sampler rebound to another known latent and mask steps on the new tensors (the binding is part of the replay key)"""
    m = _cond_unet(True)
    sch = _scheduler("ddim", 3)
    g = torch.Generator(device=cuda).manual_seed(23)
    shape = (1, 4, 8, 8, 8)
    noise, cond = torch.randn(shape, device=cuda, generator=g), torch.randn(shape, device=cuda, generator=g)
    k1, k2 = torch.randn(shape, device=cuda, generator=g), torch.randn(shape, device=cuda, generator=g)
    m1, m2 = _mask(shape[2:], cuda, 1), _mask(shape[2:], cuda, 2)
    tbuf = torch.empty((1,), device=cuda)
    x = torch.empty(shape, device=cuda)

    def chain(rs):
        rs.reset(tbuf)
        x.copy_(noise)
        for _ in range(rs.n_calls):
            m.denoise_step(x, tbuf, rs, cond=cond)
        return x.clone()

    with torch.no_grad():
        want1, want2 = chain(sch.repaint_sampler(k1, m1, seed=2)), chain(sch.repaint_sampler(k2, m2, seed=2))
        m.enable_graph_replay(True)
        try:
            rs = sch.repaint_sampler(k1, m1, seed=2)
            got1 = chain(rs)
            got1b = chain(rs)                                # recorded by now: replayed
            rs.bind(k2, m2)
            got2 = chain(rs)
            got2b = chain(rs)
        finally:
            m.enable_graph_replay(False)
    assert torch.equal(got1, want1) and torch.equal(got1b, want1)
    assert torch.equal(got2, want2) and torch.equal(got2b, want2) and not torch.equal(want1, want2)


def test_host_driven_loop_agrees_with_the_fused_one(cuda):
    """The host-driven loop (forward, the scheduler's step, repaint_merge) fed the accessors' draws against the fused chain: 1e-5 rel-L2,
    the project's gate for a host-driven against a fused chain at this call count.  Yardstick, measured first with existing code: the plain
    10-step DDPM chain host-driven (step_noise = the device sampler's draws) against fused; were that alone above 5e-6, the gate would
    be twice it."""
    from ldm3d.inferer import LatentDiffusionInferer
    m = _cond_unet(True)
    g = torch.Generator(device=cuda).manual_seed(22)
    shape = (1, 4, 8, 8, 8)
    noise = torch.randn(shape, device=cuda, generator=g)
    known = torch.randn(shape, device=cuda, generator=g) * 0.5
    cond = torch.randn(shape, device=cuda, generator=g)
    keep = torch.ones(shape[2:], device=cuda)
    keep[2:6, 1:5, 3:8] = 0.0
    with torch.no_grad():
        sch10 = _scheduler("ddpm", 10)
        inf10 = LatentDiffusionInferer(sch10)
        smp = sch10.device_sampler(9)
        ts10 = [int(t) for t in sch10.timesteps.tolist()]
        host10 = inf10.sample(noise, None, m, conditioning=cond, mode="concat", step_noise=lambda t: smp.noise(ts10.index(int(t)), shape, cuda))
        fused10 = inf10.sample(noise, None, m, conditioning=cond, mode="concat", fused_seed=9)
        yard = rel_l2(host10, fused10)
        sch = _scheduler("ddpm", 6)
        inf = LatentDiffusionInferer(sch)
        rs = sch.repaint_sampler(known, keep, 2, 2, seed=9)
        draw = {"step": rs.noise, "known": rs.noise_known, "jump": rs.noise_jump}
        calls, undo = _count(m, "forward")
        try:
            host = inf.sample(noise, None, m, conditioning=cond, mode="concat", inpaint_latent=known, keep_mask=keep, jump_length=2,
                              n_resample=2, inpaint_noise=lambda stream, k: draw[stream](k, shape, cuda))
        finally:
            undo()
        fused = inf.sample(noise, None, m, conditioning=cond, mode="concat", fused_seed=9, inpaint_latent=known, keep_mask=keep,
                           jump_length=2, n_resample=2)
        drawn = inf.sample(noise, None, m, conditioning=cond, mode="concat", inpaint_latent=known, keep_mask=keep, jump_length=2, n_resample=2)
    err = rel_l2(host, fused)
    gate = 1e-5 if yard <= 5e-6 else 2.0 * yard
    print(f"plain 10-step DDPM host vs fused: {yard:.2e}; repaint host vs fused (10 calls): {err:.2e} (gate {gate:.2e})")
    assert len(calls) == 10 and torch.isfinite(host).all()
    assert err <= gate
    kp = (keep != 0).expand(shape)
    assert torch.equal(_bits(host)[kp], _bits(known)[kp])
    assert torch.equal(_bits(drawn)[kp], _bits(known)[kp]) and not torch.equal(drawn, host)      # torch draws: another sample, the same kept region


def test_sliding_window_inpainting(cuda):
    """A 1 x 4 x 13 x 14 x 17 latent in windows of 8: sample_sliding_window(inpaint..., fused_seed) == n_calls denoise_step_windows calls
    on the repaint sampler bit for bit, eager and replayed, and the kept region of the whole latent is the known latent's bits."""
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.sliding import WindowGrid
    m = _cond_unet(False)
    sch = _scheduler("ddpm", 3)
    inf = LatentDiffusionInferer(sch)
    g = torch.Generator(device=cuda).manual_seed(24)
    shape = (1, 4, 13, 14, 17)
    noise = torch.randn(shape, device=cuda, generator=g)
    known = torch.randn(shape, device=cuda, generator=g) * 0.5
    cond = torch.randn(shape, device=cuda, generator=g)
    keep = torch.ones(shape[2:], device=cuda)
    keep[3:11, 5:9, 6:15] = 0.0                              # the region crosses window seams
    grid = WindowGrid(shape[2:], (8, 8, 8))
    chunk = 5                                                # a ragged last chunk
    with torch.no_grad():
        rs = sch.repaint_sampler(known, keep, 1, 2, seed=3)
        assert rs.n_calls == 5 and grid.n_windows % chunk
        tbuf = torch.empty((chunk,), device=cuda)
        rs.reset(tbuf)
        x = noise.clone()
        cw = grid.gather(cond)
        for _ in range(rs.n_calls):
            m.denoise_step_windows(x, tbuf, rs, grid, cond_windows=cw, sw_batch_size=chunk)
        for graph in (False, True):
            m.enable_graph_replay(graph)
            calls, undo = _count(m, "denoise_step_windows")
            try:
                got = inf.sample_sliding_window(noise, None, m, (8, 8, 8), sw_batch_size=chunk, conditioning=cond, fused_seed=3,
                                                inpaint_latent=known, keep_mask=keep, jump_length=1, n_resample=2)
            finally:
                undo()
                m.enable_graph_replay(False)
            assert len(calls) == 5 and torch.equal(got, x), (graph, rel_l2(got, x))
        # the host-driven windowed loop (gather, forward per chunk, blend, step, merge) on the accessors' draws: the same chain up to the
        # bf16 model's sensitivity to the last bit of the blend, and the same kept region exactly
        draw = {"step": rs.noise, "known": rs.noise_known, "jump": rs.noise_jump}
        host = inf.sample_sliding_window(noise, None, m, (8, 8, 8), sw_batch_size=chunk, conditioning=cond, inpaint_latent=known, keep_mask=keep,
                                         jump_length=1, n_resample=2, inpaint_noise=lambda stream, k: draw[stream](k, shape, cuda))
    kp = (keep != 0).expand(shape)
    print(f"windowed repaint host vs fused: {rel_l2(host, x):.2e}")
    assert torch.isfinite(host).all() and torch.equal(_bits(host)[kp], _bits(known)[kp]) and not torch.equal(host[~kp], known[~kp])
    assert torch.isfinite(x).all() and torch.equal(_bits(x)[kp], _bits(known)[kp]) and not torch.equal(x[~kp], known[~kp])


def test_ensemble_keeps_the_known_region_in_every_member(cuda):
    """K = 4 members, 1, 2 and 4 at a time, on a deterministic base (DDIM eta 0, n_resample 1): one known latent bound with known_batch
    = 1 serves every member of a chunk, and the kept region of every member is the known latent's bits, so the per-voxel std there is
    exactly 0.  The spread of the members across chunkings is printed, not gated: the known-region draws of the intermediate rows are
    keyed by the chunk's seed and the element's position in the chunk, like the step noise of a stochastic sampler (the limit
    sample_ensemble documents), so members of different chunkings are different draws."""
    from ldm3d.inferer import LatentDiffusionInferer
    m = _cond_unet(True)
    sch = _scheduler("ddim", 4)
    inf = LatentDiffusionInferer(sch)
    g = torch.Generator(device=cuda).manual_seed(25)
    shape = (1, 4, 8, 8, 8)
    known = torch.randn(shape, device=cuda, generator=g) * 0.5
    cond = torch.randn(shape, device=cuda, generator=g)
    keep = torch.ones(shape[2:], device=cuda)
    keep[0:4, 2:7, 1:6] = 0.0
    kp = (keep != 0).expand((4,) + shape[1:])
    res = {}
    with torch.no_grad():
        for mb in (1, 2, 4):
            calls, undo = _count(m, "denoise_step")
            try:
                res[mb] = inf.sample_ensemble(4, shape[1:], None, m, conditioning=cond, member_batch=mb, seed=31, keep_members=4,
                                              inpaint_latent=known, keep_mask=keep)
            finally:
                undo()
            assert len(calls) == 4 * (4 // mb) and res[mb].count == 4
            mem = res[mb].members
            assert torch.equal(_bits(mem)[kp], _bits(known.expand(4, -1, -1, -1, -1))[kp]), mb
            assert float(res[mb].std[0][kp[0]].max()) == 0.0 and float(res[mb].std[0][~kp[0]].max()) > 0.0
            assert not torch.equal(mem[0], mem[1])
    for mb in (2, 4):
        print(f"member_batch {mb} vs 1: members rel-L2 {rel_l2(res[mb].members, res[1].members):.2e}, mean rel-L2 {rel_l2(res[mb].mean, res[1].mean):.2e}")


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(cuda, built_lib):
    import ctypes as C
    from ldm3d import _lib
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.schedulers import PNDMScheduler, repaint_rows
    L = built_lib
    BAD, UNSUPPORTED = -1, -2
    s = _lib.current_stream()
    ddim = _scheduler("ddim", 6)
    rows = repaint_rows(ddim, 2, 2)[1]
    coef = torch.tensor(rows, dtype=torch.float32).contiguous()
    B, Cc, dhw = 3, 2, 10
    per = Cc * dhw
    x = torch.full((B, per), NAN, device=cuda)
    eps = torch.ones((B, per), device=cuda)
    known = torch.ones((B, per), device=cuda)
    keep = torch.ones((dhw,), device=cuda)
    tbuf = torch.full((B,), -7.0, device=cuda)
    plain = ddim.device_sampler()

    def create(c, n=None, kind=1):
        h = C.c_void_p()
        return L.ldm_sampler_create_repaint(c.data_ptr(), len(c) if n is None else n, kind, 0, 1, 5, C.byref(h)), h

    def step(h, n=B * per, b=B):
        return L.ldm_sampler_step(h, eps.data_ptr(), x.data_ptr(), None, n, tbuf.data_ptr(), b, s)

    for slot, val in ((3, NAN), (9, -0.5), (11, -0.5), (12, 2.0), (12, 0.5), (10, float("inf"))):      # bad tables
        bad = coef.clone()
        bad[1, slot] = val
        assert create(bad)[0] == BAD, (slot, val)
    bad = coef.clone()
    bad[0, 11] = 0.25                                        # js without the jump flag (row 0 does not jump)
    assert create(bad)[0] == BAD and b"jump" in L.ldm_last_error()
    assert create(coef, kind=3)[0] == BAD and create(coef, n=0)[0] == BAD
    big = coef[:1].repeat(16385, 1).contiguous()
    assert create(big)[0] == UNSUPPORTED
    rc, h = create(coef)
    assert rc == 0
    try:
        assert step(h) == BAD and b"bind_known" in L.ldm_last_error()                            # unbound
        assert L.ldm_sampler_bind_known(h, known.data_ptr(), B, keep.data_ptr(), per, 7) == BAD      # per_sample no multiple of dhw
        assert L.ldm_sampler_bind_known(h, None, B, keep.data_ptr(), per, dhw) == BAD
        assert L.ldm_sampler_bind_known(h, known.data_ptr(), 0, keep.data_ptr(), per, dhw) == BAD
        assert step(h) == BAD                                                                    # still unbound
        assert L.ldm_sampler_bind_known(h, known.data_ptr(), 2, keep.data_ptr(), per, dhw) == 0
        assert step(h) == BAD and b"known_batch" in L.ldm_last_error()                           # known_batch outside {1, B}
        assert L.ldm_sampler_bind_known(h, known.data_ptr(), B, keep.data_ptr(), per, dhw) == 0
        assert step(h, n=B * per - 1) == BAD and step(h, n=(B - 1) * per) == BAD                 # n != B * per_sample
        assert L.ldm_sampler_start(h, 0, known.data_ptr(), B, eps.data_ptr(), x.data_ptr(), B, per, 0, 0, s) == BAD      # no warm start
        assert L.ldm_sampler_bind_state(h, x.data_ptr(), x.numel() * 4, B * per) == BAD
        assert L.ldm_sampler_repaint_noise(h, 2, 0, x.data_ptr(), x.numel(), s) == BAD
        assert L.ldm_sampler_repaint_noise(plain._h, 0, 0, x.data_ptr(), x.numel(), s) == BAD
        assert L.ldm_sampler_bind_known(plain._h, known.data_ptr(), B, keep.data_ptr(), per, dhw) == BAD
        c4 = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)
        args = (known.data_ptr(), B, keep.data_ptr())
        assert L.ldm_repaint_merge(eps.data_ptr(), *args, None, eps.data_ptr(), x.data_ptr(), B, per, dhw, c4, 1, s) == BAD      # ks != 0, no z_known
        assert L.ldm_repaint_merge(eps.data_ptr(), *args, eps.data_ptr(), None, x.data_ptr(), B, per, dhw, c4, 1, s) == BAD      # a jump, no z_jump
        assert L.ldm_repaint_merge(eps.data_ptr(), *args, eps.data_ptr(), None, x.data_ptr(), B, per, dhw, c4, 0, s) == BAD      # js without a jump
        assert L.ldm_repaint_merge(eps.data_ptr(), known.data_ptr(), 2, keep.data_ptr(), eps.data_ptr(), eps.data_ptr(), x.data_ptr(), B, per,
                                   dhw, c4, 1, s) == BAD
        assert L.ldm_repaint_merge(eps.data_ptr(), *args, eps.data_ptr(), eps.data_ptr(), x.data_ptr(), B, per, 7, c4, 1, s) == BAD
        torch.cuda.synchronize()
        assert bool(torch.isnan(x).all()) and tbuf.tolist() == [-7.0] * B                        # nothing was written
        x.fill_(0.25)
        assert step(h) == 0                                                                      # what is allowed still runs
        torch.cuda.synchronize()
        assert torch.isfinite(x).all() and tbuf.tolist() == [rows[1][5]] * B
    finally:
        L.ldm_sampler_destroy(h)
    pndm = PNDMScheduler(skip_prk_steps=True, **cfgs.SCHED)
    pndm.set_timesteps(10)
    z = torch.zeros((1, 4, 8, 8, 8), device=cuda)
    k3 = torch.ones((8, 8, 8), device=cuda)
    with pytest.raises(NotImplementedError):
        pndm.repaint_sampler(z, k3)
    with pytest.raises(NotImplementedError):
        LatentDiffusionInferer(pndm).sample(z, None, None, fused_seed=1, inpaint_latent=z, keep_mask=k3)
    inf = LatentDiffusionInferer(ddim)
    with pytest.raises(NotImplementedError):                 # the warm-start arguments
        inf.sample(z, None, None, fused_seed=1, inpaint_latent=z, keep_mask=k3, init_latent=z, start_step=2)
    with pytest.raises(NotImplementedError):
        inf.sample_sliding_window(z, None, None, (8, 8, 8), fused_seed=1, inpaint_latent=z, keep_mask=k3, init_latent=z, start_step=2)
    with pytest.raises(NotImplementedError):
        inf.sample_ensemble(2, (4, 8, 8, 8), None, None, inpaint_latent=z, keep_mask=k3, init_latent=z, start_step=2)
    with pytest.raises(NotImplementedError):
        ddim.repaint_sampler(z, k3).start(z, 0, 1)
    soft = k3.clone()
    soft[0, 0, 0] = 0.5
    with pytest.raises(ValueError):                          # a non-binary mask
        inf.sample(z, None, None, fused_seed=1, inpaint_latent=z, keep_mask=soft)
    with pytest.raises(ValueError):
        ddim.repaint_sampler(z, soft)
    with pytest.raises(ValueError):
        inf.sample(z, None, None, fused_seed=1, inpaint_latent=z)


def test_table_at_the_row_cap(cuda, built_lib):
    """a table of LDM_REPAINT_MAX_ROWS rows: the sampler is created and one denoising step builds the time-embedding table of as many
    rows and steps (the cap the header documents is one the step entries serve)"""
    import ctypes as C
    from ldm3d import _lib
    from ldm3d.schedulers import REPAINT_MAX_ROWS, repaint_rows
    L = built_lib
    m = _cond_unet(True)
    rows = repaint_rows(_scheduler("ddpm", 1000), 1, 2)[1]
    coef = torch.tensor((rows * (REPAINT_MAX_ROWS // len(rows) + 1))[:REPAINT_MAX_ROWS], dtype=torch.float32).contiguous()
    assert coef.shape == (16384, 16)
    shape = (1, 4, 8, 8, 8)
    g = torch.Generator(device=cuda).manual_seed(26)
    x = torch.randn(shape, device=cuda, generator=g)
    known, cond = torch.randn(shape, device=cuda, generator=g), torch.randn(shape, device=cuda, generator=g)
    keep = _mask(shape[2:], cuda, 4)

    class Handle:                                            # what denoise_step asks of a sampler
        chain = -1

        def ensure_state(self, n, device):
            pass

    smp = Handle()
    smp._h = C.c_void_p()
    assert L.ldm_sampler_create_repaint(coef.data_ptr(), REPAINT_MAX_ROWS, 0, 0, 1, 7, C.byref(smp._h)) == 0
    try:
        assert L.ldm_sampler_bind_known(smp._h, known.data_ptr(), 1, keep.data_ptr(), 4 * 512, 512) == 0
        tbuf = torch.full((1,), NAN, device=cuda)
        assert L.ldm_sampler_seek(smp._h, REPAINT_MAX_ROWS - 2, tbuf.data_ptr(), 1, _lib.current_stream()) == 0
        assert tbuf.tolist() == [float(coef[-2, 5])]
        with torch.no_grad():
            m.denoise_step(x, tbuf, smp, cond=cond)
        torch.cuda.synchronize()
        assert torch.isfinite(x).all() and tbuf.tolist() == [float(coef[-1, 5])]
    finally:
        L.ldm_sampler_destroy(smp._h)


# ---- the command line ------------------------------------------------------------------------------------------------------------
def _run_cli(tmp_path, flags):
    from ldm3d.data import write_synthetic_pairs
    pair = write_synthetic_pairs(str(tmp_path / "pairs"), 1, (100, 96, 120))[0]
    env = {"npz_dir": str(tmp_path / "pairs"), "model_dir": str(tmp_path / "ckpt"), "output_dir": str(tmp_path / "out"),
           "tfevent_path": str(tmp_path / "tfevent"), "resume_ckpt": False, "seed": 0}
    env_file = str(tmp_path / "environment.json")
    with open(env_file, "w") as fh:
        json.dump(env, fh)
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-e", env_file, "-c", os.path.join(ROOT, "config", "config_synthetic_train.json"),
           "--random-init", "--steps", "4", "--condition", pair, "--inpaint", pair] + flags
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return pair, tmp_path / "out"


def test_inference_cli_inpaint(tmp_path):
    """--inpaint with a box: the volume and one inpaint.jsonl record with the chain's call count and the kept fractions; with
    --inpaint-paste the written volume is the original image outside the box, bit for bit"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import inference
    pair, out = _run_cli(tmp_path, ["--regenerate-box", "10:40,20:60,30:50", "--jump-length", "2", "--resample", "2", "--inpaint-paste"])
    vols = sorted(out.glob("synimg_*.nii"))
    assert len(vols) == 1
    data = np.fromfile(vols[0], dtype=np.float32, offset=352)
    assert data.size == 96 ** 3 and np.isfinite(data).all()
    recs = [json.loads(l) for l in open(out / "inpaint.jsonl")]
    assert len(recs) == 1
    rec = recs[0]
    assert rec["file"] == vols[0].name and rec["n_calls"] == 6 == ref.n_calls(4, 2, 2) and rec["jump_length"] == 2 and rec["n_resample"] == 2
    assert abs(rec["kept_image"] - (1.0 - 30 * 40 * 20 / 96 ** 3)) <= 1e-6
    # the box 10:40, 20:60, 30:50 touches the latent cells 2:10, 5:15, 7:13 (factor 4)
    assert abs(rec["kept_latent"] - (1.0 - 8 * 10 * 6 / 24 ** 3)) <= 1e-6 and rec["paste"] is True
    orig = inference.prepared_patch(pair, [96, 96, 96], 4, high_count=True)
    vol = data.reshape(96, 96, 96, order="F")                # the NIfTI writer stores x fastest
    outside = np.ones((96, 96, 96), dtype=bool)
    outside[10:40, 20:60, 30:50] = False
    assert np.array_equal(vol[outside], orig.astype(np.float32)[outside]) and not np.array_equal(vol[~outside], orig.astype(np.float32)[~outside])


@pytest.mark.parametrize("flags", [["--sliding-window", "--cfg", "2.0", "--metrics"], ["--ensemble", "2", "--sampler", "ddim"]],
                         ids=["whole-scan-guided-scored", "ensemble"])
def test_inference_cli_inpaint_composes(tmp_path, flags):
    """the flags it is valid with: the whole scan by sliding windows, guided and scored; an ensemble whose members keep the same region.
    The inpainting fields land in the run's own records."""
    _, out = _run_cli(tmp_path, ["--regenerate-box", "10:40,20:60,30:50", "--resample", "2"] + flags)
    want = {"n_calls": 7, "jump_length": 1, "n_resample": 2}
    inp = [json.loads(l) for l in open(out / "inpaint.jsonl")]
    assert len(inp) == 1
    if "--ensemble" in flags:
        rec = [json.loads(l) for l in open(out / "ensemble.jsonl")][0]
        assert rec["members"] == 2 and rec["max_std"] > 0
    else:
        rec = [json.loads(l) for l in open(out / "metrics.jsonl")][0]
        assert rec["shape"] == [100, 96, 120] and inp[0]["file"] == rec["file"]
        assert abs(rec["kept_image"] - (1.0 - 30 * 40 * 20 / (100 * 96 * 120))) <= 1e-6
    assert {k: rec[k] for k in want} == want and {k: inp[0][k] for k in want} == want


def test_inference_cli_refuses(tmp_path, monkeypatch, capsys):
    """the refused flag combinations exit non-zero with a message (argparse errors, raised before any device work: parsed in process)"""
    from test_repaint_cpu import REFUSED, parse
    for argv in REFUSED:
        with pytest.raises(SystemExit) as e:
            parse(argv, tmp_path, monkeypatch)
        assert e.value.code != 0, argv
        assert "error" in capsys.readouterr().err, argv
