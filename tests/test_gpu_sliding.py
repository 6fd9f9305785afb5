"""Sliding-window latent sampling (-m gpu): window gather / blend kernels against torch, the fused windowed step against the
library's own pieces bit for bit, the one-window case against denoise_step, chunking, the inferer, the graph cache and the
whole-scan inference.py path."""
import gc
import json
import os
import struct
import subprocess
import sys

import pytest
import torch

import cfgs
from util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _unet(cfg, cuda, seed=1):
    from ldm3d.networks import DiffusionModelUNet
    from oracle import unet as ou
    m = DiffusionModelUNet(**cfg)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfg), seed))
    return m.to(cuda).eval()


def _slice_gather(grid, vol):
    """[1, C, D, H, W] -> [nW, C, r...] by torch slicing"""
    rd, rh, rw = grid.roi
    return torch.stack([vol[0, :, a:a + rd, b:b + rh, c:c + rw] for a, b, c in grid.starts]).contiguous()


def _blend64(grid, win, weights=None):
    """Independent float64 blend: full 3-D maps accumulated by slicing, then divided (win: [nW, C, r...])."""
    from ldm3d.sliding import axis_profile
    rd, rh, rw = grid.roi
    if weights is None:
        p = [torch.from_numpy(axis_profile(r, grid.mode, grid.sigma_scale)) for r in grid.roi]
        weights = p[0][:, None, None] * p[1][None, :, None] * p[2][None, None, :]
    w = win.detach().double().cpu()
    num = torch.zeros((w.shape[1],) + grid.shape, dtype=torch.float64)
    den = torch.zeros(grid.shape, dtype=torch.float64)
    for k, (a, b, c) in enumerate(grid.starts):
        num[:, a:a + rd, b:b + rh, c:c + rw] += weights * w[k]
        den[a:a + rd, b:b + rh, c:c + rw] += weights
    return (num / den)[None]


def test_gather_equals_torch_slicing(cuda):
    from ldm3d.sliding import WindowGrid
    g = torch.Generator(device=cuda).manual_seed(0)
    vol = torch.randn((1, 4, 13, 22, 17), device=cuda, generator=g)
    for roi, ov in ((8, 0.25), ((8, 12, 4), 0.5), (16, 0.0)):
        grid = WindowGrid(vol.shape[2:], roi, overlap=ov)
        out = torch.full((grid.n_windows, 4) + grid.roi, float("nan"), device=cuda)
        grid.gather(vol, out=out)
        assert torch.equal(out, _slice_gather(grid, vol)), roi


@pytest.mark.parametrize("mode", ["gaussian", "constant"])
@pytest.mark.parametrize("overlap", [0.0, 0.25, 0.5])
def test_blend_matches_float64_reference(cuda, mode, overlap):
    from ldm3d.sliding import WindowGrid
    grid = WindowGrid((13, 22, 17), 8, overlap=overlap, mode=mode)
    g = torch.Generator(device=cuda).manual_seed(3)
    win = torch.randn((grid.n_windows, 4) + grid.roi, device=cuda, generator=g)
    ref = _blend64(grid, win)
    out = grid.blend(win)
    assert torch.isfinite(out).all()          # blend() allocates with torch.empty; NaN-fill a persistent target for the launch check
    tgt = torch.full_like(out, float("nan"))
    from ldm3d import _lib
    _lib.check(_lib.lib().ldm_window_blend(grid.handle(), win.data_ptr(), tgt.data_ptr(), 4, _lib.current_stream()))
    assert torch.equal(tgt, out)                                    # a second launch is bit-identical
    err, gate = rel_l2(out, ref), 1e-6
    amax = float((out.double().cpu() - ref).abs().max())
    assert err <= gate and amax <= 2e-6, (err, amax)
    # negative controls: unnormalised weights, or a grid without its flush last window, land far outside the gate
    from ldm3d.sliding import axis_profile
    p = [torch.from_numpy(axis_profile(r, mode, grid.sigma_scale)) for r in grid.roi]
    w3 = p[0][:, None, None] * p[1][None, :, None] * p[2][None, None, :]
    w = win.double().cpu()
    unnorm = torch.zeros_like(ref)
    for k, (a, b, c) in enumerate(grid.starts):
        unnorm[0, :, a:a + 8, b:b + 8, c:c + 8] += w3 * w[k]
    assert rel_l2(unnorm, ref) > 10 * gate
    num, den = torch.zeros_like(ref), torch.zeros(grid.shape, dtype=torch.float64)
    for k, (a, b, c) in enumerate(grid.starts):
        if c != grid.axis_starts[2][-1]:                          # the grid without its flush last windows along W
            num[0, :, a:a + 8, b:b + 8, c:c + 8] += w3 * w[k]
            den[a:a + 8, b:b + 8, c:c + 8] += w3
    trunc = num / den.clamp_min(1e-300)
    assert rel_l2(trunc, ref) > 10 * gate


def _composed(m, sch, seed, x0, cond, grid, chunk, nsteps):
    """The library's own pieces: slicing gather -> eager forward per chunk -> grid.blend -> sampler.step."""
    smp = sch.device_sampler(seed)
    x = x0.clone()
    tbuf = torch.empty((chunk,), device=x.device)
    smp.reset(tbuf)
    cw = _slice_gather(grid, cond) if cond is not None else None
    nw = grid.n_windows
    ts = sch.timesteps.tolist()
    for k in range(nsteps):
        assert tbuf.tolist() == [float(ts[k])] * chunk
        xw = _slice_gather(grid, x)
        eps_w = torch.empty((nw, m.out_channels) + grid.roi, device=x.device)
        for b0 in range(0, nw, chunk):
            nb = min(chunk, nw - b0)
            kw = {} if cw is None else dict(cond=cw[b0:b0 + nb])
            eps_w[b0:b0 + nb] = m(x=xw[b0:b0 + nb], timesteps=tbuf[:nb], **kw)
        smp.step(grid.blend(eps_w), x, tbuf)
    return x


def _fused(m, sch, seed, x0, cond, grid, chunk, nsteps, graph):
    m.enable_graph_replay(graph)
    smp = sch.device_sampler(seed)
    x = x0.clone()
    tbuf = torch.empty((chunk,), device=x.device)
    smp.reset(tbuf)
    cw = grid.gather(cond) if cond is not None else None
    ts = sch.timesteps.tolist()
    for k in range(nsteps):
        assert tbuf.tolist() == [float(ts[k])] * chunk
        m.denoise_step_windows(x, tbuf, smp, grid, cond_windows=cw, sw_batch_size=chunk)
    assert tbuf.tolist() == [float(ts[min(nsteps, len(ts) - 1)])] * chunk
    m.enable_graph_replay(False)
    return x


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_fused_windowed_step_equals_its_pieces(cuda, kind, precision):
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler
    from ldm3d.sliding import WindowGrid
    m = _unet(cfgs.UNET_TINY_COND, cuda)
    m.set_precision(precision)
    sch = DDPMScheduler(**cfgs.SCHED) if kind == "ddpm" else DDIMScheduler(**cfgs.SCHED)
    if kind == "ddim":
        sch.set_timesteps(10)
    g = torch.Generator(device=cuda).manual_seed(5)
    x0 = torch.randn((1, 4, 13, 14, 17), device=cuda, generator=g)
    cond = torch.randn((1, 4, 13, 14, 17), device=cuda, generator=g)
    grid = WindowGrid(x0.shape[2:], 8)
    assert grid.n_windows == 12
    with torch.no_grad():
        for chunk in (12, 5):
            ref = _composed(m, sch, 17, x0, cond, grid, chunk, 6)
            for graph in (False, True):
                got = _fused(m, sch, 17, x0, cond, grid, chunk, 6, graph)
                assert torch.equal(got, ref), (kind, precision, chunk, graph, rel_l2(got, ref))
            assert torch.isfinite(ref).all() and not torch.equal(ref, x0)


def test_sample_prediction_windowed_step_and_the_end_of_the_chain(cuda):
    """The smallest windowed step (two windows of 8^3 over 8 x 8 x 12, chunks of 2 and 1) for a stochastic DDPM and a DDIM sampler with
    prediction_type "sample": three fused calls == gather -> forward per chunk -> blend -> scheduler.step bit for bit (the DDPM noise is
    the device sampler's own draw), and beyond the end of a 3-step chain nothing moves: x, its windows and the timestep buffer."""
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler
    from ldm3d.sliding import WindowGrid
    m = _unet(cfgs.UNET_TINY, cuda)
    g = torch.Generator(device=cuda).manual_seed(6)
    xT = torch.randn((1, 4, 8, 8, 12), device=cuda, generator=g)
    grid = WindowGrid(xT.shape[2:], 8)
    assert grid.n_windows == 2

    def window_buffer():
        bufs = [v["xw"] for k, v in m._ws.items() if k[0] == "win"]
        assert len(bufs) == 1
        return bufs[0]

    def fused(sch, chunk, graph, calls):
        m.enable_graph_replay(graph)
        smp = sch.device_sampler(17)
        x = xT.clone()
        tbuf = torch.empty((chunk,), device=cuda)
        smp.reset(tbuf)
        for _ in range(calls):
            m.denoise_step_windows(x, tbuf, smp, grid, sw_batch_size=chunk)
        m.enable_graph_replay(False)
        return x, tbuf
    with torch.no_grad():
        for kind in ("ddpm", "ddim"):
            sch = DDPMScheduler(**cfgs.SCHED, prediction_type="sample") if kind == "ddpm" else DDIMScheduler(**cfgs.SCHED, prediction_type="sample")
            if kind == "ddim":
                sch.set_timesteps(10)
            ts = sch.timesteps.tolist()
            noise_src = sch.device_sampler(17)
            for chunk in (2, 1):
                ref = xT.clone()
                for k in range(3):
                    xw = grid.gather(ref)
                    out_w = torch.empty((2, 4) + grid.roi, device=cuda)
                    for b0 in range(0, 2, chunk):
                        out_w[b0:b0 + chunk] = m(x=xw[b0:b0 + chunk], timesteps=torch.full((chunk,), float(ts[k]), device=cuda))
                    noise = noise_src.noise(k, ref.shape, cuda) if kind == "ddpm" else None
                    ref, _ = sch.step(grid.blend(out_w), ts[k], ref, noise=noise)
                assert torch.isfinite(ref).all() and not torch.equal(ref, xT)
                for graph in (False, True):
                    x, _ = fused(sch, chunk, graph, 3)
                    assert torch.equal(x, ref), (kind, chunk, graph, rel_l2(x, ref))
        sch = DDIMScheduler(**cfgs.SCHED, prediction_type="sample")
        sch.set_timesteps(3)
        last = float(sch.timesteps.tolist()[-1])
        for chunk in (2, 1):
            for graph in (False, True):
                end, tbuf = fused(sch, chunk, graph, 3)
                assert not torch.equal(end, xT) and tbuf.tolist() == [last] * chunk
                x, tbuf = fused(sch, chunk, graph, 5)
                assert torch.equal(x, end), (chunk, graph)
                assert torch.equal(window_buffer(), grid.gather(x)), (chunk, graph)
                assert tbuf.tolist() == [last] * chunk, (chunk, graph)


def test_one_window_equals_denoise_step(cuda):
    from ldm3d.schedulers import DDPMScheduler
    from ldm3d.sliding import WindowGrid
    m = _unet(cfgs.UNET_TINY_COND, cuda)
    sch = DDPMScheduler(**cfgs.SCHED)
    g = torch.Generator(device=cuda).manual_seed(2)
    x0 = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g)
    cond = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g)
    grid = WindowGrid((8, 8, 8), 8)
    assert grid.n_windows == 1
    with torch.no_grad():
        for graph in (False, True):
            m.enable_graph_replay(graph)
            a = sch.device_sampler(seed=7)
            xa, ta = x0.clone(), torch.empty((1,), device=cuda)
            a.reset(ta)
            for _ in range(5):
                m.denoise_step(xa, ta, a, cond=cond)
            b = sch.device_sampler(seed=7)
            xb, tb = x0.clone(), torch.empty((1,), device=cuda)
            b.reset(tb)
            cw = grid.gather(cond)
            for _ in range(5):
                m.denoise_step_windows(xb, tb, b, grid, cond_windows=cw)
            assert torch.equal(xa, xb) and torch.equal(ta, tb), graph
        m.enable_graph_replay(False)


def test_chunking_changes_fp32_results_only_within_batch_noise(cuda):
    """The same chain with 5-window chunks (5 + 5 + 2) and with all 12 windows in one call: the fp32 plans at another batch differ
    by summation order only (the bound of test_unet_brats_latent_batch_independence).  DDPM steps: a random-weight UNet under
    DDIM's large steps multiplies any last-bit difference from step to step."""
    from ldm3d.schedulers import DDPMScheduler
    from ldm3d.sliding import WindowGrid
    m = _unet(cfgs.UNET_TINY_COND, cuda)
    m.set_precision("fp32")
    sch = DDPMScheduler(**cfgs.SCHED)
    g = torch.Generator(device=cuda).manual_seed(8)
    x0 = torch.randn((1, 4, 13, 14, 17), device=cuda, generator=g)
    cond = torch.randn((1, 4, 13, 14, 17), device=cuda, generator=g)
    grid = WindowGrid(x0.shape[2:], 8)
    with torch.no_grad():
        a = _fused(m, sch, 4, x0, cond, grid, 12, 6, False)
        b = _fused(m, sch, 4, x0, cond, grid, 5, 6, False)
    assert rel_l2(b, a) <= 5e-5


def test_sample_sliding_window_host_loop_equals_fused(cuda):
    """Host-driven loop (gather -> forward per chunk -> blend -> DDIMScheduler.step) vs the device sampler: the same algorithm; the
    two scheduler kernels may round the step differently in the last bit.  The output projection is scaled by 0.1 so that the
    random-weight UNet does not multiply such a bit from one DDIM step to the next (a trained eps-predictor is tame there)."""
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.schedulers import DDIMScheduler
    m = _unet(cfgs.UNET_TINY_COND, cuda)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith("out.2.conv."):
                p.mul_(0.1)
    m.mark_weights_dirty()
    m.set_precision("fp32")
    sch = DDIMScheduler(**cfgs.SCHED)
    sch.set_timesteps(5)
    inf = LatentDiffusionInferer(sch)
    g = torch.Generator(device=cuda).manual_seed(9)
    noise = torch.randn((1, 4, 13, 14, 17), device=cuda, generator=g)
    cond = torch.randn((1, 4, 13, 14, 17), device=cuda, generator=g)
    with torch.no_grad():
        host = inf.sample_sliding_window(noise, None, m, (8, 8, 8), sw_batch_size=5, conditioning=cond)
        fused = inf.sample_sliding_window(noise, None, m, (8, 8, 8), sw_batch_size=5, conditioning=cond, fused_seed=3)
    assert tuple(fused.shape) == (1, 4, 13, 14, 17) and torch.isfinite(fused).all()
    assert rel_l2(fused, host) <= 1e-5                      # DDIM (eta = 0) draws no noise


def test_graph_replay_never_reuses_a_graph_recorded_for_a_destroyed_grid(cuda):
    """A new WindowGrid may get a freed grid's address; the captured blend-step bakes the grid's tables in, so the cache keys on
    the grid's never-reused id: a second grid (another overlap, same window count) must equal its own eager run."""
    from ldm3d.schedulers import DDPMScheduler
    from ldm3d.sliding import WindowGrid
    m = _unet(cfgs.UNET_TINY_COND, cuda)
    sch = DDPMScheduler(**dict(cfgs.SCHED, num_train_timesteps=6))
    g = torch.Generator(device=cuda).manual_seed(4)
    x0 = torch.randn((1, 4, 13, 14, 17), device=cuda, generator=g)
    cond = torch.randn((1, 4, 13, 14, 17), device=cuda, generator=g)

    def chain(overlap, mode, graph):
        grid = WindowGrid(x0.shape[2:], 8, overlap=overlap, mode=mode)
        assert grid.n_windows == 12
        with torch.no_grad():
            out = _fused(m, sch, 21, x0, cond, grid, 12, 6, graph)
        del grid
        gc.collect()
        return out
    ea, eb = chain(0.25, "gaussian", False), chain(0.25, "constant", False)
    assert not torch.equal(ea, eb)
    ga, gb, ga2 = chain(0.25, "gaussian", True), chain(0.25, "constant", True), chain(0.25, "gaussian", True)
    assert torch.equal(ga, ea) and torch.equal(gb, eb) and torch.equal(ga2, ea)


def test_window_kernels_use_no_scratch(built_lib):
    csrc = os.path.join(ROOT, "3d-latent-diffusion-model_amd", "csrc")
    res = os.path.join(csrc, "resource_usage.txt")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hip"))]
    if not os.path.exists(res) or os.path.getmtime(res) < max(os.path.getmtime(f) for f in srcs):
        subprocess.run(["make", "-C", csrc, "asm"], check=True, capture_output=True, timeout=900)
    text = open(res).read()
    # every instantiation of the blend-step: <prediction type, family>, family 0 DDPM / DDIM, 1 PNDM (epsilon, v), 2 flow
    steps = [f"_Z24window_blend_step_kernelILi{p}ELi{f}EE" for p, f in ((0, 0), (1, 0), (2, 0), (0, 1), (2, 1), (0, 2))]
    assert text.count("Function Name: _Z24window_blend_step_kernel") == len(steps)
    for name in ["_Z20window_gather_kernel", "_Z19window_blend_kernel", "_Z24window_blend_step_kernel"] + steps:
        i = text.index("Function Name: " + name)
        block = text[i:i + 2000]
        assert "ScratchSize [bytes/lane]: 0 " in block and "VGPRs Spill: 0 " in block, block


def _nifti_dims(path):
    with open(path, "rb") as fh:
        hdr = fh.read(348)
    return struct.unpack("<8h", hdr[40:56])


def test_inference_sliding_window_writes_the_whole_scan(tmp_path):
    import numpy as np
    from ldm3d.data import write_synthetic_pairs
    pair = write_synthetic_pairs(str(tmp_path / "pairs"), 1, (130, 100, 170))[0]
    env = {"npz_dir": str(tmp_path / "pairs"), "model_dir": str(tmp_path / "ckpt"), "output_dir": str(tmp_path / "out"),
           "tfevent_path": str(tmp_path / "tfevent"), "resume_ckpt": False, "seed": 0}
    env_file = str(tmp_path / "environment.json")
    with open(env_file, "w") as fh:
        json.dump(env, fh)
    base = [sys.executable, os.path.join(ROOT, "inference.py"), "-e", env_file, "-c", os.path.join(ROOT, "config", "config_synthetic_train.json"),
            "-n", "1", "--random-init", "--steps", "3", "--condition", pair]
    r = subprocess.run(base + ["--sliding-window"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    vols = sorted((tmp_path / "out").glob("*.nii"))
    assert len(vols) == 1
    dim = _nifti_dims(vols[0])
    assert dim[1:4] == (130, 100, 170), dim
    data = np.fromfile(vols[0], dtype=np.float32, offset=352)
    assert data.size == 130 * 100 * 170 and np.isfinite(data).all()
    assert "windows of (24, 24, 24)" in r.stdout + r.stderr
    bad = subprocess.run(base + ["--sliding-window", "--batch", "2"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--batch" in bad.stderr
    for v in vols:
        v.unlink()
    r = subprocess.run(base, cwd=ROOT, capture_output=True, text=True, timeout=600)      # without the flag: the central patch
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    vols = sorted((tmp_path / "out").glob("*.nii"))
    assert len(vols) == 1 and _nifti_dims(vols[0])[1:4] == (96, 96, 96)
