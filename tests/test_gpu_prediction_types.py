"""prediction_type "sample" / "v_prediction" on the GPU (-m gpu): the step kernels against a float64 restatement of MONAI's
formulas, the fused noising + target kernel, a perfect-model check that the three types give the same chains, the device sampler
(eager, denoise_step graphs, sliding-window blend-step) against the host-driven step bit for bit, the training target and the CLI."""
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
NEW_TYPES = ("sample", "v_prediction")


def _sched(kind, pred, nsteps=20, **kw):
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler
    if kind == "ddpm":
        return DDPMScheduler(**cfgs.SCHED, prediction_type=pred, **kw)
    s = DDIMScheduler(**cfgs.SCHED, prediction_type=pred, **kw)
    s.set_timesteps(nsteps)
    return s


def _unet(cfg, cuda, seed=1):
    from ldm3d.networks import DiffusionModelUNet
    from oracle import unet as ou
    m = DiffusionModelUNet(**cfg)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfg), seed))
    return m.to(cuda).eval()


def _step64(kind, pred, row, m, x, z, clip):
    """MONAI's step (monai/networks/schedulers/ddpm.py, ddim.py; restated) in float64 on the fp32 coefficients of ``row``."""
    inv_sqrt_a, sqrt_b, c0, c1, sigma, _, sqrt_a, _ = row
    m, x = m.double().cpu(), x.double().cpu()
    if pred == "epsilon":
        x0, eps = (x - sqrt_b * m) * inv_sqrt_a, m
    elif pred == "sample":
        x0, eps = m, (x - sqrt_a * m) / sqrt_b
    else:
        x0, eps = sqrt_a * x - sqrt_b * m, sqrt_a * m + sqrt_b * x
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    prev = c0 * x0 + c1 * (x if kind == "ddpm" else eps)
    if z is not None and sigma != 0.0:
        prev = prev + sigma * z.double().cpu()
    return prev, x0


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("pred", NEW_TYPES)
@pytest.mark.parametrize("kind,eta", [("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.6)])
def test_step_matches_float64(cuda, kind, eta, pred, clip):
    sch = _sched(kind, pred, clip_sample=clip)
    ts = [int(t) for t in sch.timesteps.tolist()]
    g = torch.Generator(device=cuda).manual_seed(3)
    for t in (ts[0], ts[len(ts) // 2], ts[-2], ts[-1]):
        x = torch.randn((2, 4, 7, 8, 9), device=cuda, generator=g)
        m = torch.randn((2, 4, 7, 8, 9), device=cuda, generator=g)
        z = torch.randn((2, 4, 7, 8, 9), device=cuda, generator=g)
        if kind == "ddpm":
            prev, x0 = sch.step(m, t, x, noise=z)
            zz = z if t > 0 else None
        else:
            prev, x0 = sch.step(m, t, x, eta=eta, noise=z)
            zz = z if eta > 0 else None
        want, want_x0 = _step64(kind, pred, sch._row(t, eta), m, x, zz, clip)
        assert rel_l2(prev, want) <= 1e-6 and rel_l2(x0, want_x0) <= 1e-6, (t, rel_l2(prev, want), rel_l2(x0, want_x0))
        if clip:
            assert float(x0.abs().max()) <= 1.0


def test_unknown_type_is_refused_by_the_c_entries(cuda):
    import ctypes as C
    from ldm3d import _lib
    L = _lib.lib()
    x = torch.zeros(8, device=cuda)
    bad_arg = -1                                                       # LDM_ERR_BAD_ARG, include/ldm3d.h
    row = (C.c_float * 8)(1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0)

    def step(kind, pred):
        return L.ldm_scheduler_step(x.data_ptr(), x.data_ptr(), None, x.data_ptr(), None, 8, kind, pred, row, 1, _lib.current_stream())
    for pred in (3, -1):
        assert step(0, pred) == bad_arg
        assert L.ldm_add_noise_target(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 1, 8, pred,
                                      _lib.current_stream()) == bad_arg
        h = C.c_void_p()
        coef = torch.zeros((2, 8))
        assert L.ldm_sampler_create(coef.data_ptr(), 2, 0, pred, 1, 0, C.byref(h)) == bad_arg and not h.value
    for kind in (2, -1):
        assert step(kind, 0) == bad_arg


def test_get_velocity_and_fused_noise_target_match_float64(cuda):
    from ldm3d.schedulers import DDPMScheduler
    g = torch.Generator(device=cuda).manual_seed(4)
    x0 = torch.randn((3, 4, 6, 6, 6), device=cuda, generator=g)
    eps = torch.randn((3, 4, 6, 6, 6), device=cuda, generator=g)
    t = torch.tensor([0, 500, 999], device=cuda)
    ref = DDPMScheduler(**cfgs.SCHED)
    sa = ref._sqrt_ac.double()[t.cpu()].reshape(-1, 1, 1, 1, 1)
    sb = ref._sqrt_1mac.double()[t.cpu()].reshape(-1, 1, 1, 1, 1)
    x64, e64 = x0.double().cpu(), eps.double().cpu()
    noisy64, v64 = sa * x64 + sb * e64, sa * e64 - sb * x64
    assert rel_l2(ref.get_velocity(x0, eps, t), v64) <= 1e-6
    for pred, target64 in (("sample", x64), ("v_prediction", v64)):
        sch = DDPMScheduler(**cfgs.SCHED, prediction_type=pred)
        noisy, target = sch.add_noise_and_target(x0, eps, t)
        assert rel_l2(noisy, noisy64) <= 1e-6 and rel_l2(target, target64) <= 1e-6, pred
        assert torch.equal(noisy, sch.add_noise(x0, eps, t)) or rel_l2(noisy, sch.add_noise(x0, eps, t)) <= 1e-7
    noisy, target = ref.add_noise_and_target(x0, eps, t)     # epsilon: the reference's add_noise, the noise itself as the target
    assert target is eps and torch.equal(noisy, ref.add_noise(x0, eps, t))


def _perfect_chain(kind, pred, clip, x0_true, x_T, zs, feed=None):
    """Sample with a model that returns the exact target of ``feed`` (default: the scheduler's own type) for x0_true from the current x."""
    sch = _sched(kind, pred, nsteps=10, clip_sample=clip)
    feed = feed or pred
    ac = sch.alphas_cumprod.double().to(x_T.device)
    ts = [int(t) for t in sch.timesteps.tolist()]
    if kind == "ddpm":
        ts = [t for t in ts if t < 200]                       # the tail of the chain: 200 steps from t = 199
    x = x_T.clone()
    xt = x0_true.double()
    traj = []
    for k, t in enumerate(ts):
        a = ac[t]
        eps = (x.double() - a.sqrt() * xt) / (1 - a).sqrt()
        m = {"epsilon": eps, "sample": xt, "v_prediction": a.sqrt() * eps - (1 - a).sqrt() * xt}[feed].float()
        if kind == "ddpm":
            x, x0 = sch.step(m, t, x, noise=zs[k] if t > 0 else None)
        else:
            x, x0 = sch.step(m, t, x)
        traj.append((x, x0))
    return traj


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
def test_perfect_model_gives_the_same_chain_for_every_type(cuda, kind, clip):
    """No MONAI needed: a model that knows x0 exactly predicts eps, x0 or v exactly; the three conversions must then produce the same
    trajectory up to fp32 rounding (clip on: x0_true reaches beyond [-1, 1], so the clip is active).  Negative control: v fed to
    the epsilon instantiation is far off."""
    g = torch.Generator(device=cuda).manual_seed(6)
    x0_true = 1.3 * torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g)
    x_T = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g)
    zs = [torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g) for _ in range(200)]
    ref = _perfect_chain(kind, "epsilon", clip, x0_true, x_T, zs)
    for pred in NEW_TYPES:
        got = _perfect_chain(kind, pred, clip, x0_true, x_T, zs)
        err = max(max(rel_l2(g[0], r[0]), rel_l2(g[1], r[1])) for g, r in zip(got, ref))     # x_{t-1} and x0_hat, every step
        assert err <= 5e-5, (pred, err)
    # the perfect model re-derives its output from the current x, so a wrong chain still ends near x0_true: compare every step's x0_hat
    wrong = _perfect_chain(kind, "epsilon", clip, x0_true, x_T, zs, feed="v_prediction")
    err = max(rel_l2(w[1], r[1]) for w, r in zip(wrong, ref))
    assert err > 0.1, err


@pytest.mark.parametrize("pred", NEW_TYPES)
@pytest.mark.parametrize("kind,eta", [("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5)])
def test_device_sampler_step_equals_the_host_driven_step(cuda, kind, eta, pred):
    sch = _sched(kind, pred, nsteps=50)
    smp = sch.device_sampler(seed=99, eta=eta)
    g = torch.Generator(device=cuda).manual_seed(5)
    ref = torch.randn((2, 4, 8, 8, 8), device=cuda, generator=g)
    tbuf = torch.empty((2,), device=cuda)
    smp.reset(tbuf)
    ts = sch.timesteps.tolist()
    for k in range(5):
        t = ts[k]
        assert tbuf.tolist() == [float(t)] * 2
        m = torch.randn(ref.shape, device=cuda, generator=g)
        z = smp.noise(k, ref.shape, cuda)
        want, want_x0 = sch.step(m, t, ref, noise=z) if kind == "ddpm" else sch.step(m, t, ref, eta=eta, noise=z)
        x, x0 = ref.clone(), torch.empty_like(ref)
        smp.step(m, x, tbuf, x0_out=x0)
        assert torch.equal(x, want) and torch.equal(x0, want_x0), (k, rel_l2(x, want))
        ref = want


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_v_prediction_denoise_step_equals_forward_plus_step(cuda, precision):
    """denoise_step (eager and one HIP graph per step) with a v_prediction sampler == UNet forward + scheduler.step, bit for bit."""
    m = _unet(cfgs.UNET_TINY_COND, cuda)
    m.set_precision(precision)
    g = torch.Generator(device=cuda).manual_seed(2)
    xT = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g)
    cond = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g)
    tbuf = torch.empty((1,), device=cuda)
    with torch.no_grad():
        for kind in ("ddpm", "ddim"):
            sch = _sched(kind, "v_prediction", nsteps=10)
            ts = sch.timesteps.tolist()
            ref = xT.clone()
            smp = sch.device_sampler(seed=7)
            for k in range(4):
                eps = m(x=ref, timesteps=torch.full((1,), float(ts[k]), device=cuda), cond=cond)
                ref, _ = sch.step(eps, ts[k], ref, noise=smp.noise(k, ref.shape, cuda)) if kind == "ddpm" else sch.step(eps, ts[k], ref)
            for graph in (False, True):
                m.enable_graph_replay(graph)
                b = sch.device_sampler(seed=7)
                x = xT.clone()
                b.reset(tbuf)
                for _ in range(4):
                    m.denoise_step(x, tbuf, b, cond=cond)
                assert torch.equal(x, ref), (kind, precision, graph, rel_l2(x, ref))
            m.enable_graph_replay(False)


def test_v_prediction_windowed_step_equals_its_pieces(cuda):
    """gather -> forward per chunk -> blend -> scheduler.step (host-driven, v_prediction) == the fused windowed step, bit for bit,
    with all 12 windows in one chunk and in ragged chunks of 5, eager and graph."""
    from ldm3d.sliding import WindowGrid
    m = _unet(cfgs.UNET_TINY_COND, cuda)
    g = torch.Generator(device=cuda).manual_seed(5)
    xT = torch.randn((1, 4, 13, 14, 17), device=cuda, generator=g)
    cond = torch.randn((1, 4, 13, 14, 17), device=cuda, generator=g)
    grid = WindowGrid(xT.shape[2:], 8)
    assert grid.n_windows == 12
    with torch.no_grad():
        for kind in ("ddpm", "ddim"):
            sch = _sched(kind, "v_prediction", nsteps=10)
            ts = sch.timesteps.tolist()
            noise_src = sch.device_sampler(17)
            for chunk in (12, 5):
                ref = xT.clone()
                cw = grid.gather(cond)
                for k in range(3):
                    xw = grid.gather(ref)
                    eps_w = torch.empty((12, 4) + grid.roi, device=cuda)
                    for b0 in range(0, 12, chunk):
                        nb = min(chunk, 12 - b0)
                        eps_w[b0:b0 + nb] = m(x=xw[b0:b0 + nb], timesteps=torch.full((nb,), float(ts[k]), device=cuda), cond=cw[b0:b0 + nb])
                    blended = grid.blend(eps_w)
                    if kind == "ddpm":
                        ref, _ = sch.step(blended, ts[k], ref, noise=noise_src.noise(k, ref.shape, cuda))
                    else:
                        ref, _ = sch.step(blended, ts[k], ref)
                for graph in (False, True):
                    m.enable_graph_replay(graph)
                    smp = sch.device_sampler(17)
                    x = xT.clone()
                    tbuf = torch.empty((chunk,), device=cuda)
                    smp.reset(tbuf)
                    for _ in range(3):
                        m.denoise_step_windows(x, tbuf, smp, grid, cond_windows=cw, sw_batch_size=chunk)
                    m.enable_graph_replay(False)
                    assert torch.equal(x, ref), (kind, chunk, graph, rel_l2(x, ref))


def test_new_kernel_instantiations_use_no_scratch(built_lib):
    csrc = os.path.join(ROOT, "3d-latent-diffusion-model_amd", "csrc")
    res = os.path.join(csrc, "resource_usage.txt")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hip"))]
    if not os.path.exists(res) or os.path.getmtime(res) < max(os.path.getmtime(f) for f in srcs):
        subprocess.run(["make", "-C", csrc, "asm"], check=True, capture_output=True, timeout=900)
    text = open(res).read()
    names = [f"_Z19sampler_step_kernelILi{p}E" for p in (1, 2)] + [f"_Z24window_blend_step_kernelILi{p}E" for p in (1, 2)]
    names += [f"_Z21scheduler_step_kernelILi{p}E" for p in (0, 1, 2)] + [f"_Z23add_noise_target_kernelILi{p}E" for p in (0, 1, 2)]
    # every instantiation of the two step kernels: <prediction type, family>, family 0 DDPM / DDIM, 1 PNDM (epsilon, v), 2 flow
    rules = [(0, 0), (1, 0), (2, 0), (0, 1), (2, 1), (0, 2)]
    names += [f"_Z19sampler_step_kernelILi{p}ELi{f}EE" for p, f in rules] + [f"_Z24window_blend_step_kernelILi{p}ELi{f}EE" for p, f in rules]
    assert text.count("Function Name: _Z19sampler_step_kernel") == text.count("Function Name: _Z24window_blend_step_kernel") == len(rules)
    for name in names:
        i = text.index("Function Name: " + name)
        block = text[i:i + 2000]
        assert "ScratchSize [bytes/lane]: 0 " in block and "VGPRs Spill: 0 " in block, block


def _trainer(cuda, pred):
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.networks import AutoencoderKL, DiffusionModelUNet
    from ldm3d.schedulers import DDPMScheduler
    from ldm3d.trainer import DiffusionTrainer
    from oracle import autoencoder as oa
    from oracle import unet as ou
    vcfg = dict(cfgs.VAE_TINY, in_channels=1, out_channels=1, latent_channels=4)
    vae = AutoencoderKL(**vcfg)
    vae.load_state_dict(ou.init_state_dict(oa.ae_param_shapes(vcfg), 2))
    unet = DiffusionModelUNet(**cfgs.UNET_TINY_COND)
    unet.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfgs.UNET_TINY_COND), 3, gain=0.5))
    sch = DDPMScheduler(**cfgs.SCHED, prediction_type=pred)
    return DiffusionTrainer(unet.to(cuda), vae.to(cuda).eval(), LatentDiffusionInferer(sch, scale_factor=1.0), lr=1e-5)


def test_train_step_regresses_onto_the_velocity(cuda):
    g = torch.Generator().manual_seed(3)
    images = torch.rand((1, 1, 32, 32, 32), generator=g).to(cuda)      # latent 8^3
    labels = torch.rand((1, 1, 32, 32, 32), generator=g).to(cuda)
    noise = torch.randn((1, 4, 8, 8, 8), generator=g).to(cuda)
    t = torch.tensor([613], device=cuda)
    tr = _trainer(cuda, "v_prediction")
    sch = tr.inferer.scheduler
    with torch.no_grad():                                             # the prediction and the target, independently of train_step
        torch.manual_seed(11)
        il = tr.autoencoder.encode_stage_2_inputs(images)
        z = tr.autoencoder.encode_stage_2_inputs(labels)
        tr.unet.eval()
        pred = tr.unet(x=sch.add_noise(z, noise, t), timesteps=t, cond=il).double().cpu()
    a = float(sch.alphas_cumprod.double()[613])
    v64 = a ** 0.5 * noise.double().cpu() - (1 - a) ** 0.5 * z.double().cpu()
    want = float(((pred - v64) ** 2).mean())
    with torch.no_grad():                                             # the target the trainer regresses onto is the velocity
        _, target = tr.inferer(inputs=labels, autoencoder_model=tr.autoencoder, diffusion_model=tr.unet, noise=noise, timesteps=t,
                               condition=il, mode="concat", vae_eps=torch.zeros_like(noise), return_target=True)
        z0 = tr.autoencoder.encode_stage_2_inputs(labels, torch.zeros_like(noise)).double().cpu()
    assert rel_l2(target, a ** 0.5 * noise.double().cpu() - (1 - a) ** 0.5 * z0) <= 1e-6
    torch.manual_seed(11)
    loss, skipped = tr.train_step(images, labels, noise=noise, timesteps=t)
    assert not bool(skipped)
    loss = float(loss)
    # the same forward up to the training plan's own rounding (bf16) and <= 1 ulp in the noisy input
    assert abs(loss - want) <= 1e-2 * want, (loss, want)
    with torch.no_grad():
        torch.manual_seed(11)
        val = tr.validate([{"image": images, "label": labels}], cuda)
    assert val == val and val > 0


def test_epsilon_return_target_is_the_noise_unchanged(cuda):
    tr = _trainer(cuda, "epsilon")
    g = torch.Generator().manual_seed(8)
    images = torch.rand((1, 1, 32, 32, 32), generator=g).to(cuda)
    labels = torch.rand((1, 1, 32, 32, 32), generator=g).to(cuda)
    noise = torch.randn((1, 4, 8, 8, 8), generator=g).to(cuda)
    t = torch.tensor([250], device=cuda)
    with torch.no_grad():
        il = tr.autoencoder.encode_stage_2_inputs(images)
        kw = dict(inputs=labels, autoencoder_model=tr.autoencoder, diffusion_model=tr.unet, noise=noise, timesteps=t, condition=il,
                  mode="concat")
        vae_eps = torch.randn((1, 4, 8, 8, 8), generator=g).to(cuda)
        plain = tr.inferer(**kw, vae_eps=vae_eps)
        pred, target = tr.inferer(**kw, vae_eps=vae_eps, return_target=True)
    assert target is noise and torch.equal(pred, plain)


def _nifti_dims(path):
    with open(path, "rb") as fh:
        hdr = fh.read(348)
    return struct.unpack("<8h", hdr[40:56])


def test_cli_trains_and_samples_with_v_prediction(tmp_path):
    cfg = json.load(open(os.path.join(ROOT, "config", "config_synthetic_train.json")))
    cfg["NoiseScheduler"]["prediction_type"] = "v_prediction"
    cfg_file = str(tmp_path / "config_v.json")
    json.dump(cfg, open(cfg_file, "w"))
    env = {"npz_dir": str(tmp_path / "pairs"), "val_fraction": 0.5, "model_dir": str(tmp_path / "ckpt"),
           "tfevent_path": str(tmp_path / "tfevent"), "resume_ckpt": False, "seed": 0}

    def run(script, out, *extra):
        env_file = str(tmp_path / f"environment_{out}.json")
        json.dump(dict(env, output_dir=str(tmp_path / out)), open(env_file, "w"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, script), "-e", env_file, "-c", cfg_file, *extra], cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run("train_diffusion.py", "out", "--synthetic", "2", "--max-steps", "2", "--random-init")
    pair = sorted((tmp_path / "pairs").glob("*.npz"))[0]
    patch = tuple(cfg["diffusion_train"]["patch_size"])
    run("inference.py", "out_patch", "-n", "1", "--random-init", "--steps", "4", "--condition", str(pair))
    run("inference.py", "out_sw", "-n", "1", "--random-init", "--steps", "4", "--condition", str(pair), "--sliding-window")
    for out in ("out_patch", "out_sw"):
        vols = sorted((tmp_path / out).glob("*.nii"))
        assert len(vols) == 1, out
        assert tuple(_nifti_dims(vols[0])[1:4]) == patch, (out, _nifti_dims(vols[0]))
