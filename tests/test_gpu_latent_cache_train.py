"""Stage-2 training from a latent cache (-m gpu): ``DiffusionTrainer.train_step_cached`` against ``train_step`` bit for bit, the
device-side NaN-skip, and ``train_diffusion.py --cache-latents`` as a child process."""
import json
import os
import subprocess
import sys

import pytest
import torch

import cfgs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
VCFG = dict(cfgs.VAE_TINY, in_channels=1, out_channels=1, latent_channels=4)     # 4 latent channels: UNET_TINY_COND takes 4 + 4
PATCH, LATENT = (16, 16, 16), (4, 4, 4, 4)


class _Pairs:
    """Three fixed pairs with the attributes LatentCache.build reads off a PairVolumes."""
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
    """The frozen autoencoder, the pairs and their cache (built once, never written: the NaN test works on a copy)."""
    from ldm3d.latents import LatentCache
    from ldm3d.networks import AutoencoderKL
    from oracle import autoencoder as oa, unet as ou
    vae = AutoencoderKL(**VCFG)
    vae.load_state_dict(ou.init_state_dict(oa.ae_param_shapes(VCFG), 2))
    vae = vae.to(cuda).eval()
    pairs = _Pairs()
    cache = LatentCache.build(vae, pairs, cuda)
    assert len(cache) == 3 and cache.latent_shape == LATENT and cache.nbytes == 16 * 3 * 256 and cache.build_seconds > 0
    return vae, pairs, cache


def _trainer(cuda, vae, pred, scale):
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.networks import DiffusionModelUNet
    from ldm3d.schedulers import DDPMScheduler
    from ldm3d.trainer import DiffusionTrainer
    from oracle import unet as ou
    unet = DiffusionModelUNet(**cfgs.UNET_TINY_COND)
    unet.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfgs.UNET_TINY_COND), 3, gain=0.5))
    sch = DDPMScheduler(**cfgs.SCHED, prediction_type=pred)
    return DiffusionTrainer(unet.to(cuda), vae, LatentDiffusionInferer(sch, scale_factor=scale), lr=1e-4)


def _draws(cuda, B, seed):
    """(eps_image, eps_label) exactly as train_step's two encodes draw them after torch.manual_seed(seed) -- the image first
    (DiffusionTrainer._predict), then the label (LatentDiffusionInferer.__call__) -- and a noise and timesteps of their own."""
    torch.manual_seed(seed)
    e_image = torch.randn((B,) + LATENT, dtype=torch.float32, device=cuda)
    e_label = torch.randn((B,) + LATENT, dtype=torch.float32, device=cuda)
    g = torch.Generator().manual_seed(seed + 1)
    noise = torch.randn((B,) + LATENT, generator=g).to(cuda)
    return e_image, e_label, noise


def _same(a, b):
    assert float(a[0]) == float(b[0]) and bool(a[1]) == bool(b[1]) is False
    assert torch.equal(a[2].unet.flat_grads, b[2].unet.flat_grads), float((a[2].unet.flat_grads - b[2].unet.flat_grads).abs().max())
    assert torch.equal(a[2].unet.flat_params, b[2].unet.flat_params)
    assert float(a[2].unet.flat_grads.abs().max()) > 0.0


@pytest.mark.parametrize("pred,scale,sample,t", [("epsilon", 1.0, 2, 417), ("v_prediction", 0.7311, 0, 999)])
def test_cached_step_equals_the_uncached_step_at_batch_one(cuda, world, pred, scale, sample, t):
    """Same loss, gradients and post-step parameters, bit for bit: the cache holds what the step's own batch-1 encodes compute, and
    ldm_latent_batch rounds as the chain behind them does."""
    vae, pairs, cache = world
    e_image, e_label, noise = _draws(cuda, 1, 11)
    ts = torch.tensor([t], device=cuda)
    plain, cached = _trainer(cuda, vae, pred, scale), _trainer(cuda, vae, pred, scale)
    item = pairs[sample]
    torch.manual_seed(11)
    la, sa = plain.train_step(item["image"][None].to(cuda), item["label"][None].to(cuda), noise=noise, timesteps=ts)
    lb, sb = cached.train_step_cached(cache, [sample], noise=noise, timesteps=ts, eps_label=e_label, eps_image=e_image)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(la)) and cached.cached_steps == 1
    _same((la, sa, plain), (lb, sb, cached))


@pytest.mark.parametrize("pred,scale", [("epsilon", 0.7311), ("v_prediction", 1.0)])
def test_cached_step_equals_a_step_assembled_from_per_sample_encodes_at_batch_two(cuda, world, pred, scale):
    """B = 2 with a repeated-order batch [2, 0]: the uncached side encodes sample by sample (the encoder is not bitwise batch
    independent, and the cache is built at batch 1), then runs today's chain: scale, add_noise_and_target, UNet, mse_loss, backward, Adam."""
    from ldm3d.optim import mse_loss
    vae, pairs, cache = world
    idx = [2, 0]
    e_image, e_label, noise = _draws(cuda, 2, 5)
    ts = torch.tensor([0, 613], device=cuda)
    plain, cached = _trainer(cuda, vae, pred, scale), _trainer(cuda, vae, pred, scale)
    plain.unet.train()
    plain.optimizer.zero_grad(set_to_none=True)
    with torch.no_grad():
        cond = torch.cat([vae.encode_stage_2_inputs(pairs[n]["image"][None].to(cuda), e_image[b:b + 1]) for b, n in enumerate(idx)])
        z = torch.cat([vae.encode_stage_2_inputs(pairs[n]["label"][None].to(cuda), e_label[b:b + 1]) for b, n in enumerate(idx)])
        if scale != 1.0:
            z = z * scale
    noisy, target = plain.inferer.scheduler.add_noise_and_target(original_samples=z, noise=noise, timesteps=ts)
    la = mse_loss(plain.unet(x=noisy, timesteps=ts, context=None, cond=cond), target)
    before = plain.optimizer.skipped_steps().clone()
    la.backward()
    plain.optimizer.step()
    sa = plain.optimizer.skipped_steps() > before
    lb, sb = cached.train_step_cached(cache, idx, noise=noise, timesteps=ts, eps_label=e_label, eps_image=e_image)
    torch.cuda.synchronize()
    _same((la.detach(), sa, plain), (lb, sb, cached))


def test_device_draw_steps_train_and_validate(cuda, world):
    """Without explicit draws the step keys the kernel's draws by (cache_seed, cached_steps): two trainers with one seed walk the same
    path, another seed leaves it, and validate_cached returns a finite mean without moving the weights."""
    vae, _, cache = world
    runs = []
    for seed in (3, 3, 4):
        tr = _trainer(cuda, vae, "epsilon", 0.7311)
        tr.cache_seed = seed
        losses = []
        for k, idx in enumerate(([0, 1], [2, 1])):
            loss, skipped = tr.train_step_cached(cache, idx, timesteps=torch.tensor([100 + k, 900], device=cuda))
            assert not bool(skipped)
            losses.append(float(loss))
        assert tr.cached_steps == 2 and all(x == x and x > 0 for x in losses)
        runs.append((losses, tr.unet.flat_params.clone(), tr))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][0] != runs[2][0] and not torch.equal(runs[0][1], runs[2][1])
    tr = runs[0][2]
    val = tr.validate_cached(cache, [[0, 1], [2]])
    assert val == val and 0 < val < float("inf") and tr.cached_val_steps == 2 and torch.equal(tr.unet.flat_params, runs[0][1])


def test_a_nan_in_a_cache_row_skips_the_step_on_the_device(cuda, world):
    from ldm3d.latents import LatentCache
    vae, _, cache = world
    bad = LatentCache(cache.mu_label.clone(), cache.sigma_label.clone(), cache.mu_image.clone(), cache.sigma_image.clone())
    bad.mu_label[1, 2, 1, 0, 3] = float("nan")
    tr = _trainer(cuda, vae, "epsilon", 1.0)
    p0 = tr.unet.flat_params.clone()
    loss, skipped = tr.train_step_cached(bad, [0, 1], timesteps=torch.tensor([10, 20], device=cuda))
    assert bool(skipped) and bool(torch.isnan(loss)) and torch.equal(tr.unet.flat_params, p0)
    loss, skipped = tr.train_step_cached(bad, [0, 2], timesteps=torch.tensor([10, 20], device=cuda))   # the other rows still train
    assert not bool(skipped) and bool(torch.isfinite(loss)) and not torch.equal(tr.unet.flat_params, p0)


def test_cli_trains_from_the_cache(tmp_path):
    """train_diffusion.py --random-init --synthetic 4 --max-steps 4 --cache-latents (and --sample-steps 2, which only shortens the
    periodic sample: it still takes its batch from the loader): checkpoints and scale_factor.json are written, the losses are finite, and
    each cache is built once."""
    env = {"npz_dir": str(tmp_path / "pairs"), "val_fraction": 0.25, "model_dir": str(tmp_path / "ckpt"),
           "tfevent_path": str(tmp_path / "tfevent"), "output_dir": str(tmp_path / "out"), "resume_ckpt": False, "seed": 0}
    env_file = str(tmp_path / "environment.json")
    json.dump(env, open(env_file, "w"))
    cmd = [sys.executable, os.path.join(ROOT, "train_diffusion.py"), "-e", env_file, "-c", os.path.join(ROOT, "config", "config_synthetic_train.json"),
           "--random-init", "--synthetic", "4", "--max-steps", "4", "--cache-latents", "--sample-steps", "2"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    for name in ("diffusion_unet.pt", "diffusion_unet_last.pt", "diffusion_train_state.pt", "scale_factor.json"):
        assert os.path.exists(tmp_path / "ckpt" / name), name
    assert json.load(open(tmp_path / "ckpt" / "scale_factor.json"))["scale_factor"] > 0
    assert log.count("latent cache (train): 3 samples of 4x24x24x24") == 1 and log.count("latent cache (val): 1 samples") == 1, log[-3000:]
    assert "NaN loss" not in log and "conditional sample (2 steps" in log
    rows = [json.loads(line) for line in open(tmp_path / "tfevent" / "diffusion" / "scalars.jsonl")]
    losses = [x["value"] for x in rows if x["tag"] == "train_diffusion_loss_iter"]
    vals = [x["value"] for x in rows if x["tag"] == "val_diffusion_loss"]
    assert len(losses) == 4 and all(v == v and 0 < v < float("inf") for v in losses + vals) and len(vals) >= 1
