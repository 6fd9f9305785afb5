"""Gradient accumulation through DiffusionTrainer (-m gpu): UNET_TINY_COND with the VAE_TINY-class autoencoder and the sizes of
test_gpu_latent_cache_train.py / test_gpu_ema_train.py.  Noise and timesteps are explicit; the reference of every window is built from the
micro gradients the window's own backwards left in ``flat_grads`` (which tests/test_gpu_grad_accum.py pins to the un-armed backward), so
nothing depends on a draw."""
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
LR = 1e-4


class _Pairs:
    """Four fixed pairs with the attributes LatentCache.build reads off a PairVolumes."""
    randcrop, scale_on_host = False, True

    def __init__(self):
        g = torch.Generator().manual_seed(21)
        self.items = [{"image": torch.rand((1,) + PATCH, generator=g), "label": torch.rand((1,) + PATCH, generator=g)} for _ in range(4)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


@pytest.fixture(scope="module")
def world(cuda):
    """The frozen autoencoder, the pairs, their cache and the explicit draws (built once, never written)."""
    from ldm3d.latents import LatentCache
    from ldm3d.networks import AutoencoderKL
    from oracle import autoencoder as oa, unet as ou
    vae = AutoencoderKL(**VCFG)
    vae.load_state_dict(ou.init_state_dict(oa.ae_param_shapes(VCFG), 2))
    vae = vae.to(cuda).eval()
    pairs = _Pairs()
    cache = LatentCache.build(vae, pairs, cuda)
    g = torch.Generator().manual_seed(3)
    noise = torch.randn((4, 1) + LATENT, generator=g).to(cuda)
    ts = [torch.tensor([t], device=cuda) for t in (417, 12, 903, 650)]
    return vae, pairs, cache, noise, ts


def _trainer(cuda, vae, **kw):
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.networks import DiffusionModelUNet
    from ldm3d.schedulers import DDPMScheduler
    from ldm3d.trainer import DiffusionTrainer
    from oracle import unet as ou
    unet = DiffusionModelUNet(**cfgs.UNET_TINY_COND)
    unet.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfgs.UNET_TINY_COND), 3, gain=0.5))
    return DiffusionTrainer(unet.to(cuda), vae, LatentDiffusionInferer(DDPMScheduler(**cfgs.SCHED), scale_factor=0.7311), lr=LR, **kw)


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _state(tr):
    opt = tr.optimizer
    return (tr.unet.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), None if opt.ema_params is None else opt.ema_params.clone(),
            float(opt.skipped_steps()), opt.steps)


def _unchanged(tr, st):
    opt = tr.optimizer
    assert _same(tr.unet.flat_params, st[0]) and _same(opt.exp_avg, st[1]) and _same(opt.exp_avg_sq, st[2])
    assert (opt.ema_params is None) if st[3] is None else _same(opt.ema_params, st[3])
    assert float(opt.skipped_steps()) == st[4] and opt.steps == st[5]


def _adam_by_hand(L, p0, m0, v0, g, step, lr=LR, max_norm=1.0):
    """ldm_grad_sq_norm + ldm_adam_step (Adam defaults, no weight decay) on copies of the state: the parameters and moments after it."""
    from ldm3d import _lib
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    sq = torch.zeros(2, device=p.device)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.ldm_grad_sq_norm(g.data_ptr(), g.numel(), sq.data_ptr(), st))
    _lib.check(L.ldm_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, 0.9, 0.999, 1e-8, 0.0, step, sq.data_ptr(),
                               max_norm, st))
    torch.cuda.synchronize()
    return p, m, v


def _window_reference(micro_grads):
    K = len(micro_grads)
    s = torch.tensor(float(1.0 / K), dtype=torch.float32, device=micro_grads[0].device)
    acc = micro_grads[0] * s
    for g in micro_grads[1:]:
        acc = acc + g * s
    return acc


def _check_two_windows(tr, L, call):
    """K = 2, four calls: the first call of each window changes nothing, the second applies ldm_adam_step to the accumulated gradient."""
    opt = tr.optimizer
    assert opt.grad_accum is None and tr.grad_accum_steps == 2
    for w in range(2):
        st = _state(tr)
        l0, s0 = call(2 * w)
        assert tr.stepped is False and s0.dtype == torch.bool and s0.is_cuda and not bool(s0)
        _unchanged(tr, st)
        g0 = tr.unet.flat_grads.clone()
        l1, s1 = call(2 * w + 1)
        torch.cuda.synchronize()
        assert tr.stepped is True and not bool(s1) and opt.micro == 0
        g1 = tr.unet.flat_grads.clone()
        assert not _same(g0, g1) and bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
        ref = _window_reference([g0, g1])
        assert opt.grads is opt.grad_accum and _same(opt.grads, ref)
        p, m, v = _adam_by_hand(L, st[0], st[1], st[2], ref, step=w + 1)
        assert not _same(p, st[0])
        assert _same(tr.unet.flat_params, p) and _same(opt.exp_avg, m) and _same(opt.exp_avg_sq, v)
        assert opt.steps == w + 1 and float(opt.skipped_steps()) == 0.0
        assert opt.ema_params is not None and (w == 0 or not _same(opt.ema_params, st[3]))
        assert float(tr.window_loss) == float((l0 + l1) / 2) and float(l0) != float(l1)


def test_a_window_of_two_steps_once_on_the_accumulated_gradient(cuda, built_lib, world):
    vae, pairs, _, noise, ts = world
    tr = _trainer(cuda, vae, grad_accum_steps=2, ema_decay=0.999)
    draws0 = tr.timestep_draws
    torch.manual_seed(11)

    def call(k):
        item = pairs[k]
        return tr.train_step(item["image"][None].to(cuda), item["label"][None].to(cuda), noise=noise[k], timesteps=ts[k])
    _check_two_windows(tr, built_lib, call)
    assert tr.timestep_draws == draws0                       # explicit draws without condition dropout: the counter stays, as at K = 1


def test_the_cached_path_accumulates_the_same_way(cuda, built_lib, world):
    vae, _, cache, noise, ts = world
    tr = _trainer(cuda, vae, grad_accum_steps=2, ema_decay=0.999)

    def call(k):
        return tr.train_step_cached(cache, [k], timesteps=ts[k])
    _check_two_windows(tr, built_lib, call)
    assert tr.cached_steps == 4                              # per micro-batch


def test_one_step_windows_equal_a_trainer_built_without_the_argument(cuda, world):
    vae, pairs, _, noise, ts = world
    runs = []
    for kw in ({}, {"grad_accum_steps": 1}):
        tr = _trainer(cuda, vae, **kw)
        torch.manual_seed(11)
        out = []
        for k in range(2):
            item = pairs[k]
            loss, skipped = tr.train_step(item["image"][None].to(cuda), item["label"][None].to(cuda), noise=noise[k], timesteps=ts[k])
            assert tr.stepped is True and not bool(skipped)
            out.append((float(loss), tr.unet.flat_grads.clone(), tr.unet.flat_params.clone()))
        assert tr.optimizer.grad_accum is None and tr.optimizer.grads is tr.unet.flat_grads
        runs.append(out)
    for a, b in zip(*runs):
        assert a[0] == b[0] and _same(a[1], b[1]) and _same(a[2], b[2])
    assert not _same(runs[0][0][2], runs[0][1][2])


def test_a_nan_micro_batch_drops_the_whole_window_and_the_next_one_applies(cuda, world):
    vae, pairs, _, noise, ts = world
    tr = _trainer(cuda, vae, grad_accum_steps=2)
    p0 = tr.unet.flat_params.clone()
    torch.manual_seed(11)
    bad = pairs[0]["label"][None].clone()
    bad[0, 0, 3, 4, 5] = float("nan")
    loss, skipped = tr.train_step(pairs[0]["image"][None].to(cuda), bad.to(cuda), noise=noise[0], timesteps=ts[0])
    assert tr.stepped is False and not bool(skipped) and bool(torch.isnan(loss))
    loss, skipped = tr.train_step(pairs[1]["image"][None].to(cuda), pairs[1]["label"][None].to(cuda), noise=noise[1], timesteps=ts[1])
    assert tr.stepped is True and bool(skipped) and bool(torch.isfinite(loss))
    assert _same(tr.unet.flat_params, p0) and float(tr.optimizer.skipped_steps()) == 1.0
    assert bool(torch.isnan(tr.optimizer.grads).any())
    for k in (2, 3):                                         # the next window assigns first: the NaN is gone without any clearing
        loss, skipped = tr.train_step(pairs[k]["image"][None].to(cuda), pairs[k]["label"][None].to(cuda), noise=noise[k], timesteps=ts[k])
        assert not bool(skipped)
    assert tr.stepped is True and bool(torch.isfinite(tr.optimizer.grads).all())
    assert not _same(tr.unet.flat_params, p0) and bool(torch.isfinite(tr.unet.flat_params).all())
    assert float(tr.optimizer.skipped_steps()) == 1.0


def test_a_window_of_zero_steps_is_refused(cuda, world):
    with pytest.raises(ValueError):
        _trainer(cuda, world[0], grad_accum_steps=0)
    with pytest.raises(ValueError):
        _trainer(cuda, world[0], grad_accum_steps=2.0)


def test_cli_counts_optimizer_steps_and_logs_the_window_loss(tmp_path):
    """train_diffusion.py --synthetic 8 --max-steps 2 --grad-accum-steps 2 --cache-latents in a fresh child process: four calls, two
    optimizer steps, the window-loss scalar once per optimizer step."""
    env = {"npz_dir": str(tmp_path / "pairs"), "val_fraction": 0.25, "model_dir": str(tmp_path / "ckpt"),
           "tfevent_path": str(tmp_path / "tfevent"), "output_dir": str(tmp_path / "out"), "resume_ckpt": False, "seed": 0}
    env_file = str(tmp_path / "environment.json")
    json.dump(env, open(env_file, "w"))
    cmd = [sys.executable, os.path.join(ROOT, "train_diffusion.py"), "-e", env_file, "-c", os.path.join(ROOT, "config", "config_synthetic_train.json"),
           "--random-init", "--synthetic", "8", "--max-steps", "2", "--grad-accum-steps", "2", "--cache-latents", "--sample-steps", "2"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    assert "NaN loss" not in log
    rows = [json.loads(line) for line in open(tmp_path / "tfevent" / "diffusion" / "scalars.jsonl")]
    calls = [x for x in rows if x["tag"] == "train_diffusion_loss_iter"]
    windows = [x for x in rows if x["tag"] == "train_diffusion_loss_window"]
    assert [x["step"] for x in calls] == [1, 2, 3, 4] and [x["step"] for x in windows] == [1, 2]
    assert all(x["value"] == x["value"] and 0 < x["value"] < float("inf") for x in calls + windows)
    for w, x in enumerate(windows):                          # the mean of its two calls (summed in fp32 on the device)
        assert abs(x["value"] - 0.5 * (calls[2 * w]["value"] + calls[2 * w + 1]["value"])) <= 1e-6 * x["value"]
    state = torch.load(tmp_path / "ckpt" / "diffusion_train_state.pt", map_location="cpu", weights_only=True)
    assert int(state["total_step"]) == 2 and int(state["optimizer"]["steps"]) == 2 and int(state["open_micro_batches"]) == 0
