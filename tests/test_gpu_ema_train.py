"""EMA weights through the Python layers (-m gpu): FlatAdam(ema_decay=...) against the float64 reference (tests/ema_ref.py), the moment the
EMA is initialised, ``ema_weights()`` on the eager forward, under HIP-graph replay with the device sampler (the stale time-embedding-table
and stale-graph case) and in the fp32 precision mode, the optimizer's ``state_dict`` round trip, and the entry points end to end
(train_diffusion.py --ema-decay / --resume, inference.py --ema) as child processes.  Gradients are written straight into ``flat_grads``:
the optimizer tail is elementwise and deterministic, no backward is involved."""
import json
import os
import subprocess
import sys

import pytest
import torch

import cfgs
import ema_ref as E
import gan_ops_ref as R
from test_gpu_f32_ops import TOL_EXACT, _rel
from test_gpu_optim_ops import _bits_equal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, DECAY = 1e-2, 0.999


def _unet(cuda, seed=31, precision="bf16", state=None):
    from ldm3d.networks import DiffusionModelUNet
    torch.manual_seed(seed)
    m = DiffusionModelUNet(**cfgs.UNET_TINY)
    if state is not None:
        m.load_state_dict(state)
    else:
        with torch.no_grad():                                  # MONAI zero-initialises some convs: give every weight a value
            for q in m.parameters():
                if q.dim() > 1 and not bool(q.any()):
                    q.normal_(0.0, 0.05)
    m = m.to(cuda).eval()
    if precision == "fp32":
        m.set_precision("fp32")
    return m


def _grads(n, count, nan_at, seed=4):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for k in range(count):
        g = 0.1 * torch.randn((n,), generator=gen)
        if k == nan_at:
            g[n // 2] = float("nan")
        out.append(g)
    return out


def _step(opt, m, g):
    m.flat_grads.copy_(g)
    opt.step()


def _trained(cuda, precision="bf16", steps=3):
    """A module whose EMA differs from its live weights: `steps` optimizer steps on random gradients."""
    from ldm3d.optim import FlatAdam
    m = _unet(cuda, precision=precision)
    opt = FlatAdam(m, lr=LR, max_grad_norm=1.0, ema_decay=DECAY)
    for g in _grads(m.flat_params.numel(), steps, nan_at=-1):
        _step(opt, m, g)
    m.eval()
    return m, opt


@pytest.mark.parametrize("fused", [True, False])
def test_flat_adam_ema_against_float64(cuda, fused):
    """FlatAdam(ema_decay=0.999) on UNET_TINY, four steps, the second with a NaN gradient, on the fused re-pack path
    (ldm_model_adam_step_ema) and the plain one (ldm_adam_step_ema): p and ema_params agree with the float64 reference at 1e-5 and
    skipped_steps() == 1.  Measured rel-L2 on both paths: p 3.7e-07, ema 3.7e-07."""
    from ldm3d.optim import FlatAdam
    m = _unet(cuda)
    opt = FlatAdam(m, lr=LR, max_grad_norm=1.0, ema_decay=DECAY)
    opt.fuse_repack = fused
    n = m.flat_params.numel()
    assert opt.ema_params is None
    p = m.flat_params.cpu().double()
    mo, v, ema, skipped = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), p.clone(), 0
    hp = (R.f32(LR), R.f32(0.9), R.f32(0.999), R.f32(1e-8), 0.0)
    for k, g in enumerate(_grads(n, 4, nan_at=1)):
        if fused:
            m._sync_weights()                                  # what a forward does: nothing stale, step() takes the one-pass path
        _step(opt, m, g)
        sq = float(opt.sq_norm[0])                             # the fp32 norm the kernel read
        p, mo, v, ema, skipped = E.adam_ema_ref(p, g, mo, v, ema, *hp, k + 1, skipped, R.f32(DECAY), True, sq, 1.0)
    errs = _rel(m.flat_params, p), _rel(opt.ema_params, ema)
    print(f"FlatAdam EMA fused={fused}: rel-L2 p {errs[0]:.2e}, ema {errs[1]:.2e} (gate {TOL_EXACT:.0e})")
    assert float(opt.skipped_steps()) == 1.0 and skipped == 1
    assert max(errs) <= TOL_EXACT, errs
    assert _rel(opt.ema_params, p) > 100 * TOL_EXACT, "the EMA must lag the live weights here"


def test_ema_starts_from_the_parameters_of_the_first_step(cuda):
    """Parameters overwritten after the optimizer was constructed (a broadcast, a checkpoint load) and before its first step: after that
    step the EMA is 0.1 (overwritten) + 0.9 (new), not a mix with the values of construction time.  Measured rel-L2 2.4e-08."""
    from ldm3d.optim import FlatAdam
    m = _unet(cuda)
    opt = FlatAdam(m, lr=LR, max_grad_norm=1.0, ema_decay=DECAY)
    n = m.flat_params.numel()
    gen = torch.Generator().manual_seed(9)
    over = torch.randn((n,), generator=gen)
    m.flat_params.copy_(over)
    m.mark_weights_dirty()
    _step(opt, m, _grads(n, 1, -1)[0])
    want = 0.1 * over.double() + 0.9 * m.flat_params.cpu().double()
    e = _rel(opt.ema_params, want)
    print(f"EMA after the first step vs 0.1 old + 0.9 new: rel-L2 {e:.2e} (gate {TOL_EXACT:.0e})")
    assert e <= TOL_EXACT


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_ema_weights_on_the_eager_forward(cuda, precision):
    """Inside ``ema_weights()`` the forward is bit-identical to a second module that loaded ``ema_state_dict()``; after the block it is
    bit-identical to the one before it; ``flat_params`` never changes; ``state_dict()`` inside returns the live weights; ``train()``,
    ``step()`` and a grad-enabled forward inside raise.  Also in the fp32 precision mode (the fp32 arena follows)."""
    m, opt = _trained(cuda, precision)
    other = _unet(cuda, precision=precision, state=opt.ema_state_dict())
    gen = torch.Generator().manual_seed(6)
    x = torch.randn((1, 4, 8, 8, 8), generator=gen).to(cuda)
    t = torch.tensor([500.0], device=cuda)
    live = m.flat_params.clone()
    key = next(iter(m.state_dict()))
    with torch.no_grad():
        before = m(x=x, timesteps=t).clone()
        ref = other(x=x, timesteps=t).clone()
        with opt.ema_weights():
            inside = m(x=x, timesteps=t).clone()
            assert _bits_equal(m.flat_params, live) and torch.equal(m.state_dict()[key], dict(m.named_parameters())[key])
            with pytest.raises(RuntimeError):
                m.train()
            with pytest.raises(RuntimeError):
                opt.step()
            with pytest.raises(RuntimeError), torch.enable_grad():
                m(x=x, timesteps=t)
            again = m(x=x, timesteps=t).clone()
        after = m(x=x, timesteps=t).clone()
    assert not m.training
    assert torch.isfinite(inside).all() and _bits_equal(inside, ref) and _bits_equal(again, ref)
    assert _bits_equal(after, before) and _bits_equal(m.flat_params, live)
    assert not _bits_equal(inside, before), "the EMA and the live weights must give different outputs here"
    _step(opt, m, _grads(live.numel(), 1, -1, seed=12)[0])      # the optimizer works again after the block
    assert not _bits_equal(m.flat_params, live)


def test_ema_weights_under_graph_replay_with_the_device_sampler(cuda):
    """Graph replay on, a DeviceSampler: three denoise_steps with the live weights first (so a time-embedding table and a recorded graph
    of the LIVE weights exist), three inside ``ema_weights()``, three after it, always from the same start.  Each trajectory is
    bit-identical to the same steps on a second module that loaded the matching weights: a stale table would sample with EMA convolutions
    and live time embeddings."""
    from ldm3d.schedulers import DDIMScheduler
    m, opt = _trained(cuda)
    mods = {"live": m, "ema_ref": _unet(cuda, state=opt.ema_state_dict()), "live_ref": _unet(cuda, state=m.state_dict())}
    gen = torch.Generator().manual_seed(7)
    x0 = torch.randn((1, 4, 8, 8, 8), generator=gen).to(cuda)
    rig = {}
    for name, mod in mods.items():
        mod.enable_graph_replay(True)
        sch = DDIMScheduler(**cfgs.SCHED)
        sch.set_timesteps(5)
        rig[name] = (mod, sch.device_sampler(seed=3), torch.empty_like(x0), torch.zeros((1,), device=cuda))

    def chain(name):
        mod, sampler, x, tbuf = rig[name]
        x.copy_(x0)
        sampler.reset(tbuf)
        out = []
        with torch.no_grad():
            for _ in range(3):
                mod.denoise_step(x, tbuf, sampler)
                out.append(x.clone())
        return out
    first = chain("live")
    with opt.ema_weights():
        inside = chain("live")
    after = chain("live")
    want_ema, want_live = chain("ema_ref"), chain("live_ref")
    for k in range(3):
        assert torch.isfinite(inside[k]).all()
        assert _bits_equal(inside[k], want_ema[k]), f"step {k} inside ema_weights() is not the EMA model's"
        assert _bits_equal(after[k], want_live[k]) and _bits_equal(first[k], want_live[k]), f"step {k} after ema_weights() is not the live model's"
    assert not _bits_equal(inside[0], first[0])


def test_optimizer_state_dict_resumes_bit_identically(cuda, tmp_path):
    """Four steps in one optimizer against two steps, state_dict() through torch.save / torch.load(weights_only=True), a fresh module and
    optimizer, load_state_dict(), two more steps.  The second gradient is NaN, so the persisted skip counter decides the bias correction
    and the EMA warm-up of steps three and four.  p, m, v, ema and the counter are bit-identical; an EMA on / off mismatch raises."""
    from ldm3d.optim import FlatAdam
    a = _unet(cuda)
    start = {k: v.detach().cpu().clone() for k, v in a.state_dict().items()}
    kw = dict(lr=LR, max_grad_norm=1.0, weight_decay=1e-2, ema_decay=DECAY)
    oa = FlatAdam(a, **kw)
    grads = _grads(a.flat_params.numel(), 4, nan_at=1)
    for g in grads:
        _step(oa, a, g)
    b = _unet(cuda, state=start)
    ob = FlatAdam(b, **kw)
    for g in grads[:2]:
        _step(ob, b, g)
    torch.save({"opt": ob.state_dict(), "unet": b.state_dict()}, tmp_path / "state.pt")
    saved = torch.load(tmp_path / "state.pt", map_location="cpu", weights_only=True)
    assert float(saved["opt"]["skipped"]) == 1.0 and saved["opt"]["steps"] == 2 and saved["opt"]["ema_decay"] == DECAY
    c = _unet(cuda, seed=99, state=saved["unet"])
    oc = FlatAdam(c, **kw)
    oc.load_state_dict(saved["opt"])
    for g in grads[2:]:
        _step(oc, c, g)
    for name, x, y in (("p", a.flat_params, c.flat_params), ("m", oa.exp_avg, oc.exp_avg), ("v", oa.exp_avg_sq, oc.exp_avg_sq),
                       ("ema", oa.ema_params, oc.ema_params), ("counter", oa.sq_norm[1:], oc.sq_norm[1:])):
        assert torch.isfinite(x).all() and _bits_equal(x, y), name
    assert float(oc.skipped_steps()) == 1.0 and oc.steps == 4
    plain = FlatAdam(_unet(cuda, state=start), lr=LR, max_grad_norm=1.0, weight_decay=1e-2)
    with pytest.raises(ValueError, match="EMA"):
        plain.load_state_dict(saved["opt"])
    with pytest.raises(ValueError, match="EMA"):
        oc.load_state_dict(plain.state_dict())


def test_ema_off_allocates_and_saves_nothing(cuda):
    from ldm3d.optim import FlatAdam
    m = _unet(cuda)
    opt = FlatAdam(m, lr=LR, max_grad_norm=1.0)
    _step(opt, m, _grads(m.flat_params.numel(), 1, -1)[0])
    assert opt.ema_params is None and opt.ema_decay is None
    assert not [k for k in opt.state_dict() if "ema" in k]
    with pytest.raises(RuntimeError):
        opt.ema_state_dict()
    with pytest.raises(RuntimeError):
        opt.ema_weights().__enter__()


def test_cli_trains_resumes_and_samples_with_ema(tmp_path):
    """train_diffusion.py --ema-decay writes the four checkpoints and diffusion_train_state.pt, and the EMA file loads into a fresh UNet
    and differs from the live one; --resume continues from total_step 4; inference.py --ema writes a volume and, without the file, exits
    non-zero with a message; without --ema-decay no *_ema* file appears."""
    cfg_file = os.path.join(ROOT, "config", "config_synthetic_train.json")
    env = {"npz_dir": str(tmp_path / "pairs"), "val_fraction": 0.5, "tfevent_path": str(tmp_path / "tfevent"), "resume_ckpt": False, "seed": 0}

    def run(script, model_dir, out, *extra, ok=True):
        env_file = str(tmp_path / f"environment_{out}.json")
        json.dump(dict(env, model_dir=str(tmp_path / model_dir), output_dir=str(tmp_path / out)), open(env_file, "w"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, script), "-e", env_file, "-c", cfg_file, *extra], cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert (r.returncode == 0) == ok, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout + r.stderr
    train = ("--random-init", "--synthetic", "4", "--sample-steps", "2", "--ema-decay", "0.999")
    run("train_diffusion.py", "ckpt", "out", *train, "--max-steps", "4")
    ck = tmp_path / "ckpt"
    names = ("diffusion_unet.pt", "diffusion_unet_last.pt", "diffusion_unet_ema.pt", "diffusion_unet_ema_last.pt", "diffusion_train_state.pt")
    assert all((ck / f).exists() for f in names), sorted(os.listdir(ck))
    from ldm3d.config import define_instance
    import argparse
    ns = argparse.Namespace(**json.load(open(cfg_file)))
    live = torch.load(ck / "diffusion_unet_last.pt", map_location="cpu", weights_only=True)
    ema = torch.load(ck / "diffusion_unet_ema_last.pt", map_location="cpu", weights_only=True)
    res = define_instance(ns, "diffusion_def").load_state_dict(ema)
    assert not res.missing_keys and not res.unexpected_keys
    assert set(ema) == set(live) and any(not torch.equal(ema[k], live[k]) for k in ema)
    state = torch.load(ck / "diffusion_train_state.pt", map_location="cpu", weights_only=True)
    assert state["total_step"] == 4 and state["optimizer"]["steps"] >= 4 and state["optimizer"]["ema"] is not None
    log = run("train_diffusion.py", "ckpt", "out", *train, "--resume", "--max-steps", "6")
    assert "total_step 4" in log, log[-2000:]
    assert torch.load(ck / "diffusion_train_state.pt", map_location="cpu", weights_only=True)["total_step"] == 6
    pair = sorted((tmp_path / "pairs").glob("*.npz"))[0]
    # the stage-1 checkpoint the sampler loads next to the UNet's: the same random autoencoder for every run of this test
    torch.manual_seed(0)
    torch.save(define_instance(ns, "autoencoder_def").state_dict(), ck / "autoencoder.pt")
    run("inference.py", "ckpt", "out_ema", "-n", "1", "--ema", "--steps", "2", "--condition", str(pair))
    assert len(list((tmp_path / "out_ema").glob("*.nii"))) == 1
    (tmp_path / "empty").mkdir()
    msg = run("inference.py", "empty", "out_none", "-n", "1", "--ema", "--steps", "2", "--condition", str(pair), ok=False)
    assert "diffusion_unet_ema.pt" in msg and "not found" in msg
    run("train_diffusion.py", "ckpt_plain", "out", "--random-init", "--synthetic", "4", "--sample-steps", "2", "--max-steps", "2")
    plain = sorted(os.listdir(tmp_path / "ckpt_plain"))
    assert "diffusion_unet.pt" in plain and not [f for f in plain if "ema" in f], plain
