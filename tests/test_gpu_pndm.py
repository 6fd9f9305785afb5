"""PNDMScheduler on the GPU (-m gpu): the host-driven step against the fp64 restatement (tests/pndm_ref.py), the device sampler
against the host-driven step bit for bit, the closed-form trajectory, graph replay, sliding windows, argument errors and the CLI.

Sizes: 1 element, 1003 (ragged last quad) and 4 * 256 * 1024 + 5 (every thread of the 1024-block grid wraps once, then a tail)."""
import copy
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cfgs
from pndm_ref import PNDMRef
from util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SIZES = [1, 1003, 4 * 256 * 1024 + 5]
MODES = {"plms": dict(skip_prk_steps=True, n=10), "prk": dict(skip_prk_steps=False, n=8)}


def _pair(mode, pred, **kw):
    from ldm3d.schedulers import PNDMScheduler
    args = dict(cfgs.SCHED, skip_prk_steps=MODES[mode]["skip_prk_steps"], prediction_type=pred, **kw)
    sch, ref = PNDMScheduler(**args), PNDMRef(**args)
    sch.set_timesteps(MODES[mode]["n"])
    ref.set_timesteps(MODES[mode]["n"])
    assert sch.timesteps.tolist() == ref.timesteps.tolist()
    return sch, ref


def _feed_state(sch, ref, dev):
    """The scheduler's multistep state := the reference's (rounded to fp32)."""
    sch.counter = ref.counter
    sch.ets = [e.float().to(dev) for e in ref.ets]
    sch.cur_sample = None if ref.cur_sample is None else ref.cur_sample.float().to(dev)
    sch.cur_model_output = ref.cur_model_output.float().to(dev) if torch.is_tensor(ref.cur_model_output) else 0


@functools.lru_cache(maxsize=None)
def _chain(mode, pred, n):
    """One whole chain with random model outputs, computed once per case and shared: the outputs, the free-running host-driven chain
    (PNDMScheduler.step on its own state), the fp64 reference chain, and the per-step error of the step fed from the reference's state."""
    dev = torch.device("cuda:0")
    sch, ref = _pair(mode, pred)
    fed = copy.copy(sch)
    g = torch.Generator(device=dev).manual_seed(1000 + n % 997)
    x_init = torch.randn((n,), device=dev, generator=g)
    ts = sch.timesteps.tolist()
    ms, xs, step_err = [], [], []
    x, xr = x_init, x_init.double().cpu()
    for t in ts:
        m = torch.randn((n,), device=dev, generator=g)
        ms.append(m)
        _feed_state(fed, ref, dev)
        got, none = fed.step(m, t, xr.float().to(dev))
        assert none is None
        x, _ = sch.step(m, t, x)
        xs.append(x)
        xr, _ = ref.step(m.double().cpu(), t, xr)
        step_err.append(rel_l2(got, xr))
        assert fed.counter == ref.counter and len(fed.ets) == len(ref.ets)
    return dict(sch=sch, ts=ts, x_init=x_init, ms=ms, xs=xs, ref_end=xr, step_err=step_err)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("mode", ["plms", "prk"])
def test_host_driven_step_matches_fp64(cuda, mode, pred, n):
    """Every step, from the reference's state: rel-L2 <= 1e-6 (the project's scheduler gate).  The end-of-chain error of the chain that
    runs on its own fp32 state is reported, not gated."""
    c = _chain(mode, pred, n)
    end = rel_l2(c["xs"][-1], c["ref_end"])
    print(f"pndm {mode} {pred} n={n}: max per-step rel-L2 {max(c['step_err']):.3e}, end of chain ({len(c['ts'])} calls) {end:.3e}")
    assert len(c["step_err"]) == (11 if mode == "plms" else 17)
    assert max(c["step_err"]) <= 1e-6, c["step_err"]
    assert torch.isfinite(c["xs"][-1]).all()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("mode", ["plms", "prk"])
def test_fused_sampler_equals_host_driven_bitwise(cuda, mode, pred, n):
    c = _chain(mode, pred, n)
    sch, ts = c["sch"], c["ts"]
    smp = sch.device_sampler()
    assert smp.n_steps == len(ts) and smp.state_numel(n) == 6 * n
    x = c["x_init"].clone()
    tbuf = torch.full((2,), -1.0, device=cuda)
    smp.reset(tbuf)
    assert tbuf.tolist() == [float(ts[0])] * 2
    for k, m in enumerate(c["ms"]):
        keep = m.clone()
        smp.step(m, x, tbuf)
        assert torch.equal(x, c["xs"][k]), (k, rel_l2(x, c["xs"][k]))
        assert tbuf.tolist() == [float(ts[min(k + 1, len(ts) - 1)])] * 2, k
        assert torch.equal(m, keep)
    smp.step(c["ms"][0], x, tbuf)                            # beyond the end: nothing moves
    assert torch.equal(x, c["xs"][-1]) and tbuf.tolist() == [float(ts[-1])] * 2
    smp.reset(tbuf)                                          # a rewound chain on the used state reproduces the first
    x.copy_(c["x_init"])
    for k, m in enumerate(c["ms"]):
        smp.step(m, x, tbuf)
    assert torch.equal(x, c["xs"][-1])


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("mode", ["plms", "prk"])
def test_closed_form_trajectory(cuda, mode, pred):
    """x0 and eps fixed, set_alpha_to_one=True: with a model that is exact, every intermediate x is sqrt(abar') x0 + sqrt(1 - abar') eps
    and the chain ends at x0; rel-L2 <= 1e-5 (<= 59 steps of <= 1e-6, with slack).

    epsilon: the model output is the constant eps, so every multistep estimate is eps (the weights sum to 1).
    v_prediction: v = sqrt(abar) eps - sqrt(1 - abar) x0 changes with t, and PLMS mixes the v of several timesteps, so feeding v at each
    call's own effective t leaves the trajectory even in exact arithmetic (the fp64 reference ends 0.14 away from x0 at n = 10: that
    is PNDM's extrapolation error, not rounding).  The closed form holds when the multistep ESTIMATE is v at the effective t, so the
    output fed is the one that makes it so: the step is affine in the output, and two probes of a copy of the fp64 reference give
    the output that lands on the trajectory.  In the PRK calls this is v at the effective t itself."""
    n = 1003
    sch, ref = _pair(mode, pred, set_alpha_to_one=True)
    g = torch.Generator().manual_seed(7)
    x0, eps = torch.randn((n,), generator=g, dtype=torch.float64), torch.randn((n,), generator=g, dtype=torch.float64)
    ac = ref.alphas_cumprod
    ts = sch.timesteps.tolist()
    on_path = lambda a: a ** 0.5 * x0 + (1 - a) ** 0.5 * eps
    xr = on_path(float(ac[ts[0]]))
    x = xr.float().to(cuda)
    smp = sch.device_sampler()
    tbuf = torch.empty((1,), device=cuda)
    smp.reset(tbuf)
    worst = 0.0
    for k, t in enumerate(ts):
        t_eff, prev_t = ref.effective(ref.counter, t)
        want = on_path(ref.abar(prev_t))
        if pred == "epsilon":
            m = eps
        else:
            p0 = copy.deepcopy(ref).step(torch.zeros_like(x0), t, xr)[0]
            p1 = copy.deepcopy(ref).step(torch.ones_like(x0), t, xr)[0]
            m = (want - p0) / (p1 - p0)
            if k < len(ref.prk):
                a = float(ac[t_eff])
                assert rel_l2(m, a ** 0.5 * eps - (1 - a) ** 0.5 * x0) <= 1e-9
        xr, _ = ref.step(m, t, xr)
        assert rel_l2(xr, want) <= 1e-12                     # the reference is on the trajectory
        smp.step(m.float().to(cuda), x, tbuf)
        worst = max(worst, rel_l2(x, want))
    print(f"pndm closed form {mode} {pred}: worst intermediate rel-L2 {worst:.3e}, end {rel_l2(x, x0):.3e}")
    assert worst <= 1e-5 and rel_l2(x, x0) <= 1e-5


def _unet(cfg, cuda, seed=1):
    from ldm3d.networks import DiffusionModelUNet
    from oracle import unet as ou
    m = DiffusionModelUNet(**cfg)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfg), seed))
    return m.to(cuda).eval()


def _plms6(pred="epsilon"):
    from ldm3d.schedulers import PNDMScheduler
    sch = PNDMScheduler(**cfgs.SCHED, skip_prk_steps=True, set_alpha_to_one=True, prediction_type=pred)
    sch.set_timesteps(6)
    assert len(sch.timesteps) == 7
    return sch


def test_graph_replay_equals_eager_and_follows_the_state_buffer(cuda):
    m = _unet(cfgs.UNET_TINY, cuda)
    sch = _plms6()
    x0 = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=torch.Generator(device=cuda).manual_seed(2))
    x, tbuf = torch.empty_like(x0), torch.empty((1,), device=cuda)
    ts = sch.timesteps.tolist()

    def chain(smp):
        x.copy_(x0)
        smp.reset(tbuf)
        for k in range(len(ts)):
            assert tbuf.tolist() == [float(ts[k])]
            m.denoise_step(x, tbuf, smp)
        return x.clone()
    with torch.no_grad():
        m.enable_graph_replay(False)
        eager = chain(sch.device_sampler())
        assert torch.isfinite(eager).all() and not torch.equal(eager, x0)
        m.enable_graph_replay(True)
        smp = sch.device_sampler()
        first = chain(smp)
        second = chain(smp)                                  # replayed graph on a rewound state
        assert torch.equal(first, eager) and torch.equal(second, eager)
        old = smp._state
        fresh = torch.full_like(old, float("nan"))
        smp.bind_state(fresh, x.numel())                     # same sampler, same tensors, another state buffer: another graph key
        old.fill_(float("nan"))                              # a replay of the recorded graph would read this
        third = chain(smp)
        fourth = chain(smp)
        assert torch.equal(third, eager) and torch.equal(fourth, eager)
        assert torch.isnan(old).all() and not torch.isnan(fresh[:x.numel()]).any()
        m.enable_graph_replay(False)


def test_sliding_window_equals_the_unfused_path(cuda):
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.sliding import WindowGrid
    m = _unet(cfgs.UNET_TINY, cuda)
    for pred in ("epsilon", "v_prediction"):
        sch = _plms6(pred)
        inf = LatentDiffusionInferer(sch)
        noise = torch.randn((1, 4, 8, 8, 12), device=cuda, generator=torch.Generator(device=cuda).manual_seed(4))
        grid = WindowGrid((8, 8, 12), 8)
        assert grid.n_windows == 2
        with torch.no_grad():
            fused = inf.sample_sliding_window(noise, None, m, (8, 8, 8), sw_batch_size=2, fused_seed=0)
            stepper = sch.chain_scheduler()
            x = noise
            for t in sch.timesteps.tolist():
                tb = torch.full((2,), float(t), device=cuda)
                out_w = m(x=grid.gather(x), timesteps=tb, context=None).clone()
                x, _ = stepper.step(grid.blend(out_w), t, x)
            assert torch.equal(fused, x), (pred, rel_l2(fused, x))
            assert torch.isfinite(fused).all() and not torch.equal(fused, noise)
            host = inf.sample_sliding_window(noise, None, m, (8, 8, 8), sw_batch_size=2)      # the inferer's own host loop
            assert torch.equal(host, x)
    with torch.no_grad():                                    # one window covering the latent == sample
        one = noise[..., :8].contiguous()
        a = inf.sample_sliding_window(one, None, m, (8, 8, 8), fused_seed=0)
        b = inf.sample(one, None, m, fused_seed=0)
        c = inf.sample(one, None, m)                         # and the host-driven loop of sample: PNDM draws nothing
        assert torch.equal(a, b) and torch.equal(b, c)


def test_argument_errors_launch_nothing(cuda):
    from ldm3d import _lib
    L = _lib.lib()
    sch = _plms6()
    n = 1003
    g = torch.Generator(device=cuda).manual_seed(6)
    x, m = torch.randn((n,), device=cuda, generator=g), torch.randn((n,), device=cuda, generator=g)
    x_keep = x.clone()
    tbuf = torch.empty((1,), device=cuda)
    smp = sch.device_sampler()
    smp.reset(tbuf)
    first_t = tbuf.tolist()
    raw = lambda n_: L.ldm_sampler_step(smp._h, m.data_ptr(), x.data_ptr(), None, n_, tbuf.data_ptr(), 1, _lib.current_stream())
    assert raw(n) == -1 and b"ldm_sampler_bind_state" in L.ldm_last_error()         # no state buffer bound
    with pytest.raises(_lib.LdmError, match="state buffer"):
        smp.bind_state(torch.empty((6 * n - 1,), device=cuda), n)                  # too small
    assert raw(n) == -1                                                              # ... and still unbound
    assert smp.state_numel(n) == 6 * n
    smp.bind_state(torch.empty((6 * n,), device=cuda), n)
    with pytest.raises(_lib.LdmError, match="x0_out"):
        smp.step(m, x, tbuf, x0_out=torch.empty_like(x))                            # PNDM has no x0_hat
    assert raw(n - 1) == -1 and b"bound for" in L.ldm_last_error()                  # a step of another size than the bound state
    unet = _unet(cfgs.UNET_TINY, cuda)
    lat = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g)
    lat_keep = lat.clone()
    ws = torch.empty((L.ldm_unet_workspace_bytes(unet._h, 1, 8, 8, 8),), dtype=torch.uint8, device=cuda)
    scratch = torch.empty_like(lat)
    bare = sch.device_sampler()
    rc = L.ldm_unet_denoise_step(unet._h, bare._h, lat.data_ptr(), 4, None, 0, tbuf.data_ptr(), scratch.data_ptr(), 1, 8, 8, 8,
                                 ws.data_ptr(), ws.numel(), _lib.current_stream())
    assert rc == -1 and b"ldm_sampler_bind_state" in L.ldm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, x_keep) and torch.equal(lat, lat_keep) and tbuf.tolist() == first_t
    # nothing advanced the counter either: the first real step is step 0
    want, _ = sch.chain_scheduler().step(m, sch.timesteps[0], x)
    smp.step(m, x, tbuf)
    assert torch.equal(x, want) and tbuf.tolist() == [float(sch.timesteps[1])]
    from ldm3d.schedulers import DDIMScheduler
    ddim = DDIMScheduler(**cfgs.SCHED).device_sampler()
    assert ddim.state_numel(n) == 0
    with pytest.raises(_lib.LdmError):
        ddim.bind_state(torch.empty((8,), device=cuda), 1)


def test_inference_cli_samples_with_pndm(tmp_path):
    env = {"data_base_dir": str(tmp_path / "data"), "model_dir": str(tmp_path / "ckpt"), "output_dir": str(tmp_path / "out"),
           "resume_ckpt": False, "seed": 0}
    env_file = str(tmp_path / "environment.json")
    with open(env_file, "w") as fh:
        json.dump(env, fh)
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-e", env_file, "-c", os.path.join(ROOT, "config", "config_synthetic_24.json"),
           "-n", "1", "--random-init", "--sampler", "pndm", "--steps", "6"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    vols = sorted((tmp_path / "out").glob("*.nii"))
    assert len(vols) == 1
    data = np.fromfile(vols[0], dtype=np.float32, offset=352)
    assert data.size == 96 ** 3 and np.isfinite(data).all() and float(data.std()) > 0.0
    bad = subprocess.run(cmd[:-2], cwd=ROOT, capture_output=True, text=True, timeout=600)      # pndm without --steps
    assert bad.returncode != 0 and "--steps" in bad.stderr
