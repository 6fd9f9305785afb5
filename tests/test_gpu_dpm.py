"""DPMSolverMultistepScheduler on the GPU (-m gpu): the host-driven step against the fp64 restatement (tests/dpm_ref.py), the device
sampler against the host-driven step bit for bit, the closed-form trajectory, graph replay, sliding windows, guidance, argument errors
and the CLI.

Sizes: 1 element, 1003 (ragged last quad) and 4 * 256 * 1024 + 5 (every thread of the 1024-block grid wraps once, then a tail)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cfgs
from dpm_ref import DPMRef
from util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SIZES = [1, 1003, 4 * 256 * 1024 + 5]
PREDS = ["epsilon", "sample", "v_prediction"]
ALGOS = {"ode": "dpmsolver++", "sde": "sde-dpmsolver++"}
SEED = 5


def _pair(n_steps, pred, order=2, algo="ode", **kw):
    from ldm3d.schedulers import DPMSolverMultistepScheduler
    args = dict(cfgs.SCHED, prediction_type=pred, solver_order=order, algorithm_type=ALGOS[algo], **kw)
    sch, ref = DPMSolverMultistepScheduler(**args), DPMRef(**args)
    sch.set_timesteps(n_steps)
    ref.set_timesteps(n_steps)
    assert sch.timesteps.tolist() == ref.ts
    return sch, ref


def _cancelled(row, pred, x, m, prev, z, limit=2.0):
    """Whether the step of ONE element is ill-conditioned: sum |parts| / |sum| above ``limit`` in x0_hat's conversion or in the update
    with x0_hat written out in its parts, evaluated in fp64 on the host's row (tests/test_dpm_cpu.py pins it to the reference), never on
    the kernel under test."""
    cx, c0, sa, sb, _flags, _t, c1, cz = row[:8]
    x, m = float(x), float(m)
    parts0 = {"sample": [m], "epsilon": [x / sa, -sb * m / sa], "v_prediction": [sa * x, -sb * m]}[pred]
    parts = [cx * x] + [c0 * p for p in parts0] + [c1 * (0.0 if prev is None else float(prev)), cz * (0.0 if z is None else float(z))]
    cond = lambda ps: sum(abs(p) for p in ps) / max(abs(sum(ps)), 1e-300)
    return cond(parts0) > limit or cond(parts) > limit


@functools.lru_cache(maxsize=None)
def _one_element_inputs(pred, order, algo):
    """(x_init, [m_k], [z_k]) of a one-element chain of 10 calls whose every step is well-conditioned.  The relative error of a single
    scalar is its rounding error times the condition number of the sum that forms it, and a random draw cancels every few steps (a
    step is a sum of up to five signed parts); the rel-L2 gate is a statement about vectors, where the norm averages that out.  So the
    draws of (m, z) are repeated (CPU generator, fp64 reference and host row only) until neither x0_hat's conversion nor the update
    is cancelled (``_cancelled``: sum |parts| / |sum| <= 2).  With u = 2^-24 that bounds the error: every part carries at most three
    roundings (its coefficients, its product), the sums round at most three times more, each relative to at most sum |parts|:
    (3 u + 3 u) * 2 = 12 u = 7.2e-7 <= 1e-6.  So n = 1 checks the launch and the arithmetic rather than the draw; the gate is the same
    for every size."""
    sch, ref = _pair(10, pred, order, algo)
    g = torch.Generator().manual_seed(31)
    x_init = torch.randn((1,), generator=g)
    xr, ms, zs = x_init.double(), [], []
    for k, t in enumerate(ref.ts):
        row = sch._row(k)
        has_prev, draws = int(row[4]) & 1, int(row[4]) & 2
        for _ in range(2000):
            m, z = torch.randn((1,), generator=g), torch.randn((1,), generator=g) if draws else None
            if not _cancelled(row, pred, xr, m, ref.prev_x0 if has_prev else None, z):
                break
        else:
            raise AssertionError(f"no well-conditioned draw for call {k} in 2000 tries")
        ms.append(m)
        zs.append(z)
        xr, x0r = ref.step(m.double(), t, xr, None if z is None else z.double())
        xr, ref.prev_x0 = xr.float().double(), x0r.float().double()
    return x_init, ms, zs


@functools.lru_cache(maxsize=None)
def _chain(pred, order, algo, n, conditioned=False):
    """One whole chain of N = 10 calls, computed once per case and shared: the model outputs, the draws, the free-running host-driven
    chain, its x0_hat, the fp64 reference chain, and the per-step error of the step fed from the reference's state.  The model outputs
    are random and the draws the device sampler's own, so that the same chain serves the bit-for-bit test; ``conditioned`` (n = 1): the
    inputs of ``_one_element_inputs``, draws included.

    The reference chain continues from its own state ROUNDED to fp32 (x and the kept x0_hat), so the step under test and the reference
    see the same inputs and the error measured is the step's arithmetic alone."""
    dev = torch.device("cuda:0")
    sch, ref = _pair(10, pred, order, algo)
    fed = sch.chain_scheduler()
    smp = sch.device_sampler(SEED)
    g = torch.Generator(device=dev).manual_seed(2000 + n % 997)
    x_init = torch.randn((n,), device=dev, generator=g)
    given = None
    if conditioned:
        assert n == 1
        given = _one_element_inputs(pred, order, algo)
        x_init = given[0].to(dev)
    ts = sch.timesteps.tolist()
    ms, zs, xs, x0s, step_err = [], [], [], [], []
    x, xr = x_init, x_init.double().cpu()
    for k, t in enumerate(ts):
        if given is None:
            m = torch.randn((n,), device=dev, generator=g)
            z = smp.noise(k, (n,), dev) if algo == "sde" else None
        else:
            m, z = given[1][k].to(dev), None if given[2][k] is None else given[2][k].to(dev)
        ms.append(m)
        zs.append(z)
        fed.counter, fed.prev_x0 = ref.counter, None if ref.prev_x0 is None else ref.prev_x0.float().to(dev)
        got, got_x0 = fed.step(m, t, xr.float().to(dev), noise=z)
        x, x0 = sch.step(m, t, x, noise=z)
        xs.append(x)
        x0s.append(x0)
        xr, x0r = ref.step(m.double().cpu(), t, xr, None if z is None else z.double().cpu())
        step_err.append(max(rel_l2(got, xr), rel_l2(got_x0, x0r)))
        xr, ref.prev_x0 = xr.float().double(), x0r.float().double()
    return dict(sch=sch, ts=ts, x_init=x_init, ms=ms, zs=zs, xs=xs, x0s=x0s, ref_end=xr, step_err=step_err)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("algo", list(ALGOS))
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("pred", PREDS)
def test_host_driven_step_matches_fp64(cuda, pred, order, algo, n):
    """Every step, from the reference's state (rounded to fp32): rel-L2 <= 1e-6 (the project's scheduler gate) for x and x0_hat.  The
    end-of-chain error of the chain that runs on its own fp32 state is reported, not gated.  n = 1 runs on ``_one_element_inputs``."""
    c = _chain(pred, order, algo, n, n == 1)
    end = rel_l2(c["xs"][-1], c["ref_end"])
    print(f"dpm {pred} order {order} {algo} n={n}: max per-step rel-L2 {max(c['step_err']):.3e}, end of chain (10 calls) {end:.3e}")
    assert len(c["step_err"]) == 10
    assert max(c["step_err"]) <= 1e-6, c["step_err"]
    assert torch.isfinite(c["xs"][-1]).all()
    assert torch.equal(c["xs"][-1], c["x0s"][-1])            # the last call: x := x0_hat


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("algo", list(ALGOS))
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("pred", PREDS)
def test_fused_sampler_equals_host_driven_bitwise(cuda, pred, order, algo, n):
    c = _chain(pred, order, algo, n)
    sch, ts = c["sch"], c["ts"]
    smp = sch.device_sampler(SEED)
    assert smp.n_steps == len(ts) and smp.state_numel(n) == n
    x = c["x_init"].clone()
    x0_out = torch.full((n,), float("nan"), device=cuda)
    tbuf = torch.full((2,), -1.0, device=cuda)
    smp.reset(tbuf)
    assert tbuf.tolist() == [float(ts[0])] * 2
    for k, m in enumerate(c["ms"]):
        keep = m.clone()
        smp.step(m, x, tbuf, x0_out=x0_out)
        assert torch.equal(x, c["xs"][k]), (k, rel_l2(x, c["xs"][k]))
        assert torch.equal(x0_out, c["x0s"][k]), k
        assert tbuf.tolist() == [float(ts[min(k + 1, len(ts) - 1)])] * 2, k
        assert torch.equal(m, keep)
    smp.step(c["ms"][0], x, tbuf, x0_out=x0_out)             # beyond the end: nothing moves
    assert torch.equal(x, c["xs"][-1]) and torch.equal(x0_out, c["x0s"][-1]) and tbuf.tolist() == [float(ts[-1])] * 2
    smp.reset(tbuf)                                          # a rewound chain on the used state reproduces the first
    x.copy_(c["x_init"])
    for k, m in enumerate(c["ms"]):
        smp.step(m, x, tbuf)
    assert torch.equal(x, c["xs"][-1])
    if algo == "sde":                                        # the draws are the sampler's stream, step by step, and they matter
        other = sch.device_sampler(SEED + 1)
        assert not torch.equal(other.noise(0, (n,), cuda), c["zs"][0])
        assert torch.equal(sch.device_sampler(SEED).noise(3, (n,), cuda), c["zs"][3])


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("pred", PREDS)
def test_closed_form_trajectory(cuda, pred, order):
    """x0* and eps* fixed, a model that returns the exact eps, x0 or v of the pair at each call's timestep: every iterate of the device
    chain is alpha_t x0* + sigma_t eps* and the chain ends at x0*; rel-L2 <= 1e-5 (<= 50 steps of <= 1e-6, with slack).  |x0*| <= 0.9,
    so clip_sample=True changes nothing, bit for bit.

    N = 10, the chain length of the other device tests.  The count of steps is not what sets the error here: a model whose output
    does not depend on x is an open loop, and with prediction_type "epsilon" the step's derivative dx_t / dx_s = cx + c0 / alpha_s is
    alpha_t / alpha_s > 1, so the rounding of the START is carried to the end multiplied by 1 / alpha_0 = 1 / sqrt(abar_999) = 71 on
    this schedule, in any fp32 arithmetic.  The same chain in plain fp32 on the CPU (numpy, no fused multiply-add) gives for epsilon
    6.5e-6 at N = 10, 7.5e-6 at N = 20 and 1.2e-5 at N = 50 (order 1; order 2 6.7e-6 / 8.6e-6 / 1.3e-5), against <= 6e-7 for the other
    two types at every N; this kernel measured 1.002e-5 at N = 50, epsilon, order 1: over the bound by rounding luck, like the plain
    fp32 chain.  A trained model is a closed loop and does not amplify that way; the bound is kept and the chain is the 10-call one."""
    n, n_steps = 1003, 10
    g = torch.Generator().manual_seed(7)
    x0s = 0.9 * torch.tanh(torch.randn((n,), generator=g, dtype=torch.float64))
    epss = torch.randn((n,), generator=g, dtype=torch.float64)
    ends = []
    for clip in (False, True):
        sch, ref = _pair(n_steps, pred, order, clip_sample=clip)
        a0, s0 = ref.alpha_sigma(0)
        x = (a0 * x0s + s0 * epss).float().to(cuda)
        smp = sch.device_sampler()
        tbuf = torch.empty((1,), device=cuda)
        smp.reset(tbuf)
        worst = 0.0
        for k in range(n_steps):
            a, s = ref.alpha_sigma(k)
            m = {"epsilon": epss, "sample": x0s, "v_prediction": a * epss - s * x0s}[pred]
            smp.step(m.float().to(cuda), x, tbuf)
            a, s = ref.alpha_sigma(k + 1)
            worst = max(worst, rel_l2(x, a * x0s + s * epss))
        print(f"dpm closed form {pred} order {order} clip {clip}: worst intermediate rel-L2 {worst:.3e}, end {rel_l2(x, x0s):.3e}")
        assert worst <= 1e-5 and rel_l2(x, x0s) <= 1e-5
        ends.append(x.clone())
    assert torch.equal(ends[0], ends[1])


def _unet(cfg, cuda, seed=1):
    from ldm3d.networks import DiffusionModelUNet
    from oracle import unet as ou
    m = DiffusionModelUNet(**cfg)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfg), seed))
    return m.to(cuda).eval()


def _dpm6(pred="epsilon", algo="ode"):
    from ldm3d.schedulers import DPMSolverMultistepScheduler
    sch = DPMSolverMultistepScheduler(**cfgs.SCHED, prediction_type=pred, algorithm_type=ALGOS[algo])
    sch.set_timesteps(6)
    assert len(sch.timesteps) == 6
    return sch


@pytest.mark.parametrize("algo", list(ALGOS))
def test_graph_replay_equals_eager_and_follows_the_state_buffer(cuda, algo):
    m = _unet(cfgs.UNET_TINY, cuda)
    sch = _dpm6(algo=algo)
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
        eager = chain(sch.device_sampler(SEED))
        assert torch.isfinite(eager).all() and not torch.equal(eager, x0)
        # forward, then the host-driven step on the sampler's own draws
        stepper, probe = sch.chain_scheduler(), sch.device_sampler(SEED)
        xh = x0
        for k, t in enumerate(ts):
            out = m(x=xh, timesteps=torch.full((1,), float(t), device=cuda), context=None).clone()
            xh, _ = stepper.step(out, t, xh, noise=probe.noise(k, xh.shape, cuda))
        assert torch.equal(eager, xh), rel_l2(eager, xh)
        m.enable_graph_replay(True)
        try:
            smp = sch.device_sampler(SEED)
            first = chain(smp)
            second = chain(smp)                              # replayed graph on a rewound state
            assert torch.equal(first, eager) and torch.equal(second, eager)
            old = smp._state
            fresh = torch.full_like(old, float("nan"))
            smp.bind_state(fresh, x.numel())                 # same sampler, same tensors, another state buffer: another graph key
            old.fill_(float("nan"))                          # a replay of the recorded graph would read this
            third = chain(smp)
            fourth = chain(smp)
            assert torch.equal(third, eager) and torch.equal(fourth, eager)
            assert torch.isnan(old).all() and not torch.isnan(fresh).any()
        finally:
            m.enable_graph_replay(False)


def test_sliding_window_equals_the_unfused_path(cuda):
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.sliding import WindowGrid
    m = _unet(cfgs.UNET_TINY, cuda)
    noise = torch.randn((1, 4, 8, 8, 12), device=cuda, generator=torch.Generator(device=cuda).manual_seed(4))
    grid = WindowGrid((8, 8, 12), 8)
    assert grid.n_windows == 2
    for pred in PREDS:
        sch = _dpm6(pred)
        inf = LatentDiffusionInferer(sch)
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
    with torch.no_grad():                                    # one window covering the latent == sample, fused == host-driven
        one = noise[..., :8].contiguous()
        a = inf.sample_sliding_window(one, None, m, (8, 8, 8), fused_seed=0)
        b = inf.sample(one, None, m, fused_seed=0)
        c = inf.sample(one, None, m)                         # the ODE form draws nothing
        assert torch.equal(a, b) and torch.equal(b, c)


def test_one_guided_step_equals_host_combine_then_host_step(cuda):
    from ldm3d import _lib
    m = _unet(cfgs.UNET_TINY_COND, cuda, seed=3)
    g = torch.Generator(device=cuda).manual_seed(11)
    x0, cond = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g), torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g)
    w, fill = 3.5, -1.0
    for algo in ALGOS:
        sch = _dpm6("v_prediction", algo)
        ts = sch.timesteps.tolist()
        with torch.no_grad():
            smp = sch.device_sampler(SEED)
            x, tbuf = x0.clone(), torch.empty((2,), device=cuda)
            smp.reset(tbuf)
            stepper, xh = sch.chain_scheduler(), x0
            for k in range(2):                               # a first-order step, then a second-order one on the kept x0_hat
                out = m(x=torch.cat([xh, xh]), timesteps=torch.full((2,), float(ts[k]), device=cuda), context=None,
                        cond=torch.cat([torch.full_like(cond, fill), cond]))
                guided = torch.empty_like(xh)
                _lib.check(_lib.lib().ldm_guidance_combine(out[:1].data_ptr(), out[1:].data_ptr(), w, guided.data_ptr(), guided.numel(),
                                                           _lib.current_stream()))
                xh, _ = stepper.step(guided, ts[k], xh, noise=smp.noise(k, xh.shape, cuda))
                m.denoise_step(x, tbuf, smp, cond=cond, guidance=w, guidance_fill=fill)
                assert torch.equal(x, xh), (algo, k, rel_l2(x, xh))
                assert tbuf.tolist() == [float(ts[k + 1])] * 2
            assert smp._state_n == x.numel() and smp.state_numel(x.numel()) == x.numel()      # the state of B samples, not 2 B


def test_argument_errors_launch_nothing(cuda):
    from ldm3d import _lib
    L = _lib.lib()
    sch = _dpm6(algo="sde")
    n = 1003
    g = torch.Generator(device=cuda).manual_seed(6)
    x, m = torch.randn((n,), device=cuda, generator=g), torch.randn((n,), device=cuda, generator=g)
    x_keep = x.clone()
    tbuf = torch.empty((1,), device=cuda)
    smp = sch.device_sampler(SEED)
    smp.reset(tbuf)
    first_t = tbuf.tolist()
    raw = lambda n_: L.ldm_sampler_step(smp._h, m.data_ptr(), x.data_ptr(), None, n_, tbuf.data_ptr(), 1, _lib.current_stream())
    assert raw(n) == -1 and b"ldm_sampler_bind_state" in L.ldm_last_error()         # no state buffer bound
    with pytest.raises(_lib.LdmError, match="state buffer"):
        smp.bind_state(torch.empty((n - 1,), device=cuda), n)                      # too small
    assert raw(n) == -1                                                              # ... and still unbound
    assert smp.state_numel(n) == n
    smp.bind_state(torch.empty((n,), device=cuda), n)
    assert raw(n - 1) == -1 and b"bound for" in L.ldm_last_error()                  # a step of another size than the bound state
    with pytest.raises(_lib.LdmError, match="first row"):
        smp.seek(1, tbuf)                                                            # the row program assumes the history from row 0
    smp.seek(0, tbuf)
    with pytest.raises(_lib.LdmError, match="warm start"):
        smp.start(x.reshape(1, -1), 0, 1)
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        sch.repaint_sampler(x.reshape(1, 1, 17, 59, 1), torch.ones((17, 59, 1), device=cuda))
    rows = torch.tensor(sch._dpm_rows(), dtype=torch.float32)
    import ctypes as C
    hh = C.c_void_p()
    assert L.ldm_sampler_create_repaint(rows.data_ptr(), len(rows), 4, 0, 0, 0, C.byref(hh)) == -1 and not hh.value
    # the row program is checked when the sampler is created
    for slot, value, word in ((4, float(int(rows[0, 4]) | 1), b"row 0"), (0, float("nan"), b"not finite"), (7, -0.5, b"negative")):
        bad = rows.clone()
        bad[0, slot] = value
        assert L.ldm_sampler_create_dpm(bad.data_ptr(), len(bad), 0, 0, C.byref(hh)) == -1 and word in L.ldm_last_error() and not hh.value
    bad = rows.clone()
    bad[1, 7] = 0.0                                                                  # DRAWS with cz == 0
    assert L.ldm_sampler_create_dpm(bad.data_ptr(), len(bad), 0, 0, C.byref(hh)) == -1 and b"DRAWS" in L.ldm_last_error()
    assert L.ldm_sampler_create_dpm(rows.data_ptr(), len(rows), 3, 0, C.byref(hh)) == -1
    unet = _unet(cfgs.UNET_TINY, cuda)
    lat = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g)
    lat_keep = lat.clone()
    ws = torch.empty((L.ldm_unet_workspace_bytes(unet._h, 1, 8, 8, 8),), dtype=torch.uint8, device=cuda)
    scratch = torch.empty_like(lat)
    bare = sch.device_sampler(SEED)
    rc = L.ldm_unet_denoise_step(unet._h, bare._h, lat.data_ptr(), 4, None, 0, tbuf.data_ptr(), scratch.data_ptr(), 1, 8, 8, 8,
                                 ws.data_ptr(), ws.numel(), _lib.current_stream())
    assert rc == -1 and b"ldm_sampler_bind_state" in L.ldm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, x_keep) and torch.equal(lat, lat_keep) and tbuf.tolist() == first_t
    # nothing advanced the counter either: the first real step is step 0
    want, want_x0 = sch.chain_scheduler().step(m, sch.timesteps[0], x, noise=smp.noise(0, x.shape, cuda))
    x0_out = torch.empty_like(x)
    smp.step(m, x, tbuf, x0_out=x0_out)
    assert torch.equal(x, want) and torch.equal(x0_out, want_x0) and tbuf.tolist() == [float(sch.timesteps[1])]
    # the inferer's refusals
    from ldm3d.inferer import LatentDiffusionInferer
    inf = LatentDiffusionInferer(sch)
    z = torch.randn((1, 4, 8, 8, 8), device=cuda, generator=g)
    with pytest.raises(NotImplementedError, match="warm starts"):
        inf.sample(z, None, unet, init_latent=z, start_step=1)
    with pytest.raises(NotImplementedError, match="inpainting"):
        inf.sample(z, None, unet, inpaint_latent=z, keep_mask=torch.ones((8, 8, 8), device=cuda))
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        inf.invert(z, unet)
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        inf.get_likelihood(z, None, unet)


def _cli(tmp_path, name, *extra):
    out = tmp_path / name
    env = {"data_base_dir": str(tmp_path / "data"), "model_dir": str(tmp_path / "ckpt"), "output_dir": str(out), "resume_ckpt": False,
           "seed": 0}
    env_file = str(tmp_path / f"{name}.json")
    with open(env_file, "w") as fh:
        json.dump(env, fh)
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-e", env_file, "-c", os.path.join(ROOT, "config", "config_synthetic_24.json"),
           "-n", "1", "--random-init", "--sampler", "dpm", "--steps", "4", *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    return r, sorted(out.glob("*.nii"))


def _volume(path):
    data = np.fromfile(path, dtype=np.float32, offset=352)
    assert data.size == 96 ** 3 and np.isfinite(data).all() and float(data.std()) > 0.0
    return data


def test_inference_cli_samples_with_dpm(tmp_path):
    r, vols = _cli(tmp_path, "ode")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len(vols) == 1
    ode = _volume(vols[0])
    r, again = _cli(tmp_path, "ode2")
    assert r.returncode == 0 and len(again) == 1
    assert np.array_equal(_volume(again[0]), ode)            # the same seed: the same volume
    r, vols = _cli(tmp_path, "sde", "--dpm-sde")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len(vols) == 1 and not np.array_equal(_volume(vols[0]), ode)


def test_inference_cli_refusals(tmp_path):
    """Argument errors: the parser exits before any device work."""
    r, vols = _cli(tmp_path, "warm", "--condition", str(tmp_path / "none.npz"), "--init-from-condition")
    assert r.returncode != 0 and not vols and "DPM-Solver++" in r.stderr and "--init-from-condition" in r.stderr
    r, vols = _cli(tmp_path, "inp", "--inpaint", str(tmp_path / "none.npz"), "--regenerate-box", "0:8,0:8,0:8")
    assert r.returncode != 0 and not vols and "DPM-Solver++" in r.stderr and "--inpaint" in r.stderr
    cmd_env = tmp_path / "e.json"
    cmd_env.write_text(json.dumps({"data_base_dir": ".", "model_dir": ".", "output_dir": str(tmp_path / "o"), "resume_ckpt": False, "seed": 0}))
    base = [sys.executable, os.path.join(ROOT, "inference.py"), "-e", str(cmd_env), "-c", os.path.join(ROOT, "config", "config_synthetic_24.json"),
            "-n", "1", "--random-init"]
    bad = subprocess.run(base + ["--sampler", "dpm"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--steps" in bad.stderr
    bad = subprocess.run(base + ["--steps", "4", "--dpm-sde"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--sampler dpm" in bad.stderr
