"""prediction_type "sample" / "v_prediction" on the host (no GPU): scheduler construction, the device sampler's coefficient rows
against a float64 restatement, and the entry points reading NoiseScheduler.prediction_type."""
import os
import sys
import types

import pytest
import torch

import cfgs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ("epsilon", "sample", "v_prediction")


@pytest.mark.parametrize("pred", TYPES)
def test_schedulers_construct_with_each_prediction_type(built_lib, pred):
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler
    for cls in (DDPMScheduler, DDIMScheduler):
        sch = cls(**cfgs.SCHED, prediction_type=pred)
        assert sch.prediction_type == pred


def test_unknown_prediction_type_raises_value_error(built_lib):
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler
    for cls in (DDPMScheduler, DDIMScheduler):
        with pytest.raises(ValueError, match="prediction_type"):
            cls(**cfgs.SCHED, prediction_type="velocity")
        with pytest.raises(ValueError):
            cls(**cfgs.SCHED, prediction_type="learned")


def _abar64():
    T = cfgs.SCHED["num_train_timesteps"]
    betas = torch.linspace(cfgs.SCHED["beta_start"] ** 0.5, cfgs.SCHED["beta_end"] ** 0.5, T, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, dim=0), betas


@pytest.mark.parametrize("pred", ["sample", "v_prediction"])
@pytest.mark.parametrize("kind,eta", [("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.7)])
def test_sampler_rows_match_a_float64_restatement(built_lib, pred, kind, eta):
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler, _sampler_rows
    if kind == "ddpm":
        sch = DDPMScheduler(**cfgs.SCHED, prediction_type=pred)
    else:
        sch = DDIMScheduler(**cfgs.SCHED, prediction_type=pred)
        sch.set_timesteps(20)
    k, rows = _sampler_rows(sch, eta)
    assert k == (0 if kind == "ddpm" else 1)
    ts = [int(t) for t in sch.timesteps.tolist()]
    assert len(rows) == len(ts) and all(len(r) == 8 for r in rows)
    ac, betas = _abar64()
    ratio = sch.num_train_timesteps // sch.num_inference_steps
    for r, t in zip(rows, ts):
        a = float(ac[t])
        if kind == "ddpm":
            a_prev = float(ac[t - 1]) if t > 0 else 1.0
            beta = float(betas[t])
            var = max((1 - a_prev) / (1 - a) * beta, 1e-20)
            want = [1 / a ** 0.5, (1 - a) ** 0.5, a_prev ** 0.5 * beta / (1 - a), (1 - beta) ** 0.5 * (1 - a_prev) / (1 - a),
                    var ** 0.5 if t > 0 else 0.0, t, a ** 0.5, 1 / (1 - a) ** 0.5]
        else:
            a_prev = float(ac[t - ratio]) if t - ratio >= 0 else 1.0
            std = eta * ((1 - a_prev) / (1 - a) * (1 - a / a_prev)) ** 0.5
            want = [1 / a ** 0.5, (1 - a) ** 0.5, a_prev ** 0.5, max(1 - a_prev - std ** 2, 0.0) ** 0.5, std, t, a ** 0.5,
                    1 / (1 - a) ** 0.5]
        # the rows are MONAI's fp32 arithmetic: the fp32 cumprod, and 1 - abar_t loses digits where abar_t is close to 1, so the
        # bound scales with 1 / (1 - abar_t) (the DDIM direction of the last step is ~0: absolute there)
        tol = 2e-6 * (1.0 + 1.0 / (1.0 - a))
        for j, (g, w) in enumerate(zip(r, want)):
            assert abs(g - w) <= tol * abs(w) + 1e-6, (kind, t, j, g, w)
        assert r[5] == float(t)


def test_epsilon_rows_are_the_existing_six_coefficients(built_lib):
    """The first six entries of an epsilon row are the by-value scalars of the DDPM tables (the last two are not read for epsilon)."""
    from ldm3d.schedulers import DDPMScheduler, _sampler_rows
    sch = DDPMScheduler(**cfgs.SCHED)
    _, rows = _sampler_rows(sch)
    t = int(sch.timesteps[3])
    assert rows[3][:6] == [sch._inv_sqrt_a[t], sch._sqrt_b[t], sch._c0[t], sch._c1[t], sch._sigma[t], float(t)]


@pytest.mark.parametrize("nsteps", [50, 1000])
def test_step_rows_equal_the_scalars_the_epsilon_step_used_to_compute(built_lib, nsteps):
    """``step`` passes ``_row(t, eta)`` to ldm_scheduler_step.  Before the DDPM / DDIM step kernels were folded into one, the epsilon
    ``step`` of each scheduler computed its five scalars by hand; those expressions are restated here and every row must equal them
    with ``==``, for every timestep of the schedule, so the fold changed no coefficient."""
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler
    ddpm = DDPMScheduler(**cfgs.SCHED)
    ddpm.set_timesteps(nsteps)
    for t in ddpm.timesteps.tolist():
        old = [ddpm._inv_sqrt_a[t], ddpm._sqrt_b[t], ddpm._c0[t], ddpm._c1[t], ddpm._sigma[t] if t > 0 else 0.0]
        assert ddpm._row(t)[:5] == old, t
    ddim = DDIMScheduler(**cfgs.SCHED)
    ddim.set_timesteps(nsteps)
    for eta in (0.0, 0.5, 1.0):
        for t in ddim.timesteps.tolist():
            prev_t = t - ddim.num_train_timesteps // ddim.num_inference_steps
            a_t = ddim.alphas_cumprod[t]
            a_prev = ddim.alphas_cumprod[prev_t] if prev_t >= 0 else ddim.final_alpha_cumprod
            b_t = 1 - a_t
            var = (1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)
            std = eta * var ** 0.5
            direction = (1 - a_prev - std ** 2) ** 0.5
            old = [float(1.0 / a_t ** 0.5), float(b_t ** 0.5), float(a_prev ** 0.5), float(direction), float(std)]
            assert ddim._row(t, eta)[:5] == old, (eta, t)
            assert all(v == v for v in old), (eta, t)                  # no NaN: == above compared numbers


def _import_entry(name):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import importlib
    return importlib.import_module(name)


@pytest.mark.parametrize("pred", [None, "sample", "v_prediction"])
@pytest.mark.parametrize("steps", [0, 10])
def test_inference_make_scheduler_reads_prediction_type(built_lib, pred, steps):
    inference = _import_entry("inference")
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler
    section = {"num_train_timesteps": 1000, "beta_start": 0.0015, "beta_end": 0.0195}
    if pred is not None:
        section["prediction_type"] = pred
    sch = inference.make_scheduler(types.SimpleNamespace(NoiseScheduler=section, steps=steps))
    assert isinstance(sch, DDIMScheduler if steps else DDPMScheduler)
    assert sch.prediction_type == (pred or "epsilon")


@pytest.mark.parametrize("pred", [None, "v_prediction"])
def test_train_diffusion_scheduler_args_read_prediction_type(built_lib, pred):
    train_diffusion = _import_entry("train_diffusion")
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler
    section = {"num_train_timesteps": 1000, "beta_start": 0.0015, "beta_end": 0.0195}
    if pred is not None:
        section["prediction_type"] = pred
    kw = train_diffusion.scheduler_args(section)
    assert kw["prediction_type"] == (pred or "epsilon")
    # the training DDPM schedule and the validation DDIM schedule are both built from these
    assert DDPMScheduler(**kw).prediction_type == kw["prediction_type"]
    assert DDIMScheduler(**kw).prediction_type == kw["prediction_type"]
