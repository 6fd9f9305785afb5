"""DPMSolverMultistepScheduler on the host (no GPU): the coefficient-row table the step kernels are programmed by against the fp64
restatement tests/dpm_ref.py call by call, known answers (DDIM at order 1, the trajectory of an exact model, a closed-form linear
ODE that tells the orders apart), the timestep grids, argument checks and the stateful step's misuse.

``apply_row`` is the row format's definition (csrc/norm_elem.h), evaluated in fp64 on the fp64 row ``_row`` returns before it is stored
as fp32."""
import numpy as np
import pytest
import torch

import cfgs
from dpm_ref import DPMRef, timesteps

HAS_PREV, DRAWS, CLIP = 1, 2, 4
PREDS = ["epsilon", "sample", "v_prediction"]
ALGOS = ["dpmsolver++", "sde-dpmsolver++"]
SPACINGS = ["linspace", "leading", "trailing"]


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def apply_row(row, pred, x, m, prev, z):
    """One call of the row program in fp64 -> (x', x0_hat)."""
    cx, c0, sa, sb, flags, _t, c1, cz, isa, lo, hi = row[:11]
    flags = int(flags)
    assert row[11:] == [0.0] * 5 and len(row) == 16
    if pred == "sample":
        x0 = m
    elif pred == "epsilon":
        x0 = (x - sb * m) * isa
    else:
        x0 = sa * x - sb * m
    if flags & CLIP:
        x0 = x0.clamp(lo, hi)
    out = cx * x + c0 * x0
    if flags & HAS_PREV:
        out = out + c1 * prev
    else:
        assert c1 == 0.0
    if flags & DRAWS:
        out = out + cz * z
    else:
        assert cz == 0.0
    return out, x0


def _pair(n, **kw):
    from ldm3d.schedulers import DPMSolverMultistepScheduler
    args = dict(cfgs.SCHED, **kw)
    sch, ref = DPMSolverMultistepScheduler(**args), DPMRef(**args)
    sch.set_timesteps(n)
    ref.set_timesteps(n)
    assert sch.timesteps.tolist() == ref.ts and sch.timesteps.dtype == torch.int64
    assert torch.equal(sch.alphas_cumprod.double(), ref.alphas_cumprod)
    return sch, ref


@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("order", [1, 2])
def test_row_table_matches_the_reference_call_by_call(order, algo, spacing, pred):
    """Every call of every chain, from the reference's state: the fp64 row applied to random (m, x, prev, z) is the reference's step to
    <= 1e-12 rel-L2.  N = 1 is one first-order step straight to x0_hat, N = 2 two first-order steps."""
    worst = 0.0
    for n in (1, 2, 3, 10, 50):
        for clip in (False, True) if n == 10 else (False,):
            sch, ref = _pair(n, solver_order=order, algorithm_type=algo, timestep_spacing=spacing, prediction_type=pred, clip_sample=clip,
                             clip_sample_min=-0.7, clip_sample_max=0.9)
            rows = sch._dpm_rows()
            assert len(rows) == n
            g = torch.Generator().manual_seed(17 * n + order)
            x = torch.randn((257,), generator=g, dtype=torch.float64)
            for k, t in enumerate(ref.ts):
                m, z = torch.randn((257,), generator=g, dtype=torch.float64), torch.randn((257,), generator=g, dtype=torch.float64)
                row, flags = rows[k], int(rows[k][4])
                second = order == 2 and 0 < k < n - 1
                assert bool(flags & HAS_PREV) == second and bool(flags & DRAWS) == (algo == ALGOS[1] and k < n - 1)
                assert bool(flags & CLIP) == clip and row[5] == float(t)
                if k == n - 1:
                    assert row[0] == 0.0 and row[1] == 1.0          # the last call: x := x0_hat
                got, got_x0 = apply_row(row, pred, x, m, ref.prev_x0, z)
                want, want_x0 = ref.step(m, t, x, z)
                worst = max(worst, rel(got, want), rel(got_x0, want_x0))
                if clip:
                    assert float(want_x0.min()) >= -0.7 and float(want_x0.max()) <= 0.9
                x = want
    print(f"dpm rows order {order} {algo} {spacing} {pred}: worst rel-L2 {worst:.3e}")
    assert worst <= 1e-12


def _run_rows(sch, pred, x, model, zs=None):
    """The chain of ``sch`` on fp64 rows with ``model(x, k) -> m``: -> the iterates after every call."""
    prev, out = None, []
    for k, row in enumerate(sch._dpm_rows()):
        x, prev = apply_row(row, pred, x, model(x, k), prev, None if zs is None else zs[k])
        out.append(x)
    return out


def test_order_one_on_the_leading_grid_is_ddim():
    """solver_order=1, "leading", no clip == DDIMScheduler(clip_sample=False, set_alpha_to_one=True) with eta = 0 on the same
    timesteps, for an arbitrary nonlinear model (DDIM's formula in fp64 on its own abar table)."""
    from ldm3d.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
    worst = 0.0
    for n in (1, 2, 10, 50):
        for pred in PREDS:
            ddim = DDIMScheduler(**cfgs.SCHED, clip_sample=False, set_alpha_to_one=True, prediction_type=pred)
            ddim.set_timesteps(n)
            sch = DPMSolverMultistepScheduler(**cfgs.SCHED, solver_order=1, timestep_spacing="leading", prediction_type=pred)
            sch.set_timesteps(n)
            assert sch.timesteps.tolist() == ddim.timesteps.tolist()
            model = lambda x, t: torch.tanh(1.3 * x) + 0.1 * torch.sin(x * (1 + t / 500.0))
            ts = ddim.timesteps.tolist()
            x0 = torch.randn((301,), generator=torch.Generator().manual_seed(n), dtype=torch.float64)
            mine = _run_rows(sch, pred, x0, lambda x, k: model(x, ts[k]))
            x = x0
            for k, t in enumerate(ts):
                a, a_prev = float(ddim.alphas_cumprod[t]), float(ddim._prev_alpha_cumprod(t))
                m = model(x, t)
                if pred == "epsilon":
                    p0, e = (x - (1 - a) ** 0.5 * m) / a ** 0.5, m
                elif pred == "sample":
                    p0, e = m, (x - a ** 0.5 * m) / (1 - a) ** 0.5
                else:
                    p0, e = a ** 0.5 * x - (1 - a) ** 0.5 * m, a ** 0.5 * m + (1 - a) ** 0.5 * x
                x = a_prev ** 0.5 * p0 + (1 - a_prev) ** 0.5 * e
                worst = max(worst, rel(mine[k], x))
    print(f"dpm order 1 vs DDIM: worst rel-L2 {worst:.3e}")
    assert worst <= 1e-12


def _exact_model(ref, pred, x0s):
    """m of a model that knows the data point x0*: the prediction consistent with the x it is shown at call k."""
    def model(x, k):
        alpha, sigma = ref.alpha_sigma(k)
        eps = (x - alpha * x0s) / sigma
        return {"epsilon": eps, "sample": x0s, "v_prediction": alpha * eps - sigma * x0s}[pred]
    return model


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("order", [1, 2])
def test_exact_model_stays_on_the_trajectory_and_ends_at_x0(order, spacing):
    """x0*, eps* fixed: an exact model keeps every ODE iterate on alpha_t x0* + sigma_t eps* and the chain ends at x0*, for every N,
    order, spacing and prediction type; the SDE form leaves the trajectory (fresh noise) and still ends at x0*.  With the model's v fed to
    an epsilon scheduler the same check fails."""
    g = torch.Generator().manual_seed(3)
    x0s, epss = torch.randn((129,), generator=g, dtype=torch.float64), torch.randn((129,), generator=g, dtype=torch.float64)
    worst = 0.0
    for n in (1, 2, 3, 10, 50):
        for pred in PREDS:
            for algo in ALGOS:
                sch, ref = _pair(n, solver_order=order, algorithm_type=algo, timestep_spacing=spacing, prediction_type=pred)
                a0, s0 = ref.alpha_sigma(0)
                zs = [torch.randn((129,), generator=g, dtype=torch.float64) for _ in range(n)]
                xs = _run_rows(sch, pred, a0 * x0s + s0 * epss, _exact_model(ref, pred, x0s), zs)
                if algo == ALGOS[0]:
                    for k, x in enumerate(xs):
                        a, s = ref.alpha_sigma(k + 1)
                        worst = max(worst, rel(x, a * x0s + s * epss))
                elif n > 1:
                    a, s = ref.alpha_sigma(1)
                    assert rel(xs[0], a * x0s + s * epss) > 1e-3      # the SDE form really draws
                worst = max(worst, rel(xs[-1], x0s))
    print(f"dpm exact model order {order} {spacing}: worst rel-L2 {worst:.3e}")
    assert worst <= 1e-12
    sch, ref = _pair(10, solver_order=order, timestep_spacing=spacing, prediction_type="epsilon")
    a0, s0 = ref.alpha_sigma(0)
    wrong = _run_rows(sch, "epsilon", a0 * x0s + s0 * epss, _exact_model(ref, "v_prediction", x0s))
    off = [rel(x, ref.alpha_sigma(k + 1)[0] * x0s + ref.alpha_sigma(k + 1)[1] * epss) for k, x in enumerate(wrong)]
    assert max(off) > 1e-2 and off[-1] > 1e-6              # the same check (every iterate and the end <= 1e-12) fails by far


def test_the_second_order_is_really_used():
    """x0_hat = alpha s^2 / (alpha^2 s^2 + sigma^2) x (the posterior mean under data N(0, s^2), s = 0.5): the probability-flow ODE ends at
    x_T sqrt(s^2 / (alpha_T^2 s^2 + sigma_T^2)).  Order 2's end error is strictly below order 1's at N = 20, 40, 80, and both fall with
    N.  No factor of 4 per doubling is asserted: the first-order last step to sigma = 0 dominates."""
    s2 = 0.25
    for spacing in ("linspace", "trailing"):
        errs = {}
        for order in (1, 2):
            for n in (20, 40, 80):
                sch, ref = _pair(n, solver_order=order, timestep_spacing=spacing, prediction_type="sample")

                def model(x, k):
                    a, s = ref.alpha_sigma(k)
                    return a * s2 / (a * a * s2 + s * s) * x
                xT = torch.ones((1,), dtype=torch.float64)
                end = _run_rows(sch, "sample", xT, model)[-1]
                aT, sT = ref.alpha_sigma(0)
                want = xT * (s2 / (aT * aT * s2 + sT * sT)) ** 0.5
                errs[order, n] = rel(end, want)
        print(f"dpm linear ODE {spacing}: order 1 {[f'{errs[1, n]:.3f}' for n in (20, 40, 80)]}, "
              f"order 2 {[f'{errs[2, n]:.3f}' for n in (20, 40, 80)]}")
        for n in (20, 40, 80):
            assert errs[2, n] < errs[1, n], (spacing, n, errs)
        for order in (1, 2):
            assert errs[order, 20] > errs[order, 40] > errs[order, 80], (spacing, order, errs)


def test_timestep_grids():
    from ldm3d.schedulers import DPMSolverMultistepScheduler
    want = {"linspace": [999, 899, 799, 699, 599, 500, 400, 300, 200, 100],
            "trailing": [999, 899, 799, 699, 599, 499, 399, 299, 199, 99],
            "leading": [900, 800, 700, 600, 500, 400, 300, 200, 100, 0]}
    for spacing, ts in want.items():
        s = DPMSolverMultistepScheduler(num_train_timesteps=1000, timestep_spacing=spacing)
        s.set_timesteps(10)
        assert s.timesteps.tolist() == ts and timesteps(spacing, 1000, 10) == ts, spacing
        assert s.num_inference_steps == 10 and s.counter == 0 and s.prev_x0 is None
    s = DPMSolverMultistepScheduler(num_train_timesteps=1000, timestep_spacing="leading", steps_offset=1)
    s.set_timesteps(10)
    assert s.timesteps.tolist() == [901, 801, 701, 601, 501, 401, 301, 201, 101, 1]
    s = DPMSolverMultistepScheduler(num_train_timesteps=1000)
    assert s.timestep_spacing == "linspace" and s.solver_order == 2 and s.algorithm_type == "dpmsolver++" and s.clip_sample is False
    s.set_timesteps(1)
    assert s.timesteps.tolist() == [999]
    with pytest.raises(ValueError):
        s.set_timesteps(1001)
    with pytest.raises(ValueError):
        s.set_timesteps(0)
    with pytest.raises(ValueError, match="strictly falling"):
        s.set_timesteps(1000)                                # the rounded linspace grid repeats a timestep


def test_argument_checks_and_refused_options():
    from ldm3d.schedulers import DPMSolverMultistepScheduler as S
    for kw, word in ((dict(solver_order=3), "solver_order=3"), (dict(algorithm_type="dpmsolver"), "dpmsolver"),
                     (dict(algorithm_type="sde-dpmsolver"), "sde-dpmsolver"), (dict(solver_type="heun"), "heun"),
                     (dict(use_karras_sigmas=True), "use_karras_sigmas"), (dict(use_exponential_sigmas=True), "use_exponential_sigmas"),
                     (dict(thresholding=True), "thresholding"), (dict(final_sigmas_type="sigma_min"), "sigma_min")):
        with pytest.raises(NotImplementedError, match=word):
            S(**kw)
    for kw in (dict(solver_order=0), dict(solver_order=4), dict(algorithm_type="euler"), dict(timestep_spacing="karras"),
               dict(prediction_type="flow"), dict(solver_type="bh2"), dict(final_sigmas_type="one"),
               dict(clip_sample=True, clip_sample_min=1.0, clip_sample_max=-1.0)):
        with pytest.raises(ValueError):
            S(**kw)
    with pytest.raises(NotImplementedError):
        S(schedule="cosine")
    for pred in PREDS:
        assert S(prediction_type=pred, solver_order=1, algorithm_type="sde-dpmsolver++", timestep_spacing="trailing").kind == 4


def test_exported_next_to_the_others():
    import ldm3d.schedulers as a
    from ldm3d.config import TARGET_ALIASES
    assert issubclass(a.DPMSolverMultistepScheduler, a._Scheduler)
    assert TARGET_ALIASES["diffusers.DPMSolverMultistepScheduler"] == "ldm3d.schedulers.DPMSolverMultistepScheduler"
    for name in ("add_noise", "get_velocity", "add_noise_and_target"):           # the noising methods are inherited
        assert getattr(a.DPMSolverMultistepScheduler, name) is getattr(a._Scheduler, name)


def test_stateful_step_misuse_and_chain_independence():
    """The order checks come before any device work, so they are visible without a GPU."""
    from ldm3d.schedulers import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(**cfgs.SCHED)
    s.set_timesteps(4)
    x = torch.zeros((4,))
    with pytest.raises(ValueError, match="call 0 of the chain is at timestep 999"):
        s.step(x, 749, x)                                    # the second timestep first
    s.counter = 4
    with pytest.raises(ValueError, match="calls are made"):
        s.step(x, 250, x)
    s.reset_state()
    assert s.counter == 0 and s.prev_x0 is None
    with pytest.raises(Exception, match="CUDA tensors only"):
        s.step(x, 999, x)                                    # in order, but not on the device: no CPU fallback
    assert s.counter == 0
    with pytest.raises(ValueError):
        s._row(4)
    s.counter, s.prev_x0 = 2, x
    c = s.chain_scheduler()
    assert c is not s and c.counter == 0 and c.prev_x0 is None and s.counter == 2 and s.prev_x0 is x
    assert c.timesteps.tolist() == s.timesteps.tolist() and c._dpm_rows() == s._dpm_rows()
    c.counter = 3
    assert s.counter == 2
    s.set_timesteps(5)                                       # a new grid rewinds the state
    assert s.counter == 0 and s.prev_x0 is None and len(c.timesteps) == 4


def test_refused_entries_name_the_scheduler():
    from ldm3d.inferer import _check_inpaint, _check_warm_start
    from ldm3d.schedulers import DPMSolverMultistepScheduler, repaint_rows
    s = DPMSolverMultistepScheduler(**cfgs.SCHED)
    s.set_timesteps(4)
    z = torch.zeros((1, 4, 2, 2, 2))
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        _check_warm_start(s, 4, z, 1)
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        _check_inpaint(s, z, torch.ones((2, 2, 2)), None, 0, z.shape)
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        repaint_rows(s)
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        s.repaint_sampler(z, torch.ones((2, 2, 2)))


def test_rows_survive_the_rounding_to_fp32():
    """What ldm_sampler_create_dpm asks of the table, checked on the fp32 rows the device would be given: finite, cz >= 0, DRAWS exactly
    where cz != 0, row 0 without HAS_PREV."""
    for algo in ALGOS:
        for spacing in SPACINGS:
            for n in (1, 2, 10, 50, 500):
                sch, _ = _pair(n, algorithm_type=algo, timestep_spacing=spacing)
                rows = np.asarray(sch._dpm_rows(), dtype=np.float32)
                assert rows.shape == (n, 16) and np.isfinite(rows).all()
                flags = rows[:, 4].astype(np.int64)
                assert not flags[0] & HAS_PREV and (rows[:, 7] >= 0).all()
                assert ((flags & DRAWS) != 0).tolist() == (rows[:, 7] != 0).tolist()
                assert (rows[(flags & HAS_PREV) == 0, 6] == 0).all()
