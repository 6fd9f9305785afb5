"""Known answers of the likelihood reference (tests/likelihood_ref.py: MONAI's get_likelihood restated), the likelihood row table, the
nearest-resize index rule and the refusals of ``inference.py --likelihood``.  No GPU."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import cfgs
import likelihood_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = 1.0 / 255.0


def _draw(n=4096, seed=0):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.clamp(0.6 * torch.randn((n,), generator=g, dtype=torch.float64), -0.99, 0.99)
    return x0, torch.randn((n,), generator=g, dtype=torch.float64), torch.randn((n,), generator=g, dtype=torch.float64)


@pytest.mark.parametrize("variance_type", ["fixed_small", "fixed_large"])
def test_perfect_epsilon_model_scores_zero_above_t0(variance_type):
    tab = lr.Tables(**cfgs.SCHED, variance_type=variance_type)
    x0, z, _ = _draw()
    for t in (999, 500, 37, 1):
        kl = lr.term_map(tab, t, x0, lr.noisy(tab, t, x0, z), z)
        assert float(kl.abs().max()) < 1e-12, (t, float(kl.abs().max()))


def test_perfect_epsilon_model_at_t0():
    x0, z, _ = _draw()
    tab = lr.Tables(**cfgs.SCHED, variance_type="fixed_large")
    kl = lr.term_map(tab, 0, x0, lr.noisy(tab, 0, x0, z), z, BIN)
    u = torch.tensor(BIN / (2.0 * math.sqrt(float(tab.betas[0]))), dtype=torch.float64)
    want = -math.log(2.0 * float(lr.approx_standard_normal_cdf(u)) - 1.0)
    assert torch.allclose(kl, torch.full_like(kl, want), rtol=1e-5, atol=0), (float(kl.min()), float(kl.max()), want)
    tab = lr.Tables(**cfgs.SCHED, variance_type="fixed_small")
    kl = lr.term_map(tab, 0, x0, lr.noisy(tab, 0, x0, z), z, BIN)
    assert float(kl.abs().max()) == 0.0


@pytest.mark.parametrize("pred", ["epsilon", "sample", "v_prediction"])
@pytest.mark.parametrize("variance_type", ["fixed_small", "fixed_large"])
def test_term_above_t0_is_the_scaled_squared_x0_error(variance_type, pred):
    tab = lr.Tables(**cfgs.SCHED, variance_type=variance_type, prediction_type=pred)
    x0, z, m = _draw(seed=1)
    for t in (999, 500, 37, 1):
        kl, p = lr.term_map(tab, t, x0, lr.noisy(tab, t, x0, z), m, parts=True)
        want = p["c0"] ** 2 * (x0 - p["x0_hat"]) ** 2 / (2.0 * p["var"])
        # MONAI's order subtracts two O(1) means whose difference is O(c0): in fp64 that costs about 1e-16 / c0 ~ 1e-12 of the map's
        # norm at t = 999 (single elements with x0_hat ~ x0 lose more, so the map is compared as a whole)
        err = float((kl - want).norm() / want.norm())
        assert err <= 1e-9, (t, err)


def test_fixed_small_t0_is_a_step_function():
    tab = lr.Tables(**cfgs.SCHED, variance_type="fixed_small")
    x0, z, m = _draw(seed=2)
    kl = lr.term_map(tab, 0, x0, lr.noisy(tab, 0, x0, z), z + 0.05 * m, BIN)
    hi = -math.log(1e-12)
    assert bool(((kl == 0) | ((kl - hi).abs() < 1e-9)).all()) and 0 < int((kl > 1).sum()) < kl.numel()


def test_likelihood_rows_carry_the_scheduler_tables():
    from ldm3d.schedulers import LIK_ROW, DDPMScheduler
    for vt in ("fixed_small", "fixed_large"):
        sch, tab = DDPMScheduler(**cfgs.SCHED, variance_type=vt), lr.Tables(**cfgs.SCHED, variance_type=vt)
        sch.set_timesteps(5)
        rows = sch.likelihood_rows()
        assert [int(r[5]) for r in rows] == sch.timesteps.tolist() == [800, 600, 400, 200, 0] and all(len(r) == LIK_ROW for r in rows)
        for r in rows:
            a, _, c0, c1, var = (float(v) for v in tab.coefs(int(r[5]), torch.float64))
            want = [a ** 0.5, (1 - a) ** 0.5, a ** -0.5, c0, 1.0 / var, r[5], var ** -0.5, c1]
            assert all(abs(g - w) <= 3e-7 * abs(w) for g, w in zip(r[:8], want)), (r, want)
            assert r[8:] == [0.0] * (LIK_ROW - 8)
        assert rows[-1][7] == 0.0                                  # t = 0: abar_prev = 1, no weight on x_t


@pytest.mark.parametrize("src,dst", [((2, 3, 5), (8, 12, 20)), ((3, 4, 5), (7, 9, 11))])
def test_nearest_index_rule_is_torchs(src, dst):
    x = torch.arange(2 * 3 * src[0] * src[1] * src[2], dtype=torch.float32).reshape((2, 3) + src)
    assert torch.equal(lr.resize_nearest(x, dst), F.interpolate(x, size=dst, mode="nearest"))


def _parse(monkeypatch, *extra):
    import inference
    monkeypatch.setattr(sys, "argv", ["inference.py", "-e", os.path.join(ROOT, "config", "environment_synthetic.json"),
                                      "-c", os.path.join(ROOT, "config", "config_synthetic_24.json"), *extra])
    return inference.parse_cli()


def test_inference_cli_likelihood_refusals(monkeypatch, capsys):
    ok = ("--likelihood", "--condition", "pair.npz")
    for extra, word in ((("--likelihood",), "--condition"),
                        (ok + ("--sampler", "ddim", "--steps", "4"), "--sampler"),
                        (ok + ("--sampler", "pndm", "--steps", "4"), "--sampler"),
                        (ok + ("--sampler", "rflow", "--steps", "4"), "--sampler"),
                        (ok + ("--cfg", "2"), "--cfg"),
                        (ok + ("--sliding-window",), "--sliding-window"),
                        (ok + ("--chains", "2"), "--chains"),
                        (("--likelihood-map", "--condition", "pair.npz"), "--likelihood")):
        with pytest.raises(SystemExit) as e:
            _parse(monkeypatch, *extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, extra
    ns = _parse(monkeypatch, *ok, "--steps", "4", "--likelihood-map", "-n", "2")
    assert ns.likelihood and ns.likelihood_map and ns.steps == 4 and ns.num == 2
    assert not _parse(monkeypatch, "--steps", "4").likelihood


def test_get_likelihood_refuses_other_schedulers_and_modes():
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler, PNDMScheduler, RFlowScheduler
    z = torch.zeros((1, 4, 2, 2, 2))
    for sch in (DDIMScheduler(**cfgs.SCHED), PNDMScheduler(**cfgs.SCHED), RFlowScheduler()):
        with pytest.raises(NotImplementedError, match="DDPMScheduler"):
            LatentDiffusionInferer(sch).get_likelihood(z, None, None)
    inf = LatentDiffusionInferer(DDPMScheduler(**cfgs.SCHED))
    with pytest.raises(ValueError, match="nearest, bilinear, or trilinear"):
        inf.get_likelihood(z, None, None, resample_latent_likelihoods=True, resample_interpolation_mode="cubic")
    for mode in ("bilinear", "trilinear"):
        with pytest.raises(NotImplementedError, match=mode):
            inf.get_likelihood(z, None, None, resample_latent_likelihoods=True, resample_interpolation_mode=mode)
    with pytest.raises(ValueError, match="one of them"):
        inf.get_likelihood(z, None, None, noise=z, fused_seed=1)
