"""Warm-start sampling on the host (no GPU): the strength -> start step map, the DDIM inversion rows, the invert-then-sample identity
on an exact point-mass model in float64, and the argument errors of the Python layer and the command line that need no device."""
import os
import sys

import pytest
import torch

import cfgs
import warm_start_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_known_answers_of_the_strength_map():
    from ldm3d.schedulers import start_step_for_strength
    assert start_step_for_strength(10, 1.0) == 0
    assert start_step_for_strength(10, 0.5) == 5
    assert start_step_for_strength(7, 0.3) == 5
    with pytest.raises(ValueError):
        start_step_for_strength(10, 0.05)                    # int(0.5) = 0 steps: nothing to denoise
    for n, s in ((10, 1.0), (10, 0.5), (7, 0.3), (1000, 0.25), (50, 0.999), (3, 0.34)):
        assert start_step_for_strength(n, s) == ref.start_step(n, s), (n, s)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            start_step_for_strength(10, bad)
    with pytest.raises(ValueError):
        start_step_for_strength(0, 0.5)


@pytest.mark.parametrize("pred", ["epsilon", "sample", "v_prediction"])
def test_inversion_rows_are_ddim_rows_with_abar_next(pred):
    """``_inversion_row(t)`` field by field against a row built by hand from the scheduler's fp32 table, against the forward DDIM row
    (the slots that do not depend on the neighbouring timestep are the same numbers) and against the float64 table."""
    from ldm3d.schedulers import DDIMScheduler
    sch = DDIMScheduler(**cfgs.SCHED, prediction_type=pred)
    sch.set_timesteps(10)
    ac, ac64 = sch.alphas_cumprod, ref.alphas_cumprod(**cfgs.SCHED)
    for t in [int(t) for t in sch.timesteps.tolist()]:
        nxt = t + 100
        a_t = ac[t]
        a_next = ac[nxt] if nxt < 1000 else torch.tensor(0.0)
        hand = [float(1.0 / a_t ** 0.5), float((1 - a_t) ** 0.5), float(a_next ** 0.5), float((1 - a_next) ** 0.5), 0.0, float(t),
                float(a_t ** 0.5), float(1.0 / (1 - a_t) ** 0.5)]
        row, fwd = sch._inversion_row(t), sch._row(t, 0.0)
        assert len(row) == 8
        for j in range(8):
            assert row[j] == hand[j], (t, j, row[j], hand[j])
        for j in (0, 1, 5, 6, 7):
            assert row[j] == fwd[j], (t, j)
        assert row[4] == 0.0                                 # no noise: the deterministic sampler
        a64, n64 = float(ac64[t]), float(ac64[nxt]) if nxt < 1000 else 0.0
        want = [a64 ** -0.5, (1 - a64) ** 0.5, n64 ** 0.5, (1 - n64) ** 0.5]
        for j in range(4):                                   # fp32 table and a few fp32 operations: a handful of ulps
            assert abs(row[j] - want[j]) <= 1e-5 * max(abs(want[j]), 1e-3), (t, j, row[j], want[j])
    last = sch._inversion_row(900)                           # beyond the table: first_alpha_cumprod = 0, pure noise
    assert last[2] == 0.0 and last[3] == 1.0
    # the forward row of the next timestep walks back over the same pair of alphas: its c0 is this row's sqrt(abar_t)
    assert sch._row(500, 0.0)[2] == sch._inversion_row(400)[6]
    assert sch.inversion_timesteps() == list(range(0, 1000, 100)) and sch.inversion_timesteps(3) == [0, 100, 200]
    for bad in (0, 11):
        with pytest.raises(ValueError):
            sch.inversion_timesteps(bad)


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("pred", ["epsilon", "sample", "v_prediction"])
def test_point_mass_inversion_then_sampling_returns_the_start(pred, clip):
    """The exact model of a point mass at x*, eps*(x, t) = (x - sqrt(abar_t) x*) / sqrt(1 - abar_t), |x*| <= 1: every reversed and every
    forward DDIM step predicts x0_hat = x* and keeps eps_hat constant, so inverting j steps from z and sampling j steps returns z, and
    n - 1 - k0 reversed steps land on timesteps[k0].  Float64 throughout: the gate is round-off."""
    from ldm3d.schedulers import DDIMScheduler
    sch = DDIMScheduler(**cfgs.SCHED)
    n = 10
    sch.set_timesteps(n)
    ts = [int(t) for t in sch.timesteps.tolist()]
    ac = ref.alphas_cumprod(**cfgs.SCHED)
    g = torch.Generator().manual_seed(3)
    xs = torch.rand((64,), generator=g, dtype=torch.float64) * 1.8 - 0.9
    z = torch.randn((64,), generator=g, dtype=torch.float64)

    def model(x, t):
        a = float(ac[t])
        eps = (x - a ** 0.5 * xs) / (1 - a) ** 0.5
        if pred == "epsilon":
            return eps
        return xs if pred == "sample" else a ** 0.5 * eps - (1 - a) ** 0.5 * xs

    ratio = 1000 // n
    for k0 in (0, 4, n - 2):
        j = n - 1 - k0
        x = z.clone()
        eps0 = (z - float(ac[0]) ** 0.5 * xs) / (1 - float(ac[0])) ** 0.5
        for t in sch.inversion_timesteps(j):
            nxt = t + ratio
            x, x0 = ref.reversed_step(pred, ref.coefs(ac[t], ac[nxt] if nxt < 1000 else 0.0), model(x, t), x, clip)
            assert float((x0 - xs).abs().max()) <= 1e-12
            landed = nxt
        assert landed == ts[k0]                              # the identity invert's docstring states
        assert float((x - (float(ac[landed]) ** 0.5 * xs + (1 - float(ac[landed])) ** 0.5 * eps0)).abs().max()) <= 1e-12 * float(x.abs().max())
        for t in ts[k0:-1]:                                  # j forward steps: back to timesteps[-1], where z lives
            x, _ = ref.ddim_step(pred, ref.coefs(ac[t], ac[t - ratio]), model(x, t), x, clip)
        assert float((x - z).abs().max()) <= 1e-12 * float(z.abs().max()), (k0, float((x - z).abs().max()))


def test_python_layer_refuses_without_touching_a_device():
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler, PNDMScheduler
    ddim = DDIMScheduler(**cfgs.SCHED)
    ddim.set_timesteps(10)
    inf = LatentDiffusionInferer(ddim)
    noise, z0 = torch.zeros((1, 4, 2, 2, 2)), torch.zeros((1, 4, 2, 2, 2))
    with pytest.raises(ValueError):
        inf.sample(noise, None, None, start_step=3)                                     # no latent to start from
    for k0 in (-1, 10):
        with pytest.raises(ValueError):
            inf.sample(noise, None, None, init_latent=z0, start_step=k0)
    with pytest.raises(ValueError):
        inf.sample(noise, None, None, init_latent=torch.zeros((3, 4, 2, 2, 2)), start_step=2)     # neither 1 nor B latents
    with pytest.raises(ValueError):
        inf.sample_sliding_window(noise, None, None, (2, 2, 2), start_step=1)
    pndm = PNDMScheduler(skip_prk_steps=True, **cfgs.SCHED)
    pndm.set_timesteps(10)
    with pytest.raises(NotImplementedError):
        inf.sample(noise, None, None, scheduler=pndm, init_latent=z0, start_step=2)
    with pytest.raises(ValueError):
        ddim.inversion_sampler(eta=0.5)
    with pytest.raises(ValueError):
        inf.invert(z0, None, eta=0.5)
    with pytest.raises(NotImplementedError):
        inf.invert(z0, None, scheduler=DDPMScheduler(**cfgs.SCHED))
    with pytest.raises(NotImplementedError):
        inf.invert(z0, None, scheduler=pndm)
    with pytest.raises(ValueError):
        inf.sample_ensemble(4, (4, 2, 2, 2), None, torch.nn.Linear(1, 1), start_step=2)            # ... the ensemble too


REFUSED = [
    ["--strength", "0.5"],                                                               # without --init-from-condition
    ["--init-invert"],
    ["--init-from-condition"],                                                           # without --condition
    ["--condition", "x.npz", "--init-from-condition", "--sampler", "pndm", "--steps", "10"],
    ["--condition", "x.npz", "--init-from-condition", "--likelihood"],
    ["--condition", "x.npz", "--init-from-condition", "--chains", "2"],
    ["--condition", "x.npz", "--init-from-condition", "--init-invert"],                  # the full DDPM chain does not invert
    ["--condition", "x.npz", "--init-from-condition", "--init-invert", "--steps", "10", "--ensemble", "2"],
    ["--condition", "x.npz", "--init-from-condition", "--steps", "10", "--strength", "0.05"],
    ["--condition", "x.npz", "--init-from-condition", "--steps", "10", "--strength", "1.5"],
]


def parse(argv, tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import inference
    env = tmp_path / "environment.json"
    env.write_text("{}")
    monkeypatch.setattr(sys, "argv", ["inference.py", "-e", str(env), "-c", os.path.join(ROOT, "config", "config_synthetic_train.json")] + argv)
    monkeypatch.delenv("LDM_PRECISION", raising=False)
    return inference.parse_cli()


@pytest.mark.parametrize("argv", REFUSED, ids=[" ".join(a[-3:]) for a in REFUSED])
def test_command_line_refuses(argv, tmp_path, monkeypatch, capsys):
    with pytest.raises(SystemExit) as e:
        parse(argv, tmp_path, monkeypatch)
    assert e.value.code != 0
    assert "error" in capsys.readouterr().err


def test_command_line_resolves_the_start_step(tmp_path, monkeypatch):
    ns = parse(["--condition", "x.npz", "--init-from-condition", "--strength", "0.4", "--steps", "10"], tmp_path, monkeypatch)
    assert ns.start_step == 6 and not ns.init_invert
    ns = parse(["--condition", "x.npz", "--init-from-condition", "--init-invert", "--strength", "0.4", "--steps", "10", "--sliding-window",
                "--cfg", "2.0", "--metrics"], tmp_path, monkeypatch)
    assert ns.start_step == 6 and ns.init_invert
    ns = parse(["--condition", "x.npz", "--init-from-condition", "--strength", "0.25", "--sampler", "ddpm", "--ensemble", "3"], tmp_path, monkeypatch)
    assert ns.start_step == 750                              # the full DDPM chain of the config's 1000 timesteps
    assert parse(["--steps", "10"], tmp_path, monkeypatch).start_step == 0
