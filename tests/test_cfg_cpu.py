"""Classifier-free guidance without a GPU: known answers of the fp64 restatement (tests/cfg_ref.py), the condition-dropout decision's
statistics and key, and the argument checks of the sampler and of the two command lines."""
import os
import sys

import pytest
import torch

import cfg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_combine_known_answers():
    g = torch.Generator().manual_seed(0)
    u, c = torch.randn((257,), generator=g), torch.randn((257,), generator=g)
    assert torch.equal(cfg_ref.combine(u, c, 0.0), u.double())
    assert torch.allclose(cfg_ref.combine(u, c, 1.0), c.double(), rtol=0, atol=1e-15)
    # affine in w: the value at 3.5 lies on the line through the values at 0 and 1, and second differences vanish
    a0, a1, a35, a7 = (cfg_ref.combine(u, c, w) for w in (0.0, 1.0, 3.5, 7.0))
    assert torch.allclose(a35, a0 + 3.5 * (a1 - a0), rtol=0, atol=1e-14)
    assert torch.allclose(a0 - 2.0 * a35 + a7, torch.zeros_like(a0), rtol=0, atol=1e-14)
    assert torch.equal(cfg_ref.combine(u, u, 3.5), u.double())     # c = u: guidance has nothing to act on


def test_doubled_batch_order_is_unconditional_first():
    x, t = torch.arange(2 * 3, dtype=torch.float32).reshape(2, 3), torch.tensor([5.0, 9.0])
    cond = torch.ones((2, 3))
    xx, tt, cc = cfg_ref.doubled_inputs(x, t, cond, -1.0)
    assert torch.equal(xx[:2], x) and torch.equal(xx[2:], x) and tt.tolist() == [5.0, 9.0, 5.0, 9.0]
    assert bool((cc[:2] == -1.0).all()) and torch.equal(cc[2:], cond)
    # a model that returns its condition: u = fill, c = cond, so the guided output is fill + w (cond - fill)
    out = cfg_ref.guided_output(lambda a, b, c: c, x, t, cond, 2.0, -1.0)
    assert torch.equal(out, torch.full((2, 3), 3.0, dtype=torch.float64))


@pytest.mark.parametrize("seed,step,count", [(7, 0, 396), (7, 1, 428), (0, 0, 382)])
def test_drop_mask_statistics(seed, step, count):
    """p = 0.1 over the dataset indices 0 .. 4095: the drop count lies in [294, 525] = 409.6 +- 6 sigma, sigma = sqrt(4096 * 0.1 * 0.9) =
    19.2; the three counts are the values this generator gives and pin the key layout."""
    m = cfg_ref.drop_mask(seed, step, range(4096), 0.1)
    assert 294 <= sum(m) <= 525
    assert sum(m) == count


def test_drop_mask_key():
    a, b = cfg_ref.drop_mask(7, 0, range(4096), 0.1), cfg_ref.drop_mask(7, 1, range(4096), 0.1)
    assert a != b                                                  # the step is part of the key
    assert cfg_ref.drop_mask(8, 0, range(4096), 0.1) != a          # and the seed
    idx = [5, 900, 17, 5]
    assert cfg_ref.drop_mask(7, 0, idx, 0.1) == [a[i] for i in idx]   # a decision belongs to the dataset index, not to the slot
    assert not any(cfg_ref.drop_mask(7, 0, range(4096), 0.0)) and all(cfg_ref.drop_mask(7, 0, range(4096), 1.0))
    # a stream of its own: not the rectified-flow timestep draw's uniforms (stream 3)
    from rflow_ref import timestep_uniform
    assert [cfg_ref.drop_uniform(7, 0, i) for i in range(8)] != [timestep_uniform(7, 0, i) for i in range(8)]


def _parse(monkeypatch, *extra):
    import inference
    monkeypatch.setattr(sys, "argv", ["inference.py", "-e", os.path.join(ROOT, "config", "environment_synthetic.json"),
                                      "-c", os.path.join(ROOT, "config", "config_synthetic_24.json"), *extra])
    return inference.parse_cli()


def test_inference_cli_cfg_needs_a_condition(monkeypatch, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(monkeypatch, "--cfg", "2")
    assert e.value.code == 2 and "--condition" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--cfg", "2", "--condition", "pair.npz", "--chains", "2")
    assert "--chains" in capsys.readouterr().err
    ns = _parse(monkeypatch, "--cfg", "2", "--condition", "pair.npz", "--steps", "4")
    assert ns.cfg == 2.0 and ns.cfg_fill_value == -1.0
    ns = _parse(monkeypatch, "--cfg", "1.5", "--cfg-fill-value", "0", "--condition", "pair.npz", "--sliding-window", "--steps", "4")
    assert ns.cfg == 1.5 and ns.cfg_fill_value == 0.0 and ns.sliding_window
    assert _parse(monkeypatch, "--steps", "4").cfg is None


def test_sample_refuses_cfg_without_concat_conditioning():
    from ldm3d.inferer import LatentDiffusionInferer
    inf = LatentDiffusionInferer(scheduler=None)
    z = torch.zeros((1, 4, 2, 2, 2))
    with pytest.raises(ValueError, match="conditioning"):
        inf.sample(z, None, None, cfg=2.0)
    with pytest.raises(ValueError, match="concat"):
        inf.sample(z, None, None, conditioning=z, cfg=2.0)         # mode defaults to "crossattn"
    with pytest.raises(ValueError, match="conditioning"):
        inf.sample_sliding_window(z, None, None, (2, 2, 2), cfg=2.0)


def test_trainer_refuses_a_bad_drop_probability():
    from ldm3d.trainer import DiffusionTrainer
    for p in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="cond_drop_prob"):
            DiffusionTrainer(None, None, None, lr=1e-4, cond_drop_prob=p)


def test_new_entries_are_declared_and_exported():
    from ldm3d import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "ldm3d.h")).read()
    for name in ("ldm_guidance_combine", "ldm_unet_guided_workspace_bytes", "ldm_unet_denoise_step_guided",
                 "ldm_unet_denoise_step_windows_guided", "ldm_cond_dropout"):
        assert name + "(" in hdr and hasattr(L, name) and getattr(L, name).argtypes is not None, name
