"""Ensemble statistics without a GPU: the recurrence the kernels implement against a two-pass computation, the bias / variance
decomposition the command line reports, proof that the GPU tests' gates reject a sum-of-squares kernel, the chunk planner, and the
refusals of `inference.py --ensemble`."""
import os
import sys

import pytest
import torch

import ensemble_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["unit", "offset"])
@pytest.mark.parametrize("K", [1, 2, 5, 16])
def test_fp64_recurrence_equals_two_pass(name, K):
    x = ref.family(name, K, 4099, 10 + K)
    mean, m2, count = ref.welford(x, torch.float64)
    mean2, m22 = ref.two_pass(x)
    assert count == K
    assert float((mean - mean2).abs().max()) <= 1e-12 and float((m2 - m22).abs().max()) <= 1e-12


def test_recurrence_continues_from_a_state():
    x = ref.family("unit", 5, 257, 3)
    whole = ref.welford(x, torch.float32)
    mean, m2, c = ref.welford(x[:2], torch.float32)
    part = ref.welford(x[2:], torch.float32, mean, m2, c)
    assert torch.equal(whole[0], part[0]) and torch.equal(whole[1], part[1]) and part[2] == 5


@pytest.mark.parametrize("K", [2, 5, 16])
def test_decomposition_identity_fp64(K):
    """mean_k MSE(x_k, y) == bias_sq + mean_var(ddof=0)"""
    x = ref.family("unit", K, 4099, 20 + K).double()
    y = ref.family("unit", 1, 4099, 99)[0].double()
    mean, m2, _ = ref.welford(x, torch.float64)
    s = ref.stats(mean, m2, K, ddof=0, target=y)
    mse = float(((x - y) ** 2).mean(dim=1).mean())
    assert abs(mse - (s["bias_sq"] + s["mean_var"])) <= 1e-12


@pytest.mark.parametrize("K", [2, 5, 16])
def test_the_gate_bites_a_sum_of_squares_kernel(K):
    """On the "offset" inputs (100 + 0.01 randn) the naive fp32 sum / sum-of-squares m2 misses the GPU tests' m2 gate by orders of
    magnitude: a kernel of that kind cannot pass them."""
    x = ref.family("offset", K, 4099, 30 + K)
    _, gate_m2, _, ys, _, s64 = ref.gates(x)
    _, naive = ref.naive_fp32(x)
    err = float((naive.double() - s64).abs().max())
    print(f"K={K}: naive m2 error {err:.3e}, fp32 recurrence error {ys:.3e}, gate {gate_m2:.3e}")
    assert err > gate_m2, (err, gate_m2)


def test_plan_chunks_covers_every_member_once_in_order(built_lib):
    from ldm3d.ensemble import plan_chunks
    for K in (2, 3, 5, 8, 17):
        for mb in range(1, K + 2):
            chunks = plan_chunks(K, mb)
            flat = [first + j for first, size in chunks for j in range(size)]
            assert flat == list(range(K)), (K, mb, chunks)
            assert all(1 <= size <= mb for _, size in chunks)
            assert all(size == mb for _, size in chunks[:-1])
    assert plan_chunks(5, 2) == [(0, 2), (2, 2), (4, 1)]
    for bad in ((0, 1), (3, 0), (-1, 2)):
        with pytest.raises(ValueError):
            plan_chunks(*bad)


def _parse(monkeypatch, *extra):
    import inference
    monkeypatch.setattr(sys, "argv", ["inference.py", "-e", os.path.join(ROOT, "config", "environment_synthetic.json"),
                                      "-c", os.path.join(ROOT, "config", "config_synthetic_train.json"), *extra])
    return inference.parse_cli()


def test_inference_cli_ensemble_flags_parse(built_lib, monkeypatch):
    monkeypatch.setenv("LDM_PRECISION", "bf16")                          # --precision writes the variable: restored when the test ends
    ns = _parse(monkeypatch, "--condition", "pair.npz", "--steps", "4", "--ensemble", "5", "--ensemble-batch", "2", "--ensemble-keep", "1",
                "--metrics", "--cfg", "2.0", "--ema", "--precision", "fp32")
    assert (ns.ensemble, ns.ensemble_batch, ns.ensemble_keep) == (5, 2, 1)
    ns = _parse(monkeypatch, "--condition", "pair.npz", "--steps", "4", "--ensemble", "2", "--sliding-window", "--sw-batch", "3",
                "--sampler", "pndm")
    assert ns.ensemble == 2 and ns.sliding_window and ns.ensemble_batch == 0
    ns = _parse(monkeypatch, "--condition", "pair.npz")
    assert ns.ensemble == 0


@pytest.mark.parametrize("extra,word", [
    (["--ensemble", "3"], "--condition"),                                              # no scan to sample the posterior of
    (["--ensemble", "1", "--condition", "p.npz"], "K >= 2"),
    (["--ensemble", "3", "--condition", "p.npz", "-n", "2"], "-n"),
    (["--ensemble", "3", "--condition", "p.npz", "--chains", "2"], "--chains"),
    (["--ensemble", "3", "--condition", "p.npz", "--batch", "2"], "--batch"),
    (["--ensemble", "3", "--condition", "p.npz", "--likelihood"], "--likelihood"),
    (["--ensemble", "3", "--condition", "p.npz", "--sliding-window", "--ensemble-batch", "2"], "--ensemble-batch"),
    (["--ensemble", "3", "--condition", "p.npz", "--ensemble-batch", "4"], "--ensemble-batch"),
    (["--ensemble", "3", "--condition", "p.npz", "--ensemble-keep", "4"], "--ensemble-keep"),
    (["--condition", "p.npz", "--ensemble-batch", "2"], "--ensemble"),
    (["--condition", "p.npz", "--ensemble-keep", "1"], "--ensemble"),
])
def test_inference_cli_ensemble_refusals(built_lib, monkeypatch, capsys, extra, word):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        _parse(monkeypatch, "--steps", "4", *extra)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_inference_cli_ensemble_refuses_several_ranks(built_lib, monkeypatch, capsys):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        _parse(monkeypatch, "--steps", "4", "--ensemble", "3", "--condition", "p.npz")
    assert e.value.code == 2 and "WORLD_SIZE" in capsys.readouterr().err
