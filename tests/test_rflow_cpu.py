"""RFlowScheduler without a GPU: the inference timesteps' known answers, the device sampler's row table against the fp64 restatement
(tests/rflow_ref.py), the config aliases, and the rflow handling of the two command lines."""
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

from rflow_ref import RFlowRef, ulp32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sch(**kw):
    from ldm3d.schedulers import RFlowScheduler
    return RFlowScheduler(**kw)


def test_set_timesteps_known_answers():
    sch = _sch()
    assert sch.kind == 3 and sch.timesteps.dtype == torch.int64 and sch.timesteps.tolist() == list(range(1000, 0, -1))
    sch.set_timesteps(10)
    assert sch.timesteps.dtype == torch.int64 and sch.timesteps.tolist() == list(range(1000, 0, -100))
    assert sch.num_inference_steps == 10
    cont = _sch(use_discrete_timesteps=False)
    cont.set_timesteps(4)
    assert cont.timesteps.dtype == torch.float32 and cont.timesteps.tolist() == [1000.0, 750.0, 500.0, 250.0]
    tr = _sch(use_discrete_timesteps=False, use_timestep_transform=True)
    tr.set_timesteps(4, input_img_size_numel=8 * 32 ** 3)         # r = 2: t -> 2 t / (1 + t / T)
    assert abs(tr.transform_ratio(8 * 32 ** 3) - 2.0) < 1e-12
    want = np.array([1000.0, 6000.0 / 7.0, 2000.0 / 3.0, 400.0]).astype(np.float32)
    assert tr.timesteps.dtype == torch.float32 and np.array_equal(tr.timesteps.numpy(), want)
    off = _sch(steps_offset=1)
    off.set_timesteps(10)
    assert off.timesteps.tolist() == [t + 1 for t in range(1000, 0, -100)]
    with pytest.raises(ValueError):
        sch.set_timesteps(1001)
    with pytest.raises(ValueError, match="input_img_size_numel"):
        tr.set_timesteps(4)
    odd = _sch(num_train_timesteps=1000)
    odd.set_timesteps(7)                                          # (1 - i / 7) 1000, rounded to the nearest integer
    assert odd.timesteps.tolist() == [1000, 857, 714, 571, 429, 286, 143]


def test_constructor_refuses_what_it_cannot_sample():
    with pytest.raises(ValueError, match="sample_method"):
        _sch(sample_method="cosine")
    with pytest.raises(ValueError, match="scale"):
        _sch(sample_method="logit-normal", scale=0.0)
    with pytest.raises(TypeError):
        _sch(prediction_type="epsilon")                           # no prediction type: the model predicts the velocity
    assert not hasattr(_sch(), "get_velocity")


@pytest.mark.parametrize("n,discrete,transform", list(itertools.product([1, 10, 50], [True, False], [True, False])))
def test_row_table_matches_fp64(n, discrete, transform):
    """dt and tau of every row are the fp64 values rounded once to fp32, the dt sum to t_0 / T within N * 2^-24 (each dt <= 1 carries at
    most half an fp32 ulp), slot 5 is the timestep and the other slots are zero."""
    from ldm3d.schedulers import _sampler_rows
    kw = dict(use_discrete_timesteps=discrete, use_timestep_transform=transform, transform_scale=1.3)
    numel = 24 * 20 * 28
    sch, ref = _sch(**kw), RFlowRef(**kw)
    sch.set_timesteps(n, input_img_size_numel=numel)
    ref.set_timesteps(n, input_img_size_numel=numel)
    assert sch.timesteps.double().tolist() == ref.timesteps.tolist()
    kind, rows = _sampler_rows(sch)
    assert kind == 3 and len(rows) == n
    tab = torch.tensor(rows, dtype=torch.float32)
    assert tab.shape == (n, 8)
    want = ref.rows()
    for k, (dt, tau) in enumerate(want):
        assert float(tab[k, 0]) == float(np.float32(dt)) and float(tab[k, 1]) == float(np.float32(tau)), k
        assert float(tab[k, 5]) == ref.timesteps[k].item()
        assert tab[k, [2, 3, 4, 6, 7]].tolist() == [0.0] * 5
        assert dt > 0.0
    total = float(tab[:, 0].double().sum())
    assert abs(total - ref.timesteps[0].item() / 1000.0) <= n * 2.0 ** -24
    # the row ``step`` passes by value for step k with the inferer's next_timestep is the table's row
    ts = sch.timesteps.tolist()
    for k, t in enumerate(ts):
        assert sch._row(t, ts[k + 1] if k + 1 < n else 0) == rows[k]
    assert sch._row(ts[0], None)[0] == 1.0 / n                    # without next_timestep: dt = 1 / num_inference_steps


def test_reference_helpers():
    assert ulp32(1.0) == 2.0 ** -23 and ulp32(1000.0) == 2.0 ** -14 and ulp32(0.75) == 2.0 ** -24
    ref = RFlowRef(sample_method="logit-normal", loc=0.5, scale=2.0)
    t = ref.sample_timesteps(torch.tensor([0.0, -0.25]))
    assert t.tolist() == [622.0, 500.0]                           # floor(1000 sigmoid(0.5)), floor(1000 sigmoid(0)) = 500


def test_config_aliases_resolve():
    from ldm3d.config import define_instance
    from ldm3d.schedulers import RFlowScheduler
    for target in ("monai.networks.schedulers.RFlowScheduler", "monai.networks.schedulers.rectified_flow.RFlowScheduler"):
        sch = define_instance({"s": {"_target_": target, "num_train_timesteps": 500, "sample_method": "logit-normal"}}, "s")
        assert isinstance(sch, RFlowScheduler) and sch.num_train_timesteps == 500 and sch.sample_method == "logit-normal"


def _flow_config(tmp_path, **section):
    cfg = json.load(open(os.path.join(ROOT, "config", "config_synthetic_24.json")))
    cfg["NoiseScheduler"] = dict(cfg["NoiseScheduler"], scheduler="rflow", **section)
    path = str(tmp_path / "config_rflow.json")
    json.dump(cfg, open(path, "w"))
    return path


def _parse(monkeypatch, config, *extra):
    import inference
    monkeypatch.setattr(sys, "argv", ["inference.py", "-e", os.path.join(ROOT, "config", "environment_synthetic.json"), "-c", config, *extra])
    return inference.parse_cli()


def test_inference_cli_keeps_flow_and_beta_schedules_apart(monkeypatch, capsys, tmp_path):
    import inference
    from ldm3d.schedulers import DDIMScheduler, RFlowScheduler
    flow = _flow_config(tmp_path, use_discrete_timesteps=False)
    beta = os.path.join(ROOT, "config", "config_synthetic_24.json")
    ns = _parse(monkeypatch, flow, "--sampler", "rflow", "--steps", "6")
    sch = inference.make_scheduler(ns)
    assert isinstance(sch, RFlowScheduler) and len(sch.timesteps) == 6 and sch.use_discrete_timesteps is False
    ns = _parse(monkeypatch, flow, "--steps", "8")                 # auto resolves to rflow
    assert ns.sampler == "rflow" and len(inference.make_scheduler(ns).timesteps) == 8
    assert isinstance(inference.make_scheduler(_parse(monkeypatch, beta, "--steps", "5")), DDIMScheduler)
    for config, extra, word in ((flow, ("--sampler", "ddim", "--steps", "6"), "rflow"), (flow, ("--sampler", "ddpm"), "rflow"),
                                (flow, ("--sampler", "pndm", "--steps", "6"), "rflow"), (beta, ("--sampler", "rflow", "--steps", "6"), "rflow"),
                                (flow, (), "--steps"), (flow, ("--sampler", "rflow"), "--steps")):
        with pytest.raises(SystemExit):
            _parse(monkeypatch, config, *extra)
        assert word in capsys.readouterr().err, (config, extra)


def test_train_cli_builds_the_scheduler_the_config_names():
    import train_diffusion
    from ldm3d.schedulers import DDPMScheduler, RFlowScheduler
    ddpm = json.load(open(os.path.join(ROOT, "config", "config_synthetic_train.json")))["NoiseScheduler"]
    sch, kw = train_diffusion.build_noise_scheduler(ddpm)          # no "scheduler" key: the reference's DDPM
    assert isinstance(sch, DDPMScheduler) and kw == train_diffusion.scheduler_args(ddpm)
    assert isinstance(train_diffusion.build_noise_scheduler(dict(ddpm, scheduler="ddpm"))[0], DDPMScheduler)
    flow = json.load(open(os.path.join(ROOT, "config", "config_synthetic_rflow.json")))["NoiseScheduler"]
    sch, kw = train_diffusion.build_noise_scheduler(flow)
    assert isinstance(sch, RFlowScheduler) and sch.sample_method == flow["sample_method"] and sch.num_train_timesteps == 1000
    assert sch.use_timestep_transform is flow["use_timestep_transform"] and sch.base_img_size_numel == flow["base_img_size_numel"]
    again = RFlowScheduler(**kw)                                   # what the validation sample rebuilds
    assert again.sample_method == sch.sample_method and again.use_discrete_timesteps == sch.use_discrete_timesteps
    with pytest.raises(ValueError, match="sample_method"):
        train_diffusion.build_noise_scheduler(dict(flow, sample_method="cosine"))
    with pytest.raises(ValueError, match="scheduler"):
        train_diffusion.build_noise_scheduler(dict(flow, scheduler="edm"))
