"""PNDMScheduler on the host (no GPU): timestep lists, argument checks, and the coefficient-row table the step kernels are programmed by
against the fp64 restatement tests/pndm_ref.py.

The PNDM step is linear in (x, every model output), so a chain is followed exactly with coefficient vectors instead of tensors: the
initial x is basis vector 0 and the model output of call j is basis vector j + 1.  ``apply_row`` is the row format's definition
(csrc/norm_elem.h), evaluated in fp64 on the fp32-rounded row."""
import numpy as np
import pytest
import torch

import cfgs
from pndm_ref import PNDMRef

PUSH, SAVE, USE_SAVED, ACC_SET, ACC_ADD = 1, 2, 4, 8, 16
U = 2.0 ** -24                                            # one fp32 rounding, relative


def test_known_answer_timesteps():
    from ldm3d.schedulers import PNDMScheduler
    s = PNDMScheduler(num_train_timesteps=1000, skip_prk_steps=True)
    assert len(s.timesteps) == 1001 and s.pndm_order == 4    # the constructor ends with set_timesteps(num_train_timesteps)
    s.set_timesteps(10)
    assert s.timesteps.dtype == torch.int64
    assert s.timesteps.tolist() == [900, 800, 800, 700, 600, 500, 400, 300, 200, 100, 0]
    s = PNDMScheduler(num_train_timesteps=1000)
    s.set_timesteps(50)
    assert s.timesteps.tolist() == [980, 970, 970, 960, 960, 950, 950, 940, 940, 930, 930, 920] + list(range(920, -1, -20))
    assert len(s.timesteps) == 59
    assert s.ets == [] and s.counter == 0 and s.cur_sample is None and s.cur_model_output == 0
    assert float(s.final_alpha_cumprod) == float(s.alphas_cumprod[0])
    assert float(PNDMScheduler(set_alpha_to_one=True).final_alpha_cumprod) == 1.0


def test_argument_checks():
    from ldm3d.schedulers import PNDMScheduler
    s = PNDMScheduler()
    with pytest.raises(ValueError):
        s.set_timesteps(3)                                   # the PRK warm-up needs four timesteps
    PNDMScheduler(skip_prk_steps=True).set_timesteps(3)
    with pytest.raises(ValueError):
        PNDMScheduler(prediction_type="sample")
    with pytest.raises(TypeError):
        PNDMScheduler(clip_sample=True)                      # no clipping in this class


def test_exported_next_to_ddim():
    import ldm3d.schedulers as a
    from ldm3d.config import TARGET_ALIASES
    assert issubclass(a.PNDMScheduler, a._Scheduler)
    assert TARGET_ALIASES["monai.networks.schedulers.PNDMScheduler"] == "ldm3d.schedulers.PNDMScheduler"
    for name in ("add_noise", "get_velocity", "add_noise_and_target"):           # the noising methods are inherited
        assert getattr(a.PNDMScheduler, name) is getattr(a._Scheduler, name)


def apply_row(row, x, m, hist, saved, acc, v_pred):
    """One call of the row program on coefficient vectors: -> (prev, hist', saved', acc').  hist: pushed outputs, oldest first."""
    cx, ce, sa, sb, flags, _t, wm, w1, w2, w3, wacc, am, head = row[:13]
    flags = int(flags)
    e = wm * m
    for j, w in enumerate((w1, w2, w3), start=1):
        if w != 0.0:
            e = e + w * hist[-j]                              # an IndexError here = the row reads an unwritten slot
    if wacc != 0.0:
        e = e + wacc * acc
    if flags & ACC_SET:
        acc = am * m
    elif flags & ACC_ADD:
        acc = acc + am * m
    xs = saved if flags & USE_SAVED else x
    if v_pred:
        e = sa * e + sb * xs
    prev = cx * xs + ce * e
    if flags & PUSH:
        hist = hist + [m]
    if flags & SAVE:
        saved = x
    return prev, hist, saved, acc


CASES = [dict(n=n, skip=skip, pred=pred, one=one, off=off)
         for n in (10, 50) for skip in (True, False) for pred in ("epsilon", "v_prediction") for one, off in ((False, 0), (True, 1))]
CASES += [dict(n=10, skip=True, pred="epsilon", one=True, off=0), dict(n=50, skip=False, pred="v_prediction", one=False, off=1)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"n{c['n']}-{'plms' if c['skip'] else 'prk'}-{c['pred'][0]}-one{int(c['one'])}-off{c['off']}")
def test_row_table_equals_the_fp64_reference(case):
    """Call by call, from the reference's own state: the row applied to that state == the reference's step, to the fp32 rounding of
    the row's entries (<= 3 rounded factors per term: 4 U of the terms' absolute sum, per component); the state it leaves is the
    reference's."""
    from ldm3d.schedulers import PNDMScheduler, _sampler_rows
    kw = dict(skip_prk_steps=case["skip"], set_alpha_to_one=case["one"], prediction_type=case["pred"], steps_offset=case["off"])
    sch = PNDMScheduler(**cfgs.SCHED, **kw)
    ref = PNDMRef(**cfgs.SCHED, **kw)
    sch.set_timesteps(case["n"])
    ref.set_timesteps(case["n"])
    ts = sch.timesteps.tolist()
    assert ts == ref.timesteps.tolist()
    kind, rows = _sampler_rows(sch)
    assert kind == 2 and len(rows) == len(ts) and all(len(r) == 16 for r in rows)
    rows = np.asarray(rows, dtype=np.float32).astype(np.float64)                 # what the device table holds
    K = len(ts)
    basis = torch.eye(K + 1, dtype=torch.float64)
    x = basis[0]
    pushes, acc_weight = 0, 0.0
    for k, t in enumerate(ts):
        row = rows[k]
        assert row[5] == float(t) and row[12] == float(pushes) and row[13:].tolist() == [0.0, 0.0, 0.0]
        m = basis[k + 1]
        hist = [h.clone() for h in ref.ets]
        saved = ref.cur_sample
        acc = ref.cur_model_output if torch.is_tensor(ref.cur_model_output) else None
        want, _ = ref.step(m, t, x)
        got, hist2, saved2, acc2 = apply_row(row, x, m, hist, saved, acc, case["pred"] == "v_prediction")
        # the terms' absolute sum, per component: the same row program on absolute values
        mag = apply_row(np.abs(row), x.abs(), m.abs(), [h.abs() for h in hist], None if saved is None else saved.abs(),
                        None if acc is None else acc.abs(), case["pred"] == "v_prediction")[0]
        wsum = abs(row[6]) + abs(row[7]) + abs(row[8]) + abs(row[9]) + abs(row[10])
        assert bool(((got - want).abs() <= 4 * U * mag).all()), (k, t, float(((got - want).abs() / mag.clamp_min(1e-300)).max()) / U)
        # the weights of one call sum to 1 (the accumulator stands for the outputs it has summed)
        flags = int(row[4])
        if flags & ACC_SET:
            acc_weight = row[11]
        elif flags & ACC_ADD:
            acc_weight += row[11]
        total = row[6] + row[7] + row[8] + row[9] + row[10] * (acc_weight if row[10] != 0.0 else 0.0)
        assert abs(total - 1.0) <= 4 * U * max(1.0, wsum), (k, total)
        # the state the row leaves == the reference's
        if flags & PUSH:
            pushes += 1
        n_keep = len(ref.ets)
        assert len(hist2) >= n_keep and all(torch.equal(a, b) for a, b in zip(hist2[-n_keep:], ref.ets))
        if ref.cur_sample is not None:
            assert torch.equal(saved2, ref.cur_sample)
        if torch.is_tensor(ref.cur_model_output):
            assert float((acc2 - ref.cur_model_output).abs().max()) <= 2 * U
        x = want
    # the chain as a whole never needed more than the three previous outputs plus the current one
    assert pushes == (K - 1 if case["skip"] else 3 + K - 12)


def test_cli_scheduler_choice():
    import os
    import sys
    import types
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import inference
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler, PNDMScheduler
    section = {"num_train_timesteps": 1000, "beta_start": 0.0015, "beta_end": 0.0195, "prediction_type": "v_prediction"}
    ns = types.SimpleNamespace(NoiseScheduler=section, steps=6, sampler="pndm", pndm_prk=False)
    s = inference.make_scheduler(ns)
    assert isinstance(s, PNDMScheduler) and s.skip_prk_steps and float(s.final_alpha_cumprod) == 1.0
    assert len(s.timesteps) == 7 and s.prediction_type == "v_prediction"
    ns.pndm_prk = True
    s = inference.make_scheduler(ns)
    assert not s.skip_prk_steps and len(s.timesteps) == 12 + 3 and float(s.final_alpha_cumprod) == float(s.alphas_cumprod[0])
    assert isinstance(inference.make_scheduler(types.SimpleNamespace(NoiseScheduler=section, steps=6, sampler="ddim")), DDIMScheduler)
    assert isinstance(inference.make_scheduler(types.SimpleNamespace(NoiseScheduler=section, steps=0, sampler="ddpm")), DDPMScheduler)
    assert isinstance(inference.make_scheduler(types.SimpleNamespace(NoiseScheduler=section, steps=6, sampler="auto")), DDIMScheduler)
