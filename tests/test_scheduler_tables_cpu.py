"""What the schedulers hand to the device sampler and what the inferer refuses, pinned on the host.  The coefficient tables are pure
fp64 / fp32 host arithmetic, so they are compared with ``==`` against tests/golden/scheduler_tables.json (``python
tests/test_scheduler_tables_cpu.py`` rewrites it); the refusal table says, per scheduler class and entry, which exception names which
class.  No GPU."""
import json
import os

import pytest
import torch

import cfgs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scheduler_tables.json")
N_STEPS = 10
PREDS = ("epsilon", "sample", "v_prediction")
CLASSES = ("DDPMScheduler", "DDIMScheduler", "PNDMScheduler", "DPMSolverMultistepScheduler", "RFlowScheduler")


def _make(name, **kw):
    from ldm3d import schedulers
    sch = getattr(schedulers, name)(**kw) if name == "RFlowScheduler" else getattr(schedulers, name)(**dict(cfgs.SCHED, **kw))
    sch.set_timesteps(N_STEPS)
    return sch


def _tables() -> dict:
    """Every table by a name that says how it was made: 1000 training timesteps, 10 inference steps."""
    from ldm3d.schedulers import _sampler_rows, repaint_rows
    out = {}

    def put(name, kind_rows):
        out[name] = dict(kind=kind_rows[0], rows=[list(r) for r in kind_rows[1]])

    for pred in PREDS:
        put(f"rows/ddpm/{pred}", _sampler_rows(_make("DDPMScheduler", prediction_type=pred)))
        for eta in (0.0, 0.5):
            put(f"rows/ddim/{pred}/eta{eta}", _sampler_rows(_make("DDIMScheduler", prediction_type=pred), eta))
        for algo in ("dpmsolver++", "sde-dpmsolver++"):
            put(f"rows/dpm/{pred}/{algo}", _sampler_rows(_make("DPMSolverMultistepScheduler", prediction_type=pred, algorithm_type=algo)))
    for pred in ("epsilon", "v_prediction"):
        for skip in (False, True):
            put(f"rows/pndm/{pred}/skip_prk{int(skip)}", _sampler_rows(_make("PNDMScheduler", prediction_type=pred, skip_prk_steps=skip)))
    put("rows/flow", _sampler_rows(_make("RFlowScheduler")))
    for key, sch in (("ddpm", _make("DDPMScheduler")), ("ddim", _make("DDIMScheduler")), ("flow", _make("RFlowScheduler"))):
        schedule, rows = repaint_rows(sch, jump_length=2, n_resample=2)
        out[f"repaint/{key}"] = dict(schedule=[[level, bool(jump)] for level, jump in schedule], rows=[list(r) for r in rows])
    for pred in PREDS:
        ddim = _make("DDIMScheduler", prediction_type=pred)
        out[f"inversion/ddim/{pred}"] = dict(timesteps=ddim.inversion_timesteps(),
                                             rows=[ddim._inversion_row(t) for t in ddim.inversion_timesteps()])
    return out


def test_tables_equal_the_recorded_ones():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = _tables()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], name                 # Python floats against Python floats: bit for bit
    assert [want[f"rows/{k}"]["kind"] for k in ("ddpm/epsilon", "ddim/epsilon/eta0.0", "pndm/epsilon/skip_prk0", "flow",
                                                "dpm/epsilon/dpmsolver++")] == [0, 1, 2, 3, 4]


def _refused(cls, entry) -> bool:
    """Today's table: the multistep samplers have no warm start and no inpainting; only DDIM inverts; only DDPM scores a likelihood."""
    if entry in ("warm_start", "inpaint", "repaint_rows"):
        return cls in ("PNDMScheduler", "DPMSolverMultistepScheduler")
    return cls != {"invert": "DDIMScheduler", "get_likelihood": "DDPMScheduler"}[entry]


@pytest.mark.parametrize("entry", ["warm_start", "inpaint", "repaint_rows", "invert", "get_likelihood"])
@pytest.mark.parametrize("cls", CLASSES)
def test_refusal_table(cls, entry):
    """A refusal is a NotImplementedError that names the scheduler it refuses (invert / get_likelihood: the one they need, then the one
    given).  Where nothing is refused the check returns, or the entry goes on to the device boundary: these latents are CPU tensors."""
    from ldm3d._lib import LdmError
    from ldm3d.inferer import LatentDiffusionInferer, _check_inpaint, _check_warm_start
    from ldm3d.schedulers import repaint_rows
    sch = _make(cls, **(dict(skip_prk_steps=True) if cls == "PNDMScheduler" else {}))
    inf = LatentDiffusionInferer(sch)
    z, keep = torch.zeros((1, 4, 2, 2, 2)), torch.ones((2, 2, 2))
    calls = dict(warm_start=lambda: _check_warm_start(sch, len(sch.timesteps), z, 1, 1),
                 inpaint=lambda: _check_inpaint(sch, z, keep, None, 0, z.shape),
                 repaint_rows=lambda: repaint_rows(sch, 2, 2),
                 invert=lambda: inf.invert(z, None),
                 get_likelihood=lambda: inf.get_likelihood(z, None, None, verbose=False))
    if _refused(cls, entry):
        match = {"invert": f"DDIMScheduler, you are using {cls}", "get_likelihood": f"DDPMScheduler, you are using {cls}"}.get(entry, cls)
        with pytest.raises(NotImplementedError, match=match):
            calls[entry]()
        if entry == "warm_start":                            # the same refusal through the public entries
            with pytest.raises(NotImplementedError, match=cls):
                inf.sample(z, None, None, init_latent=z, start_step=1)
            with pytest.raises(NotImplementedError, match=cls):
                inf.sample_sliding_window(z, None, None, (2, 2, 2), init_latent=z, start_step=1)
        elif entry == "inpaint":
            with pytest.raises(NotImplementedError, match=cls):
                inf.sample(z, None, None, inpaint_latent=z, keep_mask=keep)
    elif entry in ("invert", "get_likelihood"):
        with pytest.raises(LdmError, match="a CUDA latent"):
            calls[entry]()
    elif entry == "warm_start":
        assert calls[entry]() == 1
    elif entry == "inpaint":
        known, k = calls[entry]()
        assert known.shape == z.shape and k.shape == keep.shape
    else:
        schedule, rows = calls[entry]()
        assert len(schedule) == len(rows) == N_STEPS + 2 * ((N_STEPS - 1) // 2)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(GOLDEN, "w") as f:
        json.dump(_tables(), f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
