"""Gradient accumulation over micro-batches: what can be checked without a GPU -- the two C entries are declared and bound, the Python
layers take ``grad_accum_steps``, the command line lists the flag and merges it with the config, and the documents name the feature."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "ldm3d.h")).read()


def test_both_entries_are_declared_and_bound(built_lib):
    from ldm3d import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    flat = " ".join(code.split())
    assert "int ldm_op_grad_accumulate(float* acc, const float* g, int64_t n, float scale, int assign, void* stream);" in flat
    assert "int ldm_model_set_grad_accum(ldm_model* m, float* acc_flat , int micro_index, int micro_count);" in flat
    P = C.c_void_p
    assert _lib.SIGNATURES["ldm_op_grad_accumulate"] == (C.c_int, [P, P, C.c_int64, C.c_float, C.c_int, P])
    assert _lib.SIGNATURES["ldm_model_set_grad_accum"] == (C.c_int, [P, P, C.c_int, C.c_int])
    for name in ("ldm_op_grad_accumulate", "ldm_model_set_grad_accum"):
        fn = getattr(built_lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    # both entries carry a comment of their own in the header
    for name in ("ldm_op_grad_accumulate", "ldm_model_set_grad_accum"):
        before = _header().split(f"int {name}(")[0]
        assert before.rstrip().endswith("*/"), name


def test_the_python_layers_take_grad_accum_steps(built_lib):
    from ldm3d.networks import AutoencoderKL, DiffusionModelUNet
    from ldm3d.optim import FlatAdam
    from ldm3d.trainer import DiffusionTrainer
    for cls in (FlatAdam, DiffusionTrainer):
        p = inspect.signature(cls.__init__).parameters["grad_accum_steps"]
        assert p.default == 1, cls
    for name in ("arm", "micro_done"):
        assert callable(getattr(FlatAdam, name))
    assert isinstance(FlatAdam.grads, property)
    for cls in (AutoencoderKL, DiffusionModelUNet):
        assert list(inspect.signature(cls.set_grad_accum).parameters)[:4] == ["self", "acc", "micro_index", "micro_count"]
    doc = DiffusionModelUNet.flatten_parameters.__doc__
    assert "no accumulation" not in doc and "set_grad_accum" in doc


def test_help_lists_the_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_diffusion.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--grad-accum-steps" in r.stdout and "fresh" in r.stdout      # the help says that a resumed run starts a fresh window


def test_the_flag_overrides_the_config_key():
    import train_diffusion as td
    assert td.merge_grad_accum_steps(None, {}) == 1
    assert td.merge_grad_accum_steps(None, {"grad_accum_steps": 4}) == 4
    assert td.merge_grad_accum_steps(2, {"grad_accum_steps": 4}) == 2
    assert td.merge_grad_accum_steps(1, {"grad_accum_steps": 4}) == 1
    for bad in (0, -1):
        with pytest.raises(SystemExit):
            td.merge_grad_accum_steps(bad, {})
    with pytest.raises(SystemExit):
        td.merge_grad_accum_steps(None, {"grad_accum_steps": 2.5})
    args = td.build_parser().parse_args(["--grad-accum-steps", "4"])
    assert args.grad_accum_steps == 4 and td.build_parser().parse_args([]).grad_accum_steps is None


def test_the_launcher_passes_the_flag_through():
    """train_LDM.sh -D '--grad-accum-steps 4': the diffusion stage's flags are handed on word by word."""
    sh = open(os.path.join(ROOT, "train_LDM.sh")).read()
    assert 'D) DM_FLAGS="$OPTARG"' in sh and "run_stage train_diffusion.py $DM_FLAGS" in sh      # unquoted: word-split into flag and value
    assert "--grad-accum-steps" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_documents_name_the_feature():
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "--grad-accum-steps" in readme
    assert "3.13a" in design and "ldm_model_set_grad_accum" in design and "grad_accum_kernel" in design
    section = design.split("### 3.13a")[1].split("## 4.")[0]
    for not_built in ("AutoencoderTrainer", "acc²", "partial window", "unequal micro-batch", "guided-sampling"):
        assert not_built in section, not_built
    assert "convergence" in design        # the quality side is stated as unmeasured
