"""Known answers of the float64 EMA reference (tests/ema_ref.py) that the GPU parity tests gate the kernels against, and the host-side
surface of the feature that needs no GPU (command-line flags).  No GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_ref as E            # noqa: E402
import gan_ops_ref as R        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = dict(lr=R.f32(0.05), b1=R.f32(0.9), b2=R.f32(0.999), eps=R.f32(1e-8), wd=0.0)


def test_warmup_series_and_cap():
    """0.1, 2/11, 3/12, ... capped at decay; without warm-up the decay itself from the first update."""
    assert [E.ema_decay_at(k, 0.999, True) for k in (1, 2, 3)] == [0.1, 2 / 11, 3 / 12]
    assert E.ema_decay_at(9, 0.5, True) == 0.5 and E.ema_decay_at(10, 0.5, True) == 0.5      # 9/18 = 0.5, 10/19 > 0.5
    assert E.ema_decay_at(8, 0.5, True) == 8 / 17
    assert E.ema_decay_at(10 ** 6, 0.999, True) == 0.999
    assert E.ema_decay_at(1, 0.75, False) == 0.75


def test_constant_parameters_leave_the_ema_where_it_is():
    """g = 0 from zero moments: Adam does not move p, and an EMA that starts at p stays at p exactly, warm-up or not."""
    p = torch.tensor([0.5, -2.0, 3.25], dtype=torch.float64)
    z = torch.zeros(3, dtype=torch.float64)
    for warm in (True, False):
        q, m, v, ema, sk = p, z, z, p.clone(), 0
        for step in (1, 2, 3):
            q, m, v, ema, sk = E.adam_ema_ref(q, z, m, v, ema, **HP, step=step, skipped=sk, decay=0.9, warmup=warm)
        assert torch.equal(q, p) and torch.equal(ema, p) and sk == 0


def test_constant_decay_closed_form():
    """constant d and constant p: ema_n = p + d^n (ema_0 - p)"""
    p = torch.tensor([1.0, -3.0], dtype=torch.float64)
    e0 = torch.tensor([4.0, 0.5], dtype=torch.float64)
    z = torch.zeros(2, dtype=torch.float64)
    d = 0.75
    q, m, v, ema = p, z, z, e0
    for n in range(1, 8):
        q, m, v, ema, _ = E.adam_ema_ref(q, z, m, v, ema, **HP, step=n, skipped=0, decay=d, warmup=False)
        assert torch.allclose(ema, p + d ** n * (e0 - p), rtol=1e-14, atol=0)


def test_first_update_weighs_the_new_value_by_0p9():
    """warm-up, first applied update: ema = 0.1 ema_0 + 0.9 p_new"""
    g = torch.Generator().manual_seed(0)
    p0, gr = torch.randn(5, generator=g).double(), torch.randn(5, generator=g)
    z = torch.zeros(5, dtype=torch.float64)
    e0 = torch.randn(5, generator=g).double()
    p1, _, _, ema, _ = E.adam_ema_ref(p0, gr, z, z, e0, **HP, step=1, skipped=0, decay=0.999, warmup=True)
    assert torch.allclose(ema, 0.1 * e0 + 0.9 * p1, rtol=1e-14, atol=0) and not torch.equal(p1, p0)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_skipped_step_changes_nothing_and_does_not_advance_the_warmup(bad):
    """good, skipped, good: the middle call returns its inputs and counter + 1; the third is the SECOND applied update: d = 2/11 and
    the bias corrections of step 2 -- identical to two good steps in a row."""
    g = torch.Generator().manual_seed(1)
    p0, e0 = torch.randn(7, generator=g).double(), torch.randn(7, generator=g).double()
    g1, g2 = torch.randn(7, generator=g), torch.randn(7, generator=g)
    z = torch.zeros(7, dtype=torch.float64)
    kw = dict(**HP, decay=0.999, warmup=True)
    a = E.adam_ema_ref(p0, g1, z, z, e0, step=1, skipped=0, sq_norm=1.0, **kw)
    b = E.adam_ema_ref(a[0], g2, a[1], a[2], a[3], step=2, skipped=a[4], sq_norm=bad, **kw)
    assert all(x is y for x, y in zip(a[:4], b[:4])) and b[4] == 1
    c = E.adam_ema_ref(b[0], g2, b[1], b[2], b[3], step=3, skipped=b[4], sq_norm=1.0, **kw)
    straight = E.adam_ema_ref(a[0], g2, a[1], a[2], a[3], step=2, skipped=0, sq_norm=1.0, **kw)
    assert all(torch.equal(x, y) for x, y in zip(c[:4], straight[:4])) and c[4] == 1
    assert torch.allclose(c[3], a[3] + (1 - 2 / 11) * (c[0] - a[3]), rtol=1e-14, atol=0)
    wrong = a[3] + (1 - 3 / 12) * (c[0] - a[3])                # the warm-up of call 3 instead of applied update 2
    assert float((wrong - c[3]).norm() / c[3].norm()) > 1e-3


def test_entry_points_have_the_ema_flags():
    """train_diffusion.py --ema-decay / --no-ema-warmup / --resume and inference.py --ema exist; the resume help says what is not restored."""
    import subprocess
    for script, flags in (("train_diffusion.py", ("--ema-decay", "--no-ema-warmup", "--resume")), ("inference.py", ("--ema",))):
        r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-1000:]
        for f in flags:
            assert f in r.stdout, (script, f)
        if script == "train_diffusion.py":
            assert "loader order and RNG state are NOT restored" in " ".join(r.stdout.split())


def test_library_declares_the_ema_entries(built_lib):
    from ldm3d import _lib
    for name in ("ldm_adam_step_ema", "ldm_model_adam_step_ema"):
        assert name in _lib.SIGNATURES and getattr(built_lib, name) is not None
