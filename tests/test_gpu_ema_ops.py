"""Per-kernel parity of the EMA forms of the optimizer step (-m gpu): ldm_adam_step_ema and ldm_model_adam_step_ema called directly, in the
pattern of tests/test_gpu_optim_ops.py, against the float64 restatement tests/ema_ref.py on exactly the values the kernels read.

Gates: p, m, v and ema rel-L2 <= 1e-5 (TOL_EXACT of test_gpu_f32_ops.py) against float64 after every step.  With lr = 0.05 on unit-scale
parameters and these decays an error of 1e-3 in (1 - d) moves the EMA by more than 2e-5 of its scale.  p, m, v bit-identical to ldm_adam_step
on copies of the same buffers (the EMA must not perturb the optimizer); three guard elements behind n untouched in all five buffers; a repeat
from the same inputs bit-identical (one writer per element, no atomics).  Every buffer of these entries is read before it is written, so there
is no pure output to fill with NaN: the guards carry NaN / sentinels instead.  A skipped step leaves all four buffers bit-identical, and the
update after it uses the warm-up of the applied-update count (2/11), not of the call count (3/12).  Refusals are checked only for arguments
the launchers reject before any launch.  Measured values are printed (-s) and quoted in the docstrings.
"""
import numpy as np
import pytest
import torch

import cfgs
import ema_ref as E
import gan_ops_ref as R
from test_gpu_f32_ops import TOL_EXACT, _call, _p, _rel, _stream
from test_gpu_optim_ops import ADAM, ADAMW, EPS, ERR_BAD_ARG, LR, _bits_equal, _L

pytestmark = pytest.mark.gpu
EMA_MODES = {"warmup_0p999": (R.f32(0.999), 1), "constant_0p5": (R.f32(0.5), 0)}


def _ema_launch(p, g, m, v, ema, n, hp, step, decay, warm, sq, max_norm):
    _call("ldm_adam_step_ema", _p(p), _p(g), _p(m), _p(v), _p(ema), n, LR, hp["b1"], hp["b2"], EPS, hp["wd"], step, decay, warm, _p(sq),
          max_norm, _stream())


def _plain_launch(p, g, m, v, n, hp, step, sq, max_norm):
    _call("ldm_adam_step", _p(p), _p(g), _p(m), _p(v), n, LR, hp["b1"], hp["b2"], EPS, hp["wd"], step, _p(sq), max_norm, _stream())


@pytest.mark.parametrize("n", [1, 255, 257, (1 << 21) + 5])
@pytest.mark.parametrize("ema_mode", list(EMA_MODES))
@pytest.mark.parametrize("mode", ["adam_clip_binds", "adamw_max_norm_0"])
def test_adam_step_ema_three_steps(cuda, n, mode, ema_mode):
    """adam_step_kernel<true>, three consecutive steps from zero moments: Adam (0.9, 0.999) with a clip that binds and AdamW (0.5, 0.9, wd
    1e-2, max_norm 0), each with the warm-up on (d = 0.1, 2/11, 3/12 under decay 0.999) and off at decay 0.5; n = 2^21 + 5 is past the
    8192 x 256 grid.  Measured rel-L2 over all cases: p <= 1.4e-07, m <= 9.6e-08, v <= 2.0e-07, ema <= 1.2e-07 (gate 1e-5)."""
    hp = ADAM if mode.startswith("adam_") else ADAMW
    decay, warm = EMA_MODES[ema_mode]
    gen = torch.Generator().manual_seed(n % 1000 + len(mode) + len(ema_mode))
    p0, e0 = torch.randn((n + 3,), generator=gen), torch.randn((n + 3,), generator=gen)
    e0[n:] = float("nan")
    pd, md, vd, ed = p0.to(cuda), torch.zeros((n + 3,), device=cuda), torch.zeros((n + 3,), device=cuda), e0.to(cuda)
    md[n:], vd[n:] = 7.0, 9.0
    p, m, v, ema = p0[:n].double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), e0[:n].double()
    worst = [0.0] * 4
    for step in (1, 2, 3):
        gr = torch.randn((n + 3,), generator=gen)
        gr[n:] = float("nan")
        sq32 = np.float32(float((gr[:n].double() ** 2).sum()))                  # the fp32 norm the kernel reads
        max_norm = R.f32(0.3 * float(sq32) ** 0.5) if mode == "adam_clip_binds" else 0.0
        if mode == "adam_clip_binds":
            assert R.clip_factor(float(sq32), max_norm) < 0.31
        sq = torch.tensor([float(sq32), 0.0], device=cuda)
        gd = gr.to(cuda)
        pc, mc, vc = pd.clone(), md.clone(), vd.clone()                          # ldm_adam_step on copies: the optimizer without EMA
        _plain_launch(pc, gd, mc, vc, n, hp, step, sq, max_norm)
        if step == 1:                                                             # a repeat from the same inputs
            rep = [t.clone() for t in (pd, md, vd, ed)]
            _ema_launch(*rep[:1], gd, *rep[1:], n, hp, step, decay, warm, sq, max_norm)
        _ema_launch(pd, gd, md, vd, ed, n, hp, step, decay, warm, sq, max_norm)
        torch.cuda.synchronize()
        assert _bits_equal(pd, pc) and _bits_equal(md, mc) and _bits_equal(vd, vc), "the EMA form changed p, m or v"
        if step == 1:
            assert all(_bits_equal(a, b) for a, b in zip(rep, (pd, md, vd, ed))), "a repeat launch differs"
        assert _bits_equal(gd, gr), "the gradients were written"
        p, m, v, ema, _ = E.adam_ema_ref(p, gr[:n], m, v, ema, LR, hp["b1"], hp["b2"], EPS, hp["wd"], step, 0, decay, warm, float(sq32), max_norm)
        for j, (got, ref, name) in enumerate(((pd, p, "p"), (md, m, "m"), (vd, v, "v"), (ed, ema, "ema"))):
            got = got.cpu()
            assert torch.isfinite(got[:n]).all()
            e = _rel(got[:n], ref)
            worst[j] = max(worst[j], e)
            assert e <= TOL_EXACT, (mode, ema_mode, n, step, name, e)
        assert float(sq.cpu()[1]) == 0.0, "the skip counter moved on a good step"
    assert torch.equal(pd[n:].cpu(), p0[n:]) and float(md[n]) == 7.0 and float(vd[n + 2]) == 9.0 and torch.isnan(ed[n:]).all(), "wrote past n"
    print(f"adam_step_ema {mode} {ema_mode} n={n}: worst rel-L2 over three steps p {worst[0]:.2e}, m {worst[1]:.2e}, v {worst[2]:.2e}, "
          f"ema {worst[3]:.2e} (gate {TOL_EXACT:.0e})")


@pytest.mark.parametrize("n", [257, (1 << 21) + 5])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_adam_step_ema_skip_contract(cuda, n, bad):
    """good step, non-finite sq_norm[0], good step: on the middle call p, m, v and ema stay bit-identical and the counter goes up by one; the
    third call is the SECOND applied update: bias corrections of step 2 and d = 2/11, gated against float64.  Control: d = 3/12 (the call
    count) moves the EMA far outside the gate.  Measured rel-L2 after the third call: p <= 5.9e-08, m <= 1.2e-07, v <= 1.8e-07,
    ema <= 6.4e-08; control 9.3e-03 ... 1.0e-02."""
    hp, (decay, warm) = ADAMW, EMA_MODES["warmup_0p999"]
    gen = torch.Generator().manual_seed(n % 1000 + 3)
    p0, e0 = torch.randn((n,), generator=gen), torch.randn((n,), generator=gen)
    pd, md, vd, ed = p0.to(cuda), torch.zeros((n,), device=cuda), torch.zeros((n,), device=cuda), e0.to(cuda)
    st = (p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), e0.double(), 0)
    sq = torch.zeros((2,), device=cuda)

    def call(step, sq0):
        nonlocal st
        gr = torch.randn((n,), generator=gen)
        sq32 = float(np.float32(float((gr.double() ** 2).sum()))) if sq0 is None else sq0
        max_norm = R.f32(0.5 * sq32 ** 0.5) if sq0 is None else 1.0
        sq[0] = sq32
        _ema_launch(pd, gr.to(cuda), md, vd, ed, n, hp, step, decay, warm, sq, max_norm)
        torch.cuda.synchronize()
        prev = st
        st = E.adam_ema_ref(st[0], gr, st[1], st[2], st[3], LR, hp["b1"], hp["b2"], EPS, hp["wd"], step, st[4], decay, warm, sq32, max_norm)
        return prev
    call(1, None)
    kept = [t.clone() for t in (pd, md, vd, ed)]
    call(2, bad)
    assert all(_bits_equal(a, b) for a, b in zip((pd, md, vd, ed), kept)), "a skipped step changed the state"
    assert float(sq.cpu()[1]) == 1.0 and st[4] == 1
    prev = call(3, None)
    errs = [_rel(a.cpu(), b) for a, b in zip((pd, md, vd, ed), st[:4])]
    wrong = prev[3] + (1 - 3 / 12) * (st[0] - prev[3])
    ctl = _rel(wrong, st[3])
    print(f"adam_step_ema skip contract n={n} bad={bad}: third call rel-L2 p {errs[0]:.2e}, m {errs[1]:.2e}, v {errs[2]:.2e}, ema {errs[3]:.2e} "
          f"(gate {TOL_EXACT:.0e}); warm-up of the call count instead of the applied count: {ctl:.1e}")
    assert float(sq.cpu()[1]) == 1.0
    assert max(errs) <= TOL_EXACT, errs
    assert ctl > 10 * TOL_EXACT


@pytest.mark.parametrize("case", ["ema_null", -0.1, 1.0, float("nan")])
def test_adam_step_ema_refusals(cuda, case):
    """ema = NULL and ema_decay outside [0, 1) (NaN included) return LDM_ERR_BAD_ARG before any launch: every buffer is untouched."""
    n = 300
    gen = torch.Generator().manual_seed(11)
    bufs = [torch.randn((n,), generator=gen).to(cuda) for _ in range(5)]         # p, g, m, v, ema
    sq = torch.tensor([1.0, 0.0], device=cuda)
    kept = [t.clone() for t in bufs] + [sq.clone()]
    p, g, m, v, ema = bufs
    decay = 0.9 if case == "ema_null" else case
    rc = _L().ldm_adam_step_ema(_p(p), _p(g), _p(m), _p(v), None if case == "ema_null" else _p(ema), n, LR, ADAM["b1"], ADAM["b2"], EPS, 0.0, 1,
                                decay, 1, _p(sq), 1.0, _stream())
    torch.cuda.synchronize()
    assert rc == ERR_BAD_ARG
    assert all(_bits_equal(a, b) for a, b in zip(bufs + [sq], kept))


# ------------------------------------------------------------------------------------------------ ldm_model_adam_step_ema
def _make(cfg_name, cuda, precision, seed):
    from ldm3d.networks import AutoencoderKL, DiffusionModelUNet
    cfg = getattr(cfgs, cfg_name)
    cls = AutoencoderKL if cfg_name.startswith("VAE") else DiffusionModelUNet
    torch.manual_seed(seed)
    a = cls(**cfg)
    with torch.no_grad():                                      # MONAI zero-initialises some convs: give every weight a value
        for q in a.parameters():
            if q.dim() > 1 and not bool(q.any()):
                q.normal_(0.0, 0.05)
    b = cls(**cfg)
    b.load_state_dict(a.state_dict())
    mods = []
    for mod in (a, b):
        mod = mod.to(cuda).eval()
        if precision == "fp32":
            mod.set_precision("fp32")
        mod.flatten_parameters()
        mod._sync_weights()                                    # arena packed, nothing stale: the forwards below re-pack nothing
        mods.append(mod)
    return mods


def _forward(mod, cuda):
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        if hasattr(mod, "encode"):
            x = torch.rand((1, 2, 16, 16, 16), generator=gen).to(cuda)
            mu, _ = mod.encode(x)
            return torch.cat([mu.reshape(-1), mod.decode(mu).reshape(-1)]).clone()
        x = torch.randn((1, 4, 8, 8, 8), generator=gen).to(cuda)
        return mod(x=x, timesteps=torch.tensor([500.0], device=cuda)).clone()


@pytest.mark.parametrize("cfg_name,precision", [("UNET_TINY", "bf16"), ("UNET_TINY_ODD", "bf16"), ("VAE_TINY", "bf16"), ("UNET_TINY", "fp32")])
def test_model_adam_step_ema(cuda, cfg_name, precision):
    """adam_pack_batched_kernel<true> on UNET_TINY, UNET_TINY_ODD (96 channels: cin no multiple of the 64-wide pack chunk) and VAE_TINY
    (cin = 2), two steps: flat p, m, v and ema bit-identical to ldm_adam_step_ema on copies (the block map updates every element exactly
    once), and the forward afterwards bit-identical to the one after ldm_model_adam_step from the same start (the arena is packed from the
    live weights, not from the EMA, which starts far from them here).  One case in the fp32 precision mode (pack32_device after the kernel).
    A NULL EMA buffer is refused with the model untouched."""
    a, b = _make(cfg_name, cuda, precision, seed=21)
    n = a.flat_params.numel()
    gen = torch.Generator().manual_seed(8)
    hp = ADAMW
    m_a, v_a, m_b, v_b = (torch.zeros(n, device=cuda) for _ in range(4))
    ema_a = torch.randn((n,), generator=gen).to(cuda)
    raw = [a.flat_params.clone(), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda), ema_a.clone()]
    out0 = _forward(a, cuda)
    assert _bits_equal(out0, _forward(b, cuda))
    L = _L()
    rc = L.ldm_model_adam_step_ema(a._h, _p(a.flat_params), _p(raw[1]), _p(m_a), _p(v_a), None, LR, hp["b1"], hp["b2"], EPS, hp["wd"], 1,
                                   0.9, 1, None, 0.0, _stream())
    assert rc == ERR_BAD_ARG and _bits_equal(a.flat_params, raw[0]) and _bits_equal(_forward(a, cuda), out0)
    decay, warm = EMA_MODES["warmup_0p999"]
    for step in (1, 2):
        gr = (0.1 * torch.randn((n,), generator=gen)).to(cuda)
        sq = torch.tensor([float((gr.double() ** 2).sum()), 0.0], device=cuda)
        max_norm = R.f32(0.5 * float(sq[0]) ** 0.5)
        _call("ldm_model_adam_step_ema", a._h, _p(a.flat_params), _p(gr), _p(m_a), _p(v_a), _p(ema_a), LR, hp["b1"], hp["b2"], EPS, hp["wd"],
              step, decay, warm, _p(sq), max_norm, _stream())
        _call("ldm_model_adam_step", b._h, _p(b.flat_params), _p(gr), _p(m_b), _p(v_b), LR, hp["b1"], hp["b2"], EPS, hp["wd"], step, _p(sq),
              max_norm, _stream())
        _ema_launch(raw[0], gr, raw[1], raw[2], raw[3], n, hp, step, decay, warm, sq, max_norm)
        torch.cuda.synchronize()
        for got, ref, name in zip((a.flat_params, m_a, v_a, ema_a), raw, "pmve"):
            assert torch.isfinite(got).all() and _bits_equal(got, ref), (cfg_name, step, name)
        assert _bits_equal(a.flat_params, b.flat_params) and _bits_equal(m_a, m_b) and _bits_equal(v_a, v_b)
    out_a, out_b = _forward(a, cuda), _forward(b, cuda)
    assert torch.isfinite(out_a).all() and _bits_equal(out_a, out_b), "the arena after the EMA form differs from the one after ldm_model_adam_step"
    assert not _bits_equal(out_a, out0), "two steps at lr 0.05 must move the output"
