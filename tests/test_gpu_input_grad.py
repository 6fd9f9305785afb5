"""Gradients w.r.t. the UNet input (-m gpu): ``DiffusionModelUNet.forward`` with ``x`` / ``cond`` requiring grad, through
ldm_unet_train_backward_input (the training tape, conv3_dgrad_thin_kernel at its end, and the data-only plan when every parameter is
frozen).

Checker: torch autograd through the CPU oracle with ``x.requires_grad_(True)``, an MSE loss to a seeded target, gain 0.5 weights and the
seeds of test_gpu_train.py.  The bf16 gates are the project's standing ones against the oracle's own bf16-versus-fp32 input-gradient
floor, recomputed here (measured at these shapes, in the order of SHAPES: 1.70e-2, 1.42e-2, 1.57e-2): rel-L2 <= 1.5 floor + 2e-3 against fp32
autograd and against the bf16 oracle, per input channel <= 2.5 x that channel's floor + 5e-3.  fp32 mode at unit gain: <= 1e-3.
"""
import pytest
import torch
import torch.nn.functional as F

import cfgs
from util import rel_l2

pytestmark = pytest.mark.gpu

SHAPES = [("UNET_TINY", (8, 8, 8), 2, 0), ("UNET_TINY_ALT", (6, 10, 8), 1, 0), ("UNET_TINY_COND", (8, 12, 4), 1, 4)]
_CACHE = {}


def _case(name, dims, b, gain):
    """Seeded weights, input, target and timesteps of a case, with the oracle's fp32 (and, at gain 0.5, bf16) input gradients: computed once."""
    key = (name, dims, b, gain)
    if key not in _CACHE:
        from oracle import unet as ou
        cfg = getattr(cfgs, name)
        sd = ou.init_state_dict(ou.unet_param_shapes(cfg), 3, gain=gain)
        g = torch.Generator().manual_seed(4)
        x = torch.randn((b, cfg["in_channels"], *dims), generator=g)
        target = torch.randn((b, cfg["out_channels"], *dims), generator=g)
        t = torch.tensor([211.0, 640.0][:b])

        def dx(bf):
            xr = x.clone().requires_grad_(True)
            F.mse_loss(ou.unet_forward(sd, cfg, xr, t, emulate_bf16=bf), target).backward()
            return xr.grad.detach()
        _CACHE[key] = dict(cfg=cfg, sd=sd, x=x, target=target, t=t, g32=dx(False), gbf=dx(True) if gain != 1.0 else None)
    return _CACHE[key]


def _model(c, cuda, train=True):
    from ldm3d.networks import DiffusionModelUNet
    m = DiffusionModelUNet(**c["cfg"])
    m.load_state_dict(c["sd"])
    m = m.to(cuda)
    return m.train() if train else m.eval()


def _forward(m, c, cuda, cond, grad_x=True, grad_c=True):
    """One grad-enabled forward and the MSE loss; returns (loss, x leaf, cond leaf or None)."""
    xd = c["x"].to(cuda)
    if cond:
        xl = xd[:, :-cond].contiguous().requires_grad_(grad_x)
        cl = xd[:, -cond:].contiguous().requires_grad_(grad_c)
        out = m(x=xl, timesteps=c["t"].to(cuda), cond=cl)
    else:
        xl, cl = xd.clone().requires_grad_(grad_x), None
        out = m(x=xl, timesteps=c["t"].to(cuda))
    return F.mse_loss(out.float(), c["target"].to(cuda)), xl, cl


def _input_grad(xl, cl):
    parts = [xl.grad] + ([cl.grad] if cl is not None else [])
    return torch.cat([p.detach().cpu() for p in parts], dim=1)


@pytest.mark.parametrize("name,dims,b,cond", SHAPES)
def test_bf16_input_gradients_sit_on_the_oracle_floor(cuda, name, dims, b, cond):
    c = _case(name, dims, b, 0.5)
    m = _model(c, cuda)
    loss, xl, cl = _forward(m, c, cuda, cond)
    loss.backward()
    torch.cuda.synchronize()
    got, g32, gbf = _input_grad(xl, cl), c["g32"], c["gbf"]
    assert got.shape == g32.shape and torch.isfinite(got).all()
    floor = rel_l2(gbf, g32)
    e32, ebf = rel_l2(got, g32), rel_l2(got, gbf)
    print(f"{name} {dims} B{b}: input-gradient floor {floor:.2e}, GPU vs fp32 autograd {e32:.2e}, vs bf16 oracle {ebf:.2e}")
    assert e32 <= 1.5 * floor + 2e-3, (e32, floor)
    assert ebf <= 1.5 * floor + 2e-3, (ebf, floor)
    for ch in range(g32.shape[1]):                    # every input channel has a non-zero gradient: a missing one cannot hide
        assert g32[:, ch].norm() > 0
        fl, e = rel_l2(gbf[:, ch], g32[:, ch]), rel_l2(got[:, ch], g32[:, ch])
        print(f"    channel {ch}: floor {fl:.2e}, GPU {e:.2e}")
        assert e <= 2.5 * fl + 5e-3, (ch, e, fl)
    if cond:                                          # dx and dcond each, not only their concatenation
        nx = g32.shape[1] - cond
        for what, a, r, rb in (("dx", xl.grad.cpu(), g32[:, :nx], gbf[:, :nx]), ("dcond", cl.grad.cpu(), g32[:, nx:], gbf[:, nx:])):
            fl, e = rel_l2(rb, r), rel_l2(a, r)
            print(f"    {what}: floor {fl:.2e}, GPU {e:.2e}")
            assert a.shape == r.shape and e <= 1.5 * fl + 2e-3, (what, e, fl)


@pytest.mark.parametrize("name,dims,b,cond", SHAPES)
def test_fp32_mode_input_gradients_match_fp32_autograd_at_unit_gain(cuda, name, dims, b, cond):
    c = _case(name, dims, b, 1.0)
    m = _model(c, cuda).set_precision("fp32")
    loss, xl, cl = _forward(m, c, cuda, cond)
    loss.backward()
    torch.cuda.synchronize()
    e = rel_l2(_input_grad(xl, cl), c["g32"])
    print(f"{name} {dims} B{b} fp32 mode, unit gain: input gradient vs fp32 autograd {e:.2e} (gate 1e-3)")
    assert e <= 1e-3, e


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_thin_kernel_plan_meets_the_same_gates(cuda, monkeypatch, precision):
    """LDM_DGRAD_THIN=1 (read when the plan is built): conv_in's data gradient on conv3_dgrad_thin_kernel instead of the default general
    data-gradient conv + unpack; dx and dcond against the same references at the same gates."""
    monkeypatch.setenv("LDM_DGRAD_THIN", "1")
    name, dims, b, cond = SHAPES[2]
    c = _case(name, dims, b, 0.5 if precision == "bf16" else 1.0)
    m = _model(c, cuda)
    if precision == "fp32":
        m.set_precision("fp32")
    loss, xl, cl = _forward(m, c, cuda, cond)
    loss.backward()
    torch.cuda.synchronize()
    got, g32 = _input_grad(xl, cl), c["g32"]
    e = rel_l2(got, g32)
    if precision == "fp32":
        print(f"thin plan, fp32 mode, unit gain: {e:.2e} (gate 1e-3)")
        assert e <= 1e-3
    else:
        floor = rel_l2(c["gbf"], g32)
        print(f"thin plan, bf16 mode: {e:.2e} at floor {floor:.2e}")
        assert e <= 1.5 * floor + 2e-3
        for ch in range(g32.shape[1]):
            assert rel_l2(got[:, ch], g32[:, ch]) <= 2.5 * rel_l2(c["gbf"][:, ch], g32[:, ch]) + 5e-3, ch


def test_one_backward_yields_parameter_and_input_gradients(cuda):
    """The parameter gradients of a step that also asks for dx are those of the same step without it, bit for bit."""
    c = _case("UNET_TINY_COND", (8, 12, 4), 1, 0.5)
    m = _model(c, cuda)
    loss, xl, cl = _forward(m, c, cuda, 4, grad_x=False, grad_c=False)
    loss.backward()
    plain = {k: p.grad.clone() for k, p in m.named_parameters()}
    assert xl.grad is None and cl.grad is None
    m.zero_grad(set_to_none=True)
    loss, xl, cl = _forward(m, c, cuda, 4)
    loss.backward()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, plain[k]), k
    assert rel_l2(_input_grad(xl, cl), c["g32"]) <= 1.5 * rel_l2(c["gbf"], c["g32"]) + 2e-3


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_frozen_parameters_run_the_data_only_plan(cuda, mode):
    """Every parameter frozen: dx is torch.equal to the full backward's, no .grad appears and no byte of flat_grads changes."""
    from ldm3d import _lib
    c = _case("UNET_TINY", (8, 8, 8), 2, 0.5)
    m = _model(c, cuda)
    loss, xl, _ = _forward(m, c, cuda, 0)
    loss.backward()
    full = xl.grad.clone()
    m.zero_grad(set_to_none=True)
    m.requires_grad_(False)
    if mode == "eval":
        m.eval()
    total = int(_lib.lib().ldm_model_param_numel_total(m._h))
    m.flat_grads = torch.full((total,), 12345.0, dtype=torch.float32, device=cuda)   # what a flat-gradient trainer would have attached
    loss, xl, _ = _forward(m, c, cuda, 0)
    assert loss.requires_grad
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(xl.grad, full)
    assert all(p.grad is None for p in m.parameters())
    assert bool((m.flat_grads == 12345.0).all())
    assert int(_lib.lib().ldm_model_grad_sync_pending(m._h)) == 0


def test_only_cond_requires_grad(cuda):
    c = _case("UNET_TINY_COND", (8, 12, 4), 1, 0.5)
    m = _model(c, cuda)
    m.requires_grad_(False)
    loss, xl, cl = _forward(m, c, cuda, 4, grad_x=False)
    loss.backward()
    torch.cuda.synchronize()
    assert xl.grad is None
    g32, gbf = c["g32"][:, -4:], c["gbf"][:, -4:]
    e, fl = rel_l2(cl.grad.cpu(), g32), rel_l2(gbf, g32)
    print(f"cond only: dcond vs fp32 autograd {e:.2e} (floor {fl:.2e})")
    assert cl.grad.shape == g32.shape and e <= 1.5 * fl + 2e-3


def test_backward_of_a_stale_forward_still_raises(cuda):
    from ldm3d import _lib
    c = _case("UNET_TINY", (8, 8, 8), 2, 0.5)
    m = _model(c, cuda)
    m.requires_grad_(False)
    loss1, _, _ = _forward(m, c, cuda, 0)
    loss2, xl2, _ = _forward(m, c, cuda, 0)
    with pytest.raises(_lib.LdmError, match="stale forward"):
        loss1.backward()
    loss2.backward()
    assert torch.isfinite(xl2.grad).all()


def test_all_null_backward_is_refused_and_other_inputs_still_raise(cuda):
    from ldm3d import _lib
    c = _case("UNET_TINY", (8, 8, 8), 2, 0.5)
    m = _model(c, cuda)
    L = _lib.lib()
    g = torch.zeros((2, 4, 8, 8, 8), device=cuda)
    ws = torch.empty(int(L.ldm_unet_train_input_workspace_bytes(m._h, 2, 8, 8, 8)) + 256, dtype=torch.uint8, device=cuda)
    rc = L.ldm_unet_train_backward_input(m._h, g.data_ptr(), None, None, None, 2, 8, 8, 8, ws.data_ptr(), ws.numel(),
                                         torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"NULL" in L.ldm_last_error()
    x = c["x"].to(cuda).requires_grad_(True)
    with pytest.raises(NotImplementedError):
        m(x=x, timesteps=c["t"].to(cuda), context=torch.zeros(1, device=cuda))
    with pytest.raises(NotImplementedError):
        m(x=x, timesteps=c["t"].to(cuda), class_labels=torch.zeros(1, device=cuda))
