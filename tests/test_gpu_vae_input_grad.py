"""Gradients w.r.t. the AutoencoderKL decoder's input (-m gpu): ``AutoencoderKL.decode(z)`` with ``z.requires_grad`` through
ldm_vae_decode_grad_forward / _backward (plan "dec_x": the decoder half of the training plan, a data-only backward, the unpack into dz).

Checker: torch autograd through the CPU oracle's decoder with ``z.requires_grad_(True)``, an MSE loss to a seeded target, gain 0.5
weights as in test_gpu_input_grad.py.  The bf16 gates are the project's standing ones against the oracle's own bf16-versus-fp32
latent-gradient floor, recomputed here and printed: rel-L2 <= 1.5 floor + 2e-3 against fp32 autograd and against the bf16 oracle, per
latent channel <= 2.5 x that channel's floor + 5e-3.  fp32 mode at unit gain: <= 1e-3.  The reconstruction of the grad-forward meets the
decode parity gate of test_gpu_models.py (1.5 floor + 1e-3 against both oracles).
"""
import pytest
import torch
import torch.nn.functional as F

import cfgs
from util import rel_l2

pytestmark = pytest.mark.gpu

# (config, latent dims, B): image dims (8, 16, 12), (16, 16, 16), (16, 16, 16).  VAE_TINY_ATTN: attention at the last level and the
# non-local block; VAE_FULL: the 64-channel full-resolution level and the conv_block / conv_thin ends
SHAPES = [("VAE_TINY", (2, 4, 3), 2), ("VAE_TINY_ATTN", (4, 4, 4), 1), ("VAE_FULL", (4, 4, 4), 1)]
_CACHE = {}


def _case(name, dims, b, gain):
    """Seeded weights, latent and target of a case, with the oracle's fp32 (and, at gain 0.5, bf16) reconstructions and latent gradients:
    computed once."""
    key = (name, dims, b, gain)
    if key not in _CACHE:
        from oracle import autoencoder as oa
        from oracle.unet import init_state_dict
        cfg = getattr(cfgs, name)
        sd = init_state_dict(oa.ae_param_shapes(cfg), 3, gain=gain)
        g = torch.Generator().manual_seed(4)
        z = torch.randn((b, cfg["latent_channels"], *dims), generator=g)
        f = 2 ** (len(cfg["channels"]) - 1)
        target = torch.randn((b, cfg["out_channels"], *(f * v for v in dims)), generator=g)

        def run(bf):
            zr = z.clone().requires_grad_(True)
            rec = oa.decode(sd, cfg, zr, emulate_bf16=bf)
            F.mse_loss(rec, target).backward()
            return rec.detach(), zr.grad.detach()
        r32, g32 = run(False)
        rbf, gbf = run(True) if gain != 1.0 else (None, None)
        _CACHE[key] = dict(cfg=cfg, sd=sd, z=z, target=target, r32=r32, g32=g32, rbf=rbf, gbf=gbf)
    return _CACHE[key]


def _model(c, cuda):
    from ldm3d.networks import AutoencoderKL
    m = AutoencoderKL(**c["cfg"])
    m.load_state_dict(c["sd"])
    return m.to(cuda).eval()


def _forward(m, c, cuda):
    zl = c["z"].to(cuda).requires_grad_(True)
    rec = m.decode(zl)
    assert rec.requires_grad
    return F.mse_loss(rec.float(), c["target"].to(cuda)), zl, rec


@pytest.mark.parametrize("name,dims,b", SHAPES)
def test_bf16_latent_gradients_sit_on_the_oracle_floor(cuda, name, dims, b):
    c = _case(name, dims, b, 0.5)
    m = _model(c, cuda)
    loss, zl, rec = _forward(m, c, cuda)
    loss.backward()
    torch.cuda.synchronize()
    got, g32, gbf = zl.grad.cpu(), c["g32"], c["gbf"]
    assert got.shape == g32.shape and torch.isfinite(got).all()
    floor = rel_l2(gbf, g32)
    e32, ebf = rel_l2(got, g32), rel_l2(got, gbf)
    print(f"{name} {dims} B{b}: latent-gradient floor {floor:.2e}, GPU vs fp32 autograd {e32:.2e}, vs bf16 oracle {ebf:.2e}")
    assert e32 <= 1.5 * floor + 2e-3, (e32, floor)
    assert ebf <= 1.5 * floor + 2e-3, (ebf, floor)
    for ch in range(g32.shape[1]):                    # every latent channel has a non-zero gradient: a missing one cannot hide
        assert g32[:, ch].norm() > 0
        fl, e = rel_l2(gbf[:, ch], g32[:, ch]), rel_l2(got[:, ch], g32[:, ch])
        print(f"    channel {ch}: floor {fl:.2e}, GPU {e:.2e}")
        assert e <= 2.5 * fl + 5e-3, (ch, e, fl)
    # the grad-forward's reconstruction: the decode parity gate, and next to decode() under no_grad
    rfloor = rel_l2(c["rbf"], c["r32"])
    r32, rbf = rel_l2(rec, c["r32"]), rel_l2(rec, c["rbf"])
    with torch.no_grad():
        plain = m.decode(c["z"].to(cuda))
    print(f"    reconstruction: floor {rfloor:.2e}, grad-forward vs fp32 oracle {r32:.2e}, vs bf16 oracle {rbf:.2e}; "
          f"decode() under no_grad vs fp32 oracle {rel_l2(plain, c['r32']):.2e}, grad-forward vs decode() {rel_l2(rec, plain):.2e}")
    assert r32 <= 1.5 * rfloor + 1e-3 and rbf <= 1.5 * rfloor + 1e-3, (r32, rbf, rfloor)
    assert rel_l2(plain, c["r32"]) <= 1.5 * rfloor + 1e-3
    assert all(p.grad is None for p in m.parameters())          # no parameter receives a gradient on this path


@pytest.mark.parametrize("name,dims,b", SHAPES)
def test_fp32_mode_latent_gradients_match_fp32_autograd_at_unit_gain(cuda, name, dims, b):
    c = _case(name, dims, b, 1.0)
    m = _model(c, cuda).set_precision("fp32")
    loss, zl, rec = _forward(m, c, cuda)
    loss.backward()
    torch.cuda.synchronize()
    e, er = rel_l2(zl.grad, c["g32"]), rel_l2(rec, c["r32"])
    print(f"{name} {dims} B{b} fp32 mode, unit gain: latent gradient vs fp32 autograd {e:.2e}, reconstruction {er:.2e} (gates 1e-3)")
    assert e <= 1e-3 and er <= 1e-3, (e, er)
    assert all(p.grad is None for p in m.parameters())


def test_decode_stage_2_outputs_inherits_and_parameters_stay_without_gradients(cuda):
    """Trainable parameters (requires_grad, train mode, a flat gradient buffer attached) see nothing of this backward."""
    from ldm3d import _lib
    c = _case("VAE_TINY", (2, 4, 3), 2, 0.5)
    m = _model(c, cuda).train()
    assert all(p.requires_grad for p in m.parameters())
    total = int(_lib.lib().ldm_model_param_numel_total(m._h))
    m.flat_grads = torch.full((total,), 12345.0, dtype=torch.float32, device=cuda)
    zl = c["z"].to(cuda).requires_grad_(True)
    F.mse_loss(m.decode_stage_2_outputs(zl), c["target"].to(cuda)).backward()
    torch.cuda.synchronize()
    assert rel_l2(zl.grad, c["g32"]) <= 1.5 * rel_l2(c["gbf"], c["g32"]) + 2e-3
    assert all(p.grad is None for p in m.parameters())
    assert bool((m.flat_grads == 12345.0).all())
    assert int(_lib.lib().ldm_model_grad_sync_pending(m._h)) == 0
    # the same call again gives the same bits, and a latent that does not require grad takes the inference plan
    z2 = c["z"].to(cuda).requires_grad_(True)
    F.mse_loss(m.decode(z2), c["target"].to(cuda)).backward()
    assert torch.equal(z2.grad, zl.grad)
    assert not m.decode(c["z"].to(cuda)).requires_grad


def test_backward_of_a_stale_forward_raises(cuda):
    from ldm3d import _lib
    c = _case("VAE_TINY", (2, 4, 3), 2, 0.5)
    m = _model(c, cuda)
    loss1, _, _ = _forward(m, c, cuda)
    loss2, zl2, _ = _forward(m, c, cuda)
    with pytest.raises(_lib.LdmError, match="stale forward"):
        loss1.backward()
    loss2.backward()
    assert torch.isfinite(zl2.grad).all()


def test_encoder_side_still_refuses_and_the_c_entries_check_first(cuda):
    from ldm3d import _lib
    c = _case("VAE_TINY", (2, 4, 3), 2, 0.5)
    m = _model(c, cuda)
    x = torch.zeros((1, 2, 8, 16, 12), device=cuda, requires_grad=True)
    with pytest.raises(NotImplementedError):
        m.encode(x)
    with pytest.raises(NotImplementedError):
        m.encode_stage_2_inputs(x)
    with pytest.raises(NotImplementedError):
        m.train()(x)
    m.eval()
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    m._sync_weights()
    B, d = 1, (2, 2, 2)                                           # a shape no forward has run at
    nbytes = int(L.ldm_vae_decode_grad_workspace_bytes(m._h, B, *d))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    z, dz = torch.zeros((B, 8, *d), device=cuda), torch.full((B, 8, *d), 7.0, device=cuda)
    out = torch.full((B, 2, 8, 8, 8), 7.0, device=cuda)
    assert L.ldm_vae_decode_grad_backward(m._h, out.data_ptr(), dz.data_ptr(), B, *d, ws.data_ptr(), nbytes, s) == -1      # LDM_ERR_BAD_ARG
    assert b"before any ldm_vae_decode_grad_forward" in L.ldm_last_error()
    for args, word in (((m._h, None, out.data_ptr(), B, *d, ws.data_ptr(), nbytes, s), b"null"),
                       ((m._h, z.data_ptr(), out.data_ptr(), 0, *d, ws.data_ptr(), nbytes, s), b"shape"),
                       ((m._h, z.data_ptr(), out.data_ptr(), B, 2, 0, 2, ws.data_ptr(), nbytes, s), b"shape"),
                       ((m._h, z.data_ptr(), out.data_ptr(), B, *d, ws.data_ptr(), nbytes - 1024, s), b"workspace"),
                       ((None, z.data_ptr(), out.data_ptr(), B, *d, ws.data_ptr(), nbytes, s), b"AutoencoderKL")):
        assert L.ldm_vae_decode_grad_forward(*args) != 0
        assert word in L.ldm_last_error().lower() or word in L.ldm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dz == 7.0).all())    # nothing was launched
    assert L.ldm_vae_decode_grad_forward(m._h, z.data_ptr(), out.data_ptr(), B, *d, ws.data_ptr(), nbytes, s) == 0
    assert L.ldm_vae_decode_grad_backward(m._h, out.data_ptr(), dz.data_ptr(), B, *d, ws.data_ptr(), nbytes, s) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(dz).all() and not bool((dz == 7.0).any())
