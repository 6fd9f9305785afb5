"""Stage-wise, teacher-forced parity of the bf16 path (-m gpu).

End to end a bf16 network of this depth can only be gated at its own rounding-noise floor (~3e-2, test_gpu_models.py),
which cannot see a small plumbing error (a dropped bias, one wrong time_emb_proj row, a GroupNorm eps).  Here every block
is fed the fp32 CPU oracle's input (``forward_taps(force=...)``: the library exports each block output, then overwrites
it with the oracle's tensor) and its output is compared with the oracle's output of the same block, so the only noise
in each comparison is that block's own handful of bf16 roundings: gate 5e-3 per block (measured <= 4.2e-3), 1e-2 for
attention blocks (measured <= 6.5e-3).  The fp32 precision mode runs through the same taps at 2e-5 per block (measured ~1e-6).
"""
import pytest
import torch

import cfgs
from util import rel_l2

pytestmark = pytest.mark.gpu
BLOCK_TOL_BF16 = 5e-3
BLOCK_TOL_FP32 = 2e-5


def _unet(cfg, seed, cuda):
    from ldm3d.networks import DiffusionModelUNet
    from oracle import unet as ou
    sd = ou.init_state_dict(ou.unet_param_shapes(cfg), seed)
    m = DiffusionModelUNet(**cfg)
    m.load_state_dict(sd)
    return m.to(cuda).eval(), sd


def _block_taps(taps):
    return {k: v for k, v in taps.items() if "." in k or k == "conv_in"}


def _check_blocks(got, ref, tol, what, attn=()):
    """``attn``: names of attention blocks whose name does not say so (AutoencoderKL).  Attention blocks get twice the tolerance in bf16: GroupNorm, q|k|v, P, O and out_proj are five bf16 storage points in a row
    (the attention kernel alone is gated at 8e-3 in test_gpu_ops.py), a ResBlock has four, a lone conv one."""
    assert set(got) == set(ref), (sorted(set(got) ^ set(ref)))
    worst = {}
    for name in got:
        e = rel_l2(got[name].cpu(), ref[name])
        kind = "attention" if ".attention" in name or name in attn else "other"
        lim = 2 * tol if (kind == "attention" and tol > 1e-3) else tol
        if e > worst.get(kind, ("", 0.0))[1]:
            worst[kind] = (name, e)
        assert torch.isfinite(got[name]).all(), (what, name)
        assert e <= lim, (what, name, e, lim)
    print(f"{what}: {len(got)} blocks, worst " + ", ".join(f"{k}: {v[0]} {v[1]:.2e}" for k, v in worst.items()) + f" (gate {tol:.0e})")


@pytest.mark.parametrize("name,dims,b", [("UNET_TINY", (8, 8, 8), 2), ("UNET_TINY_ALT", (6, 10, 8), 1), ("UNET_FULL", (16, 16, 16), 1),
                                         ("UNET_TINY_HEAD32", (8, 8, 8), 1), ("UNET_TINY_ODD", (8, 8, 8), 2)])
def test_unet_blocks_teacher_forced(cuda, name, dims, b):
    from oracle import unet as ou
    cfg = getattr(cfgs, name)
    m, sd = _unet(cfg, 11, cuda)
    g = torch.Generator().manual_seed(12)
    x = torch.randn((b, cfg["in_channels"], *dims), generator=g)
    t = torch.tensor([37.0, 911.0][:b])
    taps = {}
    ref_out = ou.unet_forward(sd, cfg, x, t, taps=taps)
    ref = _block_taps(taps)
    with torch.no_grad():
        out, got = m.forward_taps(x.to(cuda), t.to(cuda), force=ref)
        _check_blocks(got, ref, BLOCK_TOL_BF16, f"{name} {dims} bf16, teacher forced")
        # the last stage (out.0 GroupNorm + SiLU + out.2 conv) ran on the oracle's last block output
        assert rel_l2(out.cpu(), ref_out) <= BLOCK_TOL_BF16
        m.set_precision("fp32")
        out32, got32 = m.forward_taps(x.to(cuda), t.to(cuda), force=ref)
        _check_blocks(got32, ref, BLOCK_TOL_FP32, f"{name} {dims} fp32, teacher forced")
        assert rel_l2(out32.cpu(), ref_out) <= BLOCK_TOL_FP32


def test_unet_full_24cube_blocks_teacher_forced(cuda):
    """The headline shape: every block of the benchmark UNet at 1x4x24^3 on the oracle's inputs."""
    from oracle import unet as ou
    cfg = cfgs.UNET_FULL
    m, sd = _unet(cfg, 0, cuda)
    x = torch.randn((1, 4, 24, 24, 24), generator=torch.Generator().manual_seed(0))
    t = torch.tensor([500.0])
    taps = {}
    ref_out = ou.unet_forward(sd, cfg, x, t, taps=taps)
    ref = _block_taps(taps)
    with torch.no_grad():
        out, got = m.forward_taps(x.to(cuda), t.to(cuda), force=ref)
    _check_blocks(got, ref, BLOCK_TOL_BF16, "UNET_FULL 24^3 bf16, teacher forced")
    assert rel_l2(out.cpu(), ref_out) <= BLOCK_TOL_BF16
    # the fp32 plans at this shape make their own choices (x3 halo tiles, x3_halo_ok's M range): same taps, fp32 gate
    with torch.no_grad():
        m.set_precision("fp32")
        out32, got32 = m.forward_taps(x.to(cuda), t.to(cuda), force=ref)
    _check_blocks(got32, ref, BLOCK_TOL_FP32, "UNET_FULL 24^3 fp32, teacher forced")
    assert rel_l2(out32.cpu(), ref_out) <= BLOCK_TOL_FP32


def test_export_only_taps_do_not_change_the_result(cuda):
    """Without ``force`` the tapped plan launches the production kernels: same eps_hat bit for bit, and the free-running taps
    track the oracle within the compounding bf16 floor."""
    from oracle import unet as ou
    cfg = cfgs.UNET_TINY
    m, sd = _unet(cfg, 13, cuda)
    x = torch.randn((1, 4, 8, 8, 8), generator=torch.Generator().manual_seed(14))
    t = torch.tensor([250.0])
    taps = {}
    ou.unet_forward(sd, cfg, x, t, taps=taps)
    with torch.no_grad():
        plain = m(x=x.to(cuda), timesteps=t.to(cuda))
        out, got = m.forward_taps(x.to(cuda), t.to(cuda))
    assert torch.equal(plain, out)
    ref = _block_taps(taps)
    assert set(got) == set(ref)
    assert rel_l2(got["conv_in"].cpu(), ref["conv_in"]) <= 3e-3            # one conv: one rounding of inputs, weights, output
    for name in got:
        assert rel_l2(got[name].cpu(), ref[name]) <= 0.1, name


@pytest.mark.parametrize("name,dims", [("VAE_TINY", (16, 16, 16)), ("VAE_FULL", (32, 32, 32)), ("VAE_TINY_ATTN", (16, 16, 16)),
                                       ("VAE_FULL_ATTN", (32, 32, 32))])
def test_vae_blocks_teacher_forced(cuda, name, dims):
    from ldm3d.networks import AutoencoderKL
    from oracle import autoencoder as oa
    from oracle.unet import init_state_dict
    cfg = getattr(cfgs, name)
    sd = init_state_dict(oa.ae_param_shapes(cfg), 15)
    m = AutoencoderKL(**cfg)
    m.load_state_dict(sd)
    m = m.to(cuda).eval()
    x = torch.rand((1, cfg["in_channels"], *dims), generator=torch.Generator().manual_seed(16))
    attn = {f"{pre}.blocks.{k}" for pre, lay in (("encoder", oa.encoder_layout(oa.norm_cfg(cfg))), ("decoder", oa.decoder_layout(oa.norm_cfg(cfg))))
            for k, (kind, _) in enumerate(lay) if kind == "attn"}
    etaps, dtaps = {}, {}
    mu, sigma = oa.encode(sd, cfg, x, taps=etaps)
    rec = oa.decode(sd, cfg, mu, taps=dtaps)
    with torch.no_grad():
        g_mu, g_sigma, got_e = m.encode_taps(x.to(cuda), force=etaps)
        g_rec, got_d = m.decode_taps(mu.to(cuda), force=dtaps)
    _check_blocks(got_e, etaps, BLOCK_TOL_BF16, f"{name} encoder bf16, teacher forced", attn)
    _check_blocks(got_d, dtaps, BLOCK_TOL_BF16, f"{name} decoder bf16, teacher forced", attn)
    assert rel_l2(g_mu.cpu(), mu) <= BLOCK_TOL_BF16 and rel_l2(g_rec.cpu(), rec) <= BLOCK_TOL_BF16
    with torch.no_grad():
        m.set_precision("fp32")
        g_mu, g_sigma, got_e = m.encode_taps(x.to(cuda), force=etaps)
        g_rec, got_d = m.decode_taps(mu.to(cuda), force=dtaps)
    _check_blocks(got_e, etaps, BLOCK_TOL_FP32, f"{name} encoder fp32, teacher forced")
    _check_blocks(got_d, dtaps, BLOCK_TOL_FP32, f"{name} decoder fp32, teacher forced")
    assert rel_l2(g_mu.cpu(), mu) <= BLOCK_TOL_FP32 and rel_l2(g_rec.cpu(), rec) <= BLOCK_TOL_FP32
