#!/usr/bin/env python3
"""Cost of an image-space measurement-guided denoising step (DiffusionModelUNet.denoise_step_measured(..., autoencoder=)) on UNET_FULL
with a 4-channel condition at 1 x 4 x 24^3 and VAE_FULL (image 1 x 1 x 96^3), bf16, pool 4: same box, ONE process, the variants measured
alternately in rounds.  A HIP event pair per call; medians of the per-call times after warm-up.

    python tools/bench_image_guided_step.py [--steps 40] [--warmup 10] [--rounds 3] [--size 24] [--pool 4] [--precision bf16]

(a) ms per step of the unguided step (graph mode and eager), the latent-guided step and the image-guided step;
(b) ms of the nine phases of the image-guided step, each through its own entry: UNet training forward, x0 kernel, decoder grad-forward,
    image residual + fold, decoder data-only backward, chain kernel, UNet data-only input backward, sampler step, update kernel;
(c) image_residual_kernel + its fold: bytes moved (y_hat read, g_img written, target read) over time, against the 6.29 TB/s a float4
    copy reaches on this chip.

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_COPY_TBS = 6.29


def make_vae(dev, seed=1):
    """VAE_FULL with bench.make_unet's random init."""
    import torch
    import cfgs
    from ldm3d.networks import AutoencoderKL
    m = AutoencoderKL(**cfgs.VAE_FULL)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5)
            elif name.endswith(".weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    return m.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=24)
    ap.add_argument("--pool", type=int, default=4)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args()
    import torch
    import bench
    import cfgs
    from bench_guided_step import timed
    from ldm3d import _lib
    from ldm3d.guidance import ConsistencyGuidance, ImageConsistencyGuidance
    from ldm3d.schedulers import DDIMScheduler
    dev = torch.device("cuda:0")
    s, B, pool, sf = args.size, 1, args.pool, 1.0
    m = bench.make_unet(dev, in_channels=8)
    mg = bench.make_unet(dev, in_channels=8).enable_graph_replay(True)
    vae = make_vae(dev)
    for u in (m, mg, vae):
        u.set_precision(args.precision)
    f = vae.factor
    si = s * f
    sch = DDIMScheduler(**cfgs.SCHED)
    sch.set_timesteps(1000)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((B, 4, s, s, s), device=dev, generator=g)
    cond = torch.randn((B, 4, s, s, s), device=dev, generator=g)
    low = torch.rand((B, 1, si, si, si), device=dev, generator=g)
    x0 = x.clone()
    tbuf = torch.empty((B,), device=dev)
    smp_i, smp_l, smp_g, smp_p, smp_s = (sch.device_sampler(1) for _ in range(5))
    lat = ConsistencyGuidance(torch.nn.functional.avg_pool3d(cond, 2), pool=2, scale=0.1)
    lat_state = lat.device_state(x.shape, dev, len(sch.timesteps))
    img = ImageConsistencyGuidance(torch.nn.functional.avg_pool3d(low, pool) if pool > 1 else low, pool=pool, scale=0.1)
    state = img.device_state(x.shape, dev, len(sch.timesteps), autoencoder=vae, scale_factor=sf)
    rec, bufs = state
    L = _lib.lib()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    t = torch.full((B,), 500.0, device=dev)
    out = torch.empty_like(x)
    m._sync_weights()
    vae._sync_weights()
    ws = m._sized_workspace(("train", B, s, s, s), dev, L.ldm_unet_train_input_workspace_bytes, (B, s, s, s))
    vws = bufs["vae_workspace"]
    abar = float(sch.alphas_cumprod[500])
    coef = (abar ** 0.5, (1 - abar) ** 0.5, 0, 1.0 / sf)
    n = x.numel()
    tgt = bufs["target"]

    def fwd():
        _lib.check(L.ldm_unet_train_forward(m._h, x0.data_ptr(), 4, cond.data_ptr(), 4, t.data_ptr(), out.data_ptr(), B, s, s, s, ws.data_ptr(),
                                            ws.numel(), stream()))

    def x0k():
        _lib.check(L.ldm_op_guidance_x0(x0.data_ptr(), out.data_ptr(), *coef, bufs["z0"].data_ptr(), n, stream()))

    def dec_fwd():
        _lib.check(L.ldm_vae_decode_grad_forward(vae._h, bufs["z0"].data_ptr(), bufs["recon"].data_ptr(), B, s, s, s, vws.data_ptr(), vws.numel(),
                                                 stream()))

    def residual():
        _lib.check(L.ldm_op_image_residual(bufs["recon"].data_ptr(), tgt.data_ptr(), tgt.shape[0], None, 1, pool, bufs["recon"].data_ptr(),
                                           bufs["norm2"].data_ptr(), bufs["partials"].data_ptr(), bufs["partials"].numel() * 8, B, 1, si, si, si,
                                           stream()))

    def dec_bwd():
        _lib.check(L.ldm_vae_decode_grad_backward(vae._h, bufs["recon"].data_ptr(), bufs["dz"].data_ptr(), B, s, s, s, vws.data_ptr(), vws.numel(),
                                                  stream()))

    def chain():
        _lib.check(L.ldm_op_guidance_chain(bufs["dz"].data_ptr(), *coef, bufs["grad_out"].data_ptr(), bufs["gx"].data_ptr(), n, stream()))

    def unet_bwd():
        _lib.check(L.ldm_unet_train_backward_input(m._h, bufs["grad_out"].data_ptr(), None, bufs["dx"].data_ptr(), None, B, s, s, s, ws.data_ptr(),
                                                   ws.numel(), stream()))

    def update():
        _lib.check(L.ldm_op_guidance_update(x.data_ptr(), bufs["gx"].data_ptr(), bufs["dx"].data_ptr(), bufs["norm2"].data_ptr(), 0.1, 1, B,
                                            n // B, stream()))

    def reset(sampler):
        x.copy_(x0)
        sampler.reset(tbuf)

    phases = ("unet_forward", "x0_kernel", "decoder_forward", "image_residual_and_fold", "decoder_backward", "chain_kernel",
              "unet_backward_data_only", "sampler_step", "update_kernel")
    res = {k: [] for k in ("image_guided_step", "latent_guided_step", "denoise_step_graph", "denoise_step_eager") + phases}
    T = lambda call, before=None: timed(call, args.steps, args.warmup, before)
    with torch.no_grad():
        for _ in range(args.rounds):
            reset(smp_i)
            res["image_guided_step"].append(T(lambda: m.denoise_step_measured(x, tbuf, smp_i, state, cond=cond, autoencoder=vae)))
            reset(smp_l)
            res["latent_guided_step"].append(T(lambda: m.denoise_step_measured(x, tbuf, smp_l, lat_state, cond=cond)))
            reset(smp_g)
            res["denoise_step_graph"].append(T(lambda: mg.denoise_step(x, tbuf, smp_g, cond=cond)))
            reset(smp_p)
            res["denoise_step_eager"].append(T(lambda: m.denoise_step(x, tbuf, smp_p, cond=cond)))
            # the phases, in the step's order, each fed by the one before it
            res["unet_forward"].append(T(fwd))
            res["x0_kernel"].append(T(x0k))
            res["decoder_forward"].append(T(dec_fwd))
            res["image_residual_and_fold"].append(T(residual, before=dec_fwd))
            res["decoder_backward"].append(T(dec_bwd, before=lambda: (dec_fwd(), residual())))
            res["chain_kernel"].append(T(chain))
            res["unet_backward_data_only"].append(T(unet_bwd, before=fwd))
            reset(smp_s)
            res["sampler_step"].append(T(lambda: smp_s.step(out, x, tbuf)))
            res["update_kernel"].append(T(update))
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in res.items()}
    vox = B * si ** 3
    moved = 8 * vox + 4 * tgt.numel()
    chunks = int(L.ldm_image_residual_scratch_bytes(B, 1, si, si, si, pool)) // 8 // B
    tbs = moved / (med["image_residual_and_fold"] * 1e-3) / 1e12
    print(json.dumps({"latent": [B, 4, s, s, s], "image": [B, 1, si, si, si], "pool": pool, "precision": args.precision, "steps": args.steps,
                      "warmup": args.warmup, "rounds": args.rounds, "ms": {k: [round(v, 4) for v in vs] for k, vs in res.items()},
                      "median_ms": {k: round(v, 4) for k, v in med.items()},
                      "phase_sum_ms": round(sum(med[k] for k in phases), 4),
                      "image_over_denoise_graph": round(med["image_guided_step"] / med["denoise_step_graph"], 3),
                      "image_over_denoise_eager": round(med["image_guided_step"] / med["denoise_step_eager"], 3),
                      "image_over_latent_guided": round(med["image_guided_step"] / med["latent_guided_step"], 3),
                      "image_residual": {"chunks_per_sample": chunks, "bytes_moved": moved, "tb_per_s": round(tbs, 4),
                                         "of_hbm_copy_rate": round(tbs / HBM_COPY_TBS, 4)},
                      "chain_finite": bool(torch.isfinite(x).all())}))


if __name__ == "__main__":
    main()
