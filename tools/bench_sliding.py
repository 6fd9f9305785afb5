#!/usr/bin/env python3
"""Cost of a sliding-window denoising step (DiffusionModelUNet.denoise_step_windows, graph mode) against the UNet forward alone at
the same batch: the difference is what gather-free windowing costs (the blend + scheduler step + window write-back kernel).
Default: the concat-conditioned UNET_FULL topology on the latent of a 132 x 100 x 172 scan (33 x 25 x 43, 24^3 windows: 12).

    python tools/bench_sliding.py --steps 50 --warmup 10 [--latent 33 25 43] [--roi 24] [--chunk 12]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--latent", type=int, nargs=3, default=[33, 25, 43])
    ap.add_argument("--roi", type=int, default=24)
    ap.add_argument("--overlap", type=float, default=0.25)
    ap.add_argument("--chunk", type=int, default=0, help="windows per UNet call (0 = all)")
    args = ap.parse_args()
    import torch
    import cfgs
    from ldm3d.networks import DiffusionModelUNet
    from ldm3d.schedulers import DDPMScheduler
    from ldm3d.sliding import WindowGrid
    from oracle import unet as ou
    dev = torch.device("cuda:0")
    cfg = dict(cfgs.UNET_FULL, in_channels=8)
    m = DiffusionModelUNet(**cfg)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfg), 0))
    m = m.to(dev).eval().enable_graph_replay(True)
    grid = WindowGrid(args.latent, args.roi, overlap=args.overlap)
    nw = grid.n_windows
    chunk = args.chunk or nw
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn([1, 4] + args.latent, device=dev, generator=g)
    cw = grid.gather(torch.randn([1, 4] + args.latent, device=dev, generator=g))
    sch = DDPMScheduler(**cfgs.SCHED)
    smp = sch.device_sampler(1)
    tbuf = torch.empty((chunk,), device=dev)
    smp.reset(tbuf)
    total = args.warmup + args.steps
    assert total <= len(sch.timesteps)
    with torch.no_grad():
        ms_step = timed(lambda: m.denoise_step_windows(x, tbuf, smp, grid, cond_windows=cw, sw_batch_size=chunk), args.steps, args.warmup)
        xw = grid.gather(x)
        tb = torch.full((chunk,), 500.0, device=dev)

        def forwards():
            for b0 in range(0, nw, chunk):
                nb = min(chunk, nw - b0)
                m(x=xw[b0:b0 + nb], timesteps=tb[:nb], cond=cw[b0:b0 + nb])
        ms_unet = timed(forwards, args.steps, args.warmup)
    assert torch.isfinite(x).all()
    print(json.dumps({"latent": args.latent, "roi": args.roi, "windows": nw, "chunk": chunk,
                      "ms_per_windowed_step": round(ms_step, 4), "ms_unet_forward": round(ms_unet, 4),
                      "overhead_ms": round(ms_step - ms_unet, 4), "overhead_pct": round(100.0 * (ms_step / ms_unet - 1.0), 2)}))


if __name__ == "__main__":
    main()
