#!/usr/bin/env python3
"""Cost of a likelihood step (DiffusionModelUNet.likelihood_step: the UNet forward, the term kernel with the next timestep's noising, the
finalize kernel) against the device sampler's denoising step (DiffusionModelUNet.denoise_step) on the headline model (UNET_FULL at
1 x 4 x 24^3), DDPM timesteps, graph mode, in ONE process, the two chains measured alternately.  A HIP event pair per step; medians.

    python tools/bench_likelihood.py [--steps 100] [--warmup 10] [--rounds 3] [--size 24]

Prints one JSON line: the two medians in ms per round and likelihood / denoise."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def chain_ms(step, reset, steps, warmup):
    """Per-step milliseconds of ``steps`` timed calls after ``warmup`` untimed ones (which also record the graph)."""
    import torch
    reset()
    for _ in range(warmup):
        step()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        step()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=24)
    args = ap.parse_args()
    import torch
    import bench
    import cfgs
    from ldm3d.schedulers import DDPMScheduler, DeviceLikelihood
    dev = torch.device("cuda:0")
    m = bench.make_unet(dev).enable_graph_replay(True)
    sch = DDPMScheduler(**cfgs.SCHED)
    g = torch.Generator(device=dev).manual_seed(0)
    s = args.size
    x0 = torch.clamp(0.6 * torch.randn((1, 4, s, s, s), device=dev, generator=g), -1.0, 1.0)
    x, x_t, tbuf, total = x0.clone(), torch.empty_like(x0), torch.empty((1,), device=dev), torch.zeros((1,), device=dev)
    smp, lik = sch.device_sampler(1), DeviceLikelihood(sch, seed=1)
    res = {"denoise": [], "likelihood": []}
    with torch.no_grad():
        for _ in range(args.rounds):
            res["denoise"].append(statistics.median(chain_ms(lambda: m.denoise_step(x, tbuf, smp), lambda: smp.reset(tbuf), args.steps, args.warmup)))
            res["likelihood"].append(statistics.median(chain_ms(lambda: m.likelihood_step(x0, x_t, tbuf, lik, total),
                                                                lambda: lik.reset(x0, x_t, tbuf, total), args.steps, args.warmup)))
    assert torch.isfinite(total).all() and torch.isfinite(x).all()
    d, l = statistics.median(res["denoise"]), statistics.median(res["likelihood"])
    print(json.dumps({"size": s, "steps": args.steps, "warmup": args.warmup, "ms_denoise_step": [round(v, 4) for v in res["denoise"]],
                      "ms_likelihood_step": [round(v, 4) for v in res["likelihood"]], "likelihood_over_denoise": round(l / d, 4)}))


if __name__ == "__main__":
    main()
