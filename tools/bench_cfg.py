#!/usr/bin/env python3
"""Cost of a classifier-free-guidance step (DiffusionModelUNet.denoise_step(..., guidance=w): one UNet call at batch 2 B with shared
weights, the combine, the scheduler step) against the unguided device step at B = 1 and at B = 2, on the concat-conditioned UNET_FULL
topology (in_channels 8) at 1 x 4 x 24^3, N DDIM steps, graph mode.  A HIP event pair per step; medians over the chain.

    python tools/bench_cfg.py [--steps 50] [--warmup 10] [--size 24] [--cfg 2.0]

Prints one JSON line: the three medians in ms and guided / (2 x unguided B = 1), the cost relative to running the two halves as separate
B = 1 steps."""
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=int, default=24)
    ap.add_argument("--cfg", type=float, default=2.0)
    args = ap.parse_args()
    import torch
    import cfgs
    from ldm3d.networks import DiffusionModelUNet
    from ldm3d.schedulers import DDIMScheduler
    from oracle import unet as ou
    dev = torch.device("cuda:0")
    cfg = dict(cfgs.UNET_FULL, in_channels=8)
    m = DiffusionModelUNet(**cfg)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfg), 0))
    m = m.to(dev).eval().enable_graph_replay(True)
    sch = DDIMScheduler(**cfgs.SCHED)
    sch.set_timesteps(args.steps + args.warmup)
    g = torch.Generator(device=dev).manual_seed(0)
    s = args.size
    res = {}
    with torch.no_grad():
        for name, B, guided in (("guided_b1", 1, True), ("unguided_b1", 1, False), ("unguided_b2", 2, False)):
            x0 = torch.randn((B, 4, s, s, s), device=dev, generator=g)
            cond = torch.randn((B, 4, s, s, s), device=dev, generator=g)
            x, tbuf = x0.clone(), torch.empty((2 * B if guided else B,), device=dev)
            smp = sch.device_sampler(1)
            kw = dict(guidance=args.cfg) if guided else {}
            ms = chain_ms(lambda: m.denoise_step(x, tbuf, smp, cond=cond, **kw), lambda: smp.reset(tbuf), args.steps, args.warmup)
            assert torch.isfinite(x).all()
            res[name] = ms
    med = {k: statistics.median(v) for k, v in res.items()}
    print(json.dumps({"size": s, "steps": args.steps, "warmup": args.warmup, "cfg": args.cfg,
                      "ms_guided_b1": round(med["guided_b1"], 4), "ms_unguided_b1": round(med["unguided_b1"], 4),
                      "ms_unguided_b2": round(med["unguided_b2"], 4),
                      "guided_over_2x_unguided_b1": round(med["guided_b1"] / (2.0 * med["unguided_b1"]), 4),
                      "guided_over_unguided_b2": round(med["guided_b1"] / med["unguided_b2"], 4),
                      "min_ms": {k: round(min(v), 4) for k, v in res.items()}, "max_ms": {k: round(max(v), 4) for k, v in res.items()}}))


if __name__ == "__main__":
    main()
