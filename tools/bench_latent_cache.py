#!/usr/bin/env python3
"""What the latent cache saves per stage-2 step at the reference's own training shape (config_train_16g.json: AutoencoderKL with 2 image
and 8 latent channels, patch 144x176x112 -> latent 8x36x44x28, concat-conditioned UNet 16 -> 8, batch 1, one GPU):

    python tools/bench_latent_cache.py [--steps 30] [--warmup 3] [--samples 2] [--out profiles/latent_cache_bench.json]

``DiffusionTrainer.train_step`` (two autoencoder encodes per step) and ``train_step_cached`` (one ldm_latent_batch launch) run in ONE
process, alternating step by step on the same trainer, each step between a HIP event pair; median / min / max per path.  Beside them:
the ldm_latent_batch launch alone, the cache build time per sample, and bench.py's own phase trace of the uncached step on the same
box, so that the saving can be held against the two encode phases it replaces.  Writes one JSON file and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="timed steps per path (at least 30)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=2, help="synthetic pairs in the cache")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent_cache_bench.json"))
    args = ap.parse_args()
    steps = max(args.steps, 30)

    import torch
    import bench
    import cfgs
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.latents import LatentCache
    from ldm3d.networks import AutoencoderKL, DiffusionModelUNet
    from ldm3d.schedulers import DDPMScheduler
    from ldm3d.trainer import DiffusionTrainer

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ref = cfgs.REF_CONFIGS["config_train_16g"]
    patch, lc = tuple(ref["unet_patch"]), ref["ae"]["latent_channels"]
    torch.manual_seed(100)
    vae = AutoencoderKL(**ref["ae"])
    unet = DiffusionModelUNet(**dict(ref["unet"], in_channels=2 * lc))       # mode="concat": noisy label latent | image latent
    with torch.no_grad():
        for mod, gain in ((vae, 1.0), (unet, 0.5)):
            for _, p in mod.named_parameters():
                if p.dim() > 1:
                    p.copy_(torch.randn(p.shape) * (gain / p[0].numel() ** 0.5))
    vae, unet = vae.to(dev).eval(), unet.to(dev)
    tr = DiffusionTrainer(unet, vae, LatentDiffusionInferer(DDPMScheduler(**cfgs.SCHED), scale_factor=0.7311), lr=1e-5)
    if not tr.overlap:                                                       # the in-library exchange on a world-size-1 communicator, as bench.py
        tr.overlap = tr.sync.attach(unet, force_single=True)

    class Pairs:                                                             # what LatentCache.build reads off a PairVolumes
        randcrop, scale_on_host = False, True

        def __init__(self, n):
            g = torch.Generator().manual_seed(7)
            self.items = [{k: torch.rand((ref["ae"]["in_channels"],) + patch, generator=g) for k in ("image", "label")} for _ in range(n)]

        def __len__(self):
            return len(self.items)

        def __getitem__(self, i):
            return self.items[i]
    pairs = Pairs(args.samples)
    LatentCache.build(vae, pairs, dev)                                       # once for the encoder's plan and workspace, then timed
    cache = LatentCache.build(vae, pairs, dev)
    images, labels = pairs[0]["image"][None].to(dev), pairs[0]["label"][None].to(dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b
    for _ in range(args.warmup):
        tr.train_step(images, labels)
        tr.train_step_cached(cache, [0])
    torch.cuda.synchronize()
    ev = {"uncached": [], "cached": []}
    for k in range(steps):
        ev["uncached"].append(timed(lambda: tr.train_step(images, labels)))
        ev["cached"].append(timed(lambda: tr.train_step_cached(cache, [k % len(cache)])))
    torch.cuda.synchronize()
    ms = {name: [a.elapsed_time(b) for a, b in pairs_] for name, pairs_ in ev.items()}
    sch = tr.inferer.scheduler
    t = torch.randint(0, sch.num_train_timesteps, (1,), device=dev)
    for _ in range(args.warmup):
        cache.batch([0], sch, t, 0.7311, seed=1, step=0)
    launch = [timed(lambda: cache.batch([k % len(cache)], sch, t, 0.7311, seed=1, step=k)) for k in range(steps)]
    torch.cuda.synchronize()
    phases = bench.ddp_phase_trace(tr, images, labels, dev)
    u, c = stats(ms["uncached"]), stats(ms["cached"])
    rec = {"what": "stage-2 train step at config_train_16g (patch 144x176x112, latent 8x36x44x28, UNet 16 -> 8, batch 1, world 1): "
                   "train_step (two autoencoder encodes) vs train_step_cached (one ldm_latent_batch launch), alternating in one process, "
                   "a HIP event pair per step",
           "device": torch.cuda.get_device_name(dev), "steps_per_path": steps, "warmup_per_path": args.warmup,
           "train_step_ms": u, "train_step_cached_ms": c, "saved_ms_median": round(u["median"] - c["median"], 4),
           "speedup_median": round(u["median"] / c["median"], 4),
           "ldm_latent_batch_ms": stats([a.elapsed_time(b) for a, b in launch]),
           "ldm_latent_batch_note": "LatentCache.batch: the table gathers, three torch.empty and the launch, device draws",
           "cache": {"samples": len(cache), "bytes": cache.nbytes, "build_s_per_sample": round(cache.build_seconds / len(cache), 4)},
           "uncached_phase_trace_ms": phases,
           "encode_phases_ms": round(phases["vae_encode_condition"] + phases["vae_encode_labels"], 3)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
