#!/usr/bin/env python3
"""Two measurements of the ensemble path, device events around whole calls, every alternative warmed up and
then alternated inside one run:

1. LatentDiffusionInferer.sample_ensemble on the concat-conditioned UNET_FULL topology and the VAE_FULL decoder, 24^3 latent -> 96^3
   volume, 20 DDIM steps, K = 8 members, graph mode: ms per member for member_batch 1, 2, 4, 8, against what the library offered before
   it: K batch-1 ``sample`` calls, then ``torch.stack(...).mean / .std`` over the decoded volumes.  ``ratio`` = ensemble / that.
2. ldm_ensemble_update alone at n = 160 x 224 x 160 for B = 1, 4, 8 (count > 0: the state is read and written): achieved bytes/s from
   the algorithm's byte count 4 n (B + 4) over the time between events, a kernel-plus-launch share of the HBM bandwidth bound (8.0 TB/s
   spec; 6.29 TB/s is what a float4 copy reaches).  The calls rotate over enough buffer sets to exceed the 256 MiB Infinity Cache.

    python tools/bench_ensemble.py [--rounds 6] [--members 8] [--steps 20] [--size 24] [--out profiles/ensemble_bench.json]

Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8.0e12
HBM_COPY = 6.29e12


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def bench_sampling(args, dev):
    import torch
    import cfgs
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.networks import AutoencoderKL, DiffusionModelUNet
    from ldm3d.schedulers import DDIMScheduler
    from oracle import autoencoder as oa
    from oracle import unet as ou
    ucfg = dict(cfgs.UNET_FULL, in_channels=8)
    m = DiffusionModelUNet(**ucfg)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(ucfg), 0))
    m = m.to(dev).eval().enable_graph_replay(True)
    v = AutoencoderKL(**cfgs.VAE_FULL)
    v.load_state_dict(ou.init_state_dict(oa.ae_param_shapes(cfgs.VAE_FULL), 2))
    v = v.to(dev).eval()
    sch = DDIMScheduler(**cfgs.SCHED)
    sch.set_timesteps(args.steps)
    inf = LatentDiffusionInferer(sch)
    K, s = args.members, args.size
    latent = (4, s, s, s)
    cond = torch.randn((1,) + latent, generator=torch.Generator().manual_seed(1)).to(dev)

    def parent_way():
        vols = []
        for k in range(K):
            z = torch.randn(latent, generator=torch.Generator().manual_seed(k))[None].to(dev)
            vols.append(inf.sample(z, v, m, conditioning=cond, mode="concat", fused_seed=k))
        stack = torch.stack(vols)
        return stack.mean(dim=0), stack.std(dim=0)

    batches = [b for b in (1, 2, 4, 8) if b <= K]
    alts = {"parent_stack": parent_way}
    for b in batches:
        alts[f"ensemble_b{b}"] = (lambda b=b: inf.sample_ensemble(K, latent, v, m, conditioning=cond, member_batch=b, seed=0))
    ms = {name: [] for name in alts}
    with torch.no_grad():
        for name, fn in alts.items():                                     # warm-up: plans, graphs and workspaces of every batch size
            fn()
        for _ in range(args.rounds):
            for name, fn in alts.items():
                t, _ = timed(fn)
                ms[name].append(t)
        ref_mean, _ = parent_way()
        res = inf.sample_ensemble(K, latent, v, m, conditioning=cond, member_batch=1, seed=0)
        diff = float((res.mean[0] - ref_mean[0]).abs().max())            # the same members (batch 1, same seeds): rounding only
    med = {k: statistics.median(t) for k, t in ms.items()}
    return {"members": K, "steps": args.steps, "latent": list(latent), "rounds": args.rounds,
            "seconds_timed": {k: round(sum(t) / 1e3, 3) for k, t in ms.items()},
            "ms_per_member": {k: round(t / K, 4) for k, t in med.items()},
            "min_ms_per_member": {k: round(min(t) / K, 4) for k, t in ms.items()},
            "max_ms_per_member": {k: round(max(t) / K, 4) for k, t in ms.items()},
            "ratio_vs_parent": {k: round(med[k] / med["parent_stack"], 4) for k in med if k != "parent_stack"},
            "max_abs_diff_mean_b1_vs_parent": diff}


def bench_update(dev):
    import torch
    from ldm3d import _lib
    L = _lib.lib()
    n = 160 * 224 * 160
    out = {"n": n, "hbm_peak_bytes_per_s": HBM_PEAK, "hbm_copy_bytes_per_s": HBM_COPY, "cases": {}}
    st = _lib.current_stream()
    for B in (1, 4, 8):
        nbytes = 4 * n * (B + 4)
        sets = max(2, -(-(1200 << 20) // (4 * n * (B + 2))))              # footprint of all sets > 1.2 GB
        bufs = [(torch.rand((B, n), device=dev), torch.zeros((n,), device=dev), torch.zeros((n,), device=dev)) for _ in range(sets)]

        def run(iters):
            for i in range(iters):
                x, mean, m2 = bufs[i % sets]
                _lib.check(L.ldm_ensemble_update(x.data_ptr(), B, n, n, mean.data_ptr(), m2.data_ptr(), 1, st))

        run(2 * sets)
        t, _ = timed(lambda: run(50))
        iters = max(100, int(2500.0 / (t / 50)))                          # >= 2.5 s of work
        t, _ = timed(lambda: run(iters))
        per = t / 1e3 / iters
        out["cases"][f"B{B}"] = {"iters": iters, "sets": sets, "seconds_timed": round(t / 1e3, 3), "us_per_call": round(per * 1e6, 2),
                                 "bytes_per_call": nbytes, "bytes_per_s": round(nbytes / per, 1),
                                 "share_of_hbm_peak": round(nbytes / per / HBM_PEAK, 4), "share_of_float4_copy": round(nbytes / per / HBM_COPY, 4)}
        del bufs
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--size", type=int, default=24)
    ap.add_argument("--skip-sampling", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    res = {"update": bench_update(dev)}
    if not args.skip_sampling:
        res["sampling"] = bench_sampling(args, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
