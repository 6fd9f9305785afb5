#!/usr/bin/env python3
"""Time of `ldm3d.metrics.image_metrics` (one launch of ldm_op_image_metrics + its finalize) against the same quantities computed with
torch-ROCm on the GPU: five dense win^3 `F.conv3d` calls for the windowed moments plus the element-wise passes and reductions behind
SSIM, MSE, MAE, PSNR and NRMSE (what a user without this kernel would write).  Both legs run in this process, alternating, on the same
tensors; every launch is timed with HIP events and the median is reported.  The torch leg's result is compared with the kernel's, so
the two legs are known to compute the same thing.

    python tools/bench_metrics.py [--reps 30] [--warmup 5] [--out profiles/metrics_bench.json]

Bytes: the floor is one read of both volumes, 2 * N * 4.  A workgroup loads a (16 + win - 1) x (32 + win - 1) tile per 16 x 32 tile of
the map and win - 1 extra planes per run of output planes, so it requests `halo_factor` times the floor (neighbouring tiles re-read each
other's halo, mostly from L2); both rates are printed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TH, TW = 16, 32                                                    # csrc/metrics.h MT_TH, MT_TW


def plan(shape, win):
    """metrics_plan of csrc/ldm3d.hip for B = C = 1: (runs along D, output planes per run, requested / floor bytes)."""
    D, H, W = shape
    Do, Ho, Wo = D - win + 1, H - win + 1, W - win + 1
    th, tw = -(-Ho // TH), -(-Wo // TW)
    want = max(1, min(-(-512 // (th * tw)), -(-Do // 8)))
    planes = -(-Do // want)
    runs = -(-Do // planes)
    loaded = 0
    for r in range(runs):
        nin = min(planes, Do - r * planes) + win - 1
        for i in range(th):
            for j in range(tw):
                loaded += nin * min(TH + win - 1, H - i * TH) * min(TW + win - 1, W - j * TW)
    loaded += th * tw * runs * min(TH + win - 1, H) * min(TW + win - 1, W)       # the pivot pass re-reads each run's first plane
    return runs, planes, loaded / (D * H * W)


def torch_metrics(x, y, w3, data_range, k1=0.01, k2=0.03):
    import torch
    import torch.nn.functional as F
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    mx, my = F.conv3d(x, w3), F.conv3d(y, w3)
    exx, eyy, exy = F.conv3d(x * x, w3), F.conv3d(y * y, w3), F.conv3d(x * y, w3)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    ssim = (((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))).mean()
    d = x - y
    mse = (d * d).mean()
    return torch.stack([ssim, 20 * torch.log10(torch.tensor(data_range, device=x.device)) - 10 * torch.log10(mse), mse, d.abs().mean(),
                        torch.sqrt((d * d).sum() / (y * y).sum())])


def time_alternating(legs, reps, warmup):
    import torch
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--win", type=int, default=11)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from ldm3d.metrics import image_metrics, window_weights
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    w1 = torch.tensor(window_weights("gaussian", args.win, 1.5), dtype=torch.float32, device=dev)
    w3 = (w1[:, None, None] * w1[None, :, None] * w1[None, None, :])[None, None]
    results = []
    for shape in ((96, 96, 96), (160, 224, 160)):
        g = torch.Generator(device=dev).manual_seed(0)
        y = torch.rand((1, 1) + shape, device=dev, generator=g)
        x = (y + 0.05 * torch.randn((1, 1) + shape, device=dev, generator=g)).contiguous()
        names = ("ssim", "psnr", "mse", "mae", "nrmse")
        kern = lambda: image_metrics(x, y, data_range=1.0, win_size=args.win)
        ref = lambda: torch_metrics(x, y, w3, 1.0)
        mine = torch.stack([kern()[k][0] for k in names]).cpu()
        theirs = ref().cpu()
        diff = (mine - theirs).abs() / theirs.abs()
        t = time_alternating({"kernel": kern, "torch": ref}, args.reps, args.warmup)
        med = {k: statistics.median(v) for k, v in t.items()}
        n = shape[0] * shape[1] * shape[2]
        runs, planes, halo = plan(shape, args.win)
        rec = {"shape": list(shape), "win": args.win, "reps": args.reps,
               "image_metrics_ms_median": med["kernel"], "image_metrics_ms_min": min(t["kernel"]), "image_metrics_ms_max": max(t["kernel"]),
               "torch_conv3d_ms_median": med["torch"], "torch_conv3d_ms_min": min(t["torch"]), "torch_conv3d_ms_max": max(t["torch"]),
               "speedup_median": med["torch"] / med["kernel"],
               "floor_bytes": 2 * n * 4, "floor_GBps": 2 * n * 4 / (med["kernel"] * 1e-3) / 1e9,
               "halo_factor": halo, "requested_GBps": halo * 2 * n * 4 / (med["kernel"] * 1e-3) / 1e9,
               "runs_along_d": runs, "planes_per_run": planes,
               "max_rel_diff_kernel_vs_torch": float(diff.max()), "kernel": dict(zip(names, mine.tolist())), "torch": dict(zip(names, theirs.tolist()))}
        print(json.dumps(rec))
        results.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "note": "image_metrics time includes its host wrapper (three small allocations) "
                       "and both of its kernels; the torch leg is five dense conv3d + element-wise passes", "results": results}, fh, indent=1)


if __name__ == "__main__":
    main()
