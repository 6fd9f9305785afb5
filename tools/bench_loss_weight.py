#!/usr/bin/env python3
"""Time of the weighted stage-2 loss (ldm_op_weighted_mse_loss with a Min-SNR table, importance weights and the tracker update: two
launches) against the plain loss it stands in for (ldm_op_mse_loss: two launches), and of the loss-aware timestep draw
(ldm_timestep_resample: one launch), on the training shapes: B = 1 and 4, latents of 4 x 24^3 and 4 x 36 x 44 x 28.

All legs run in this process on the same buffers, alternating: one window of a leg is `--calls` back-to-back calls between two device
events, and every leg gets one window per round after a warm-up.  Reported per shape and leg: the per-call time of every window and their
median / min / max, in microseconds.

    python tools/bench_loss_weight.py [--rounds 7] [--calls 2000] [--warmup 200] [--out profiles/loss_weight_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"4x24x24x24": (4, 24, 24, 24), "4x36x44x28": (4, 36, 44, 28)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2000, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from ldm3d import _lib
    from ldm3d.loss_weighting import LossTracker, min_snr_weights
    from ldm3d.schedulers import DDPMScheduler
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss_weight.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    sch = DDPMScheduler(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0195)
    table = min_snr_weights(sch, 5.0).to(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls_per_window": args.calls, "unit": "us per call", "shapes": {}}
    for name, shape in SHAPES.items():
        for B in (1, 4):
            n = 1
            for s in shape:
                n *= s
            pred, target = torch.randn((B, n), device=dev, generator=gen), torch.randn((B, n), device=dev, generator=gen)
            grad = torch.empty_like(pred)
            ts = torch.randint(0, 1000, (B,), device=dev, generator=gen)
            iw = torch.rand((B,), device=dev, generator=gen) + 0.5
            tracker = LossTracker(1000, n_bins=20, device=dev)
            loss1, loss2 = torch.empty((1,), device=dev), torch.empty((2,), device=dev)
            t_out, iw_out = torch.empty((B,), dtype=torch.int64, device=dev), torch.empty((B,), device=dev)

            def plain():
                assert L.ldm_op_mse_loss(pred.data_ptr(), target.data_ptr(), B * n, loss1.data_ptr(), grad.data_ptr(), stream) == 0

            def weighted():
                assert L.ldm_op_weighted_mse_loss(pred.data_ptr(), target.data_ptr(), B, n, ts.data_ptr(), table.data_ptr(), 1000, iw.data_ptr(),
                                                  tracker.state.data_ptr(), 20, 0.9, loss2.data_ptr(), None, grad.data_ptr(), stream) == 0
            step = [0]

            def resample():
                step[0] += 1
                assert L.ldm_timestep_resample(tracker.state.data_ptr(), 20, 1000, 10, 1e-3, None, B, 42, step[0], None, t_out.data_ptr(),
                                               iw_out.data_ptr(), stream) == 0
            legs = {"mse_loss": plain, "weighted_mse_loss": weighted, "timestep_resample": resample}
            for fn in legs.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in legs}
            for _ in range(args.rounds):
                for leg, fn in legs.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.calls):
                        fn()
                    b.record()
                    b.synchronize()
                    times[leg].append(a.elapsed_time(b) * 1e3 / args.calls)
            assert bool(torch.isfinite(loss1).all()) and bool(torch.isfinite(loss2).all()) and bool(torch.isfinite(iw_out).all())
            rec["shapes"][f"B{B}_{name}"] = {"elements": B * n, "legs": {
                leg: {"us_windows": [round(t, 3) for t in v], "us_median": round(statistics.median(v), 3), "us_min": round(min(v), 3),
                      "us_max": round(max(v), 3)} for leg, v in times.items()}}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
