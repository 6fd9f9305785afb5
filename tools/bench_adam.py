#!/usr/bin/env python3
"""Time of the optimizer tail on the benchmark UNet (tests/cfgs.py UNET_FULL, 191 M parameters): the fused Adam + bf16 re-pack launch
(ldm_model_adam_step), its EMA form (ldm_model_adam_step_ema) and the same launch followed by a stand-alone EMA pass over the flat buffers
(`torch.Tensor.lerp_`: what an EMA kept outside the kernel costs on the device, leaving aside that it cannot see the device-side skip).
With --baseline-lib a second build of the library (e.g. the parent commit's) is loaded into the same process and its ldm_model_adam_step is
timed as two separate legs, so that the same code's own leg-to-leg spread is the yardstick for "EMA off costs nothing".

All legs run in this process on the same p / g / m / v buffers, alternating: one window of a leg is `--launches` back-to-back launches
between two device events (default 900: above a second at ~1.2 ms per launch), and every leg gets one window per round.  Reported per leg: the
per-launch time of every window, their median / min / max, and the achieved bytes/s for the bytes the form has to move (p, m, v read and
written, g read, the bf16 arena written = 30 bytes per parameter; + 8 for the EMA read and written; the stand-alone pass reads p again: + 12).

    python tools/bench_adam.py [--rounds 5] [--launches 900] [--warmup 20] [--baseline-lib PATH] [--out profiles/ema_adam.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HYPER = (1e-6, 0.9, 0.999, 1e-8, 0.0)                       # lr small enough that thousands of launches on one gradient stay finite


def open_lib(path):
    """A build of the library with the handful of entries this benchmark calls (a baseline build need not have the EMA ones)."""
    from ldm3d import _lib
    h = C.CDLL(path)
    for name in ("ldm_last_error", "ldm_unet_create", "ldm_model_destroy", "ldm_model_param_numel_total", "ldm_model_load_params_flat",
                 "ldm_grad_sq_norm", "ldm_model_adam_step", "ldm_model_adam_step_ema"):
        fn = getattr(h, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return h


def unet_handle(lib, cfg):
    from ldm3d import _lib
    c = _lib.UNetCfg()
    n = len(cfg["channels"])
    c.spatial_dims, c.in_channels, c.out_channels, c.num_levels = cfg["spatial_dims"], cfg["in_channels"], cfg["out_channels"], n
    for i in range(n):
        c.channels[i], c.attention_levels[i] = int(cfg["channels"][i]), int(bool(cfg["attention_levels"][i]))
        nhc, nrb = cfg["num_head_channels"], cfg["num_res_blocks"]
        c.num_head_channels[i] = int(nhc if isinstance(nhc, int) else nhc[i])
        c.num_res_blocks[i] = int(nrb if isinstance(nrb, int) else nrb[i])
    c.norm_num_groups, c.norm_eps = int(cfg.get("norm_num_groups", 32)), float(cfg.get("norm_eps", 1e-6))
    h = C.c_void_p()
    if lib.ldm_unet_create(C.byref(c), C.byref(h)) != 0:
        raise SystemExit(f"ldm_unet_create: {lib.ldm_last_error()}")
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=900, help="launches per timed window (a window should last a second or more)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--baseline-lib", default=None, help="another build of libldm3d.so whose ldm_model_adam_step is timed in the same process")
    ap.add_argument("--config", default="UNET_FULL", help="name of a UNet definition in tests/cfgs.py")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import cfgs
    from ldm3d import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    cfg = getattr(cfgs, args.config)
    libs = {"this": open_lib(_lib.LIB_PATH)}
    if args.baseline_lib:
        libs["baseline"] = open_lib(os.path.abspath(args.baseline_lib))
    stream = torch.cuda.current_stream().cuda_stream
    h0 = unet_handle(libs["this"], cfg)
    n = int(libs["this"].ldm_model_param_numel_total(h0))
    gen = torch.Generator(device=dev).manual_seed(0)
    p = 0.05 * torch.randn((n,), device=dev, generator=gen)
    g = 0.01 * torch.randn((n,), device=dev, generator=gen)
    m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    sq = torch.zeros((2,), device=dev)
    assert libs["this"].ldm_grad_sq_norm(g.data_ptr(), n, sq.data_ptr(), stream) == 0

    def handle(lib):
        h = unet_handle(lib, cfg)
        if lib.ldm_model_load_params_flat(h, p.data_ptr(), stream) != 0:          # allocates and fills this handle's arena
            raise SystemExit(f"ldm_model_load_params_flat: {lib.ldm_last_error()}")
        return h
    step = [0]

    def adam(lib, h):
        def fn():
            step[0] += 1
            rc = lib.ldm_model_adam_step(h, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), *HYPER, step[0], sq.data_ptr(), 1.0, stream)
            assert rc == 0, lib.ldm_last_error()
        return fn

    def adam_ema(lib, h):
        def fn():
            step[0] += 1
            rc = lib.ldm_model_adam_step_ema(h, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ema.data_ptr(), *HYPER, step[0],
                                             0.999, 1, sq.data_ptr(), 1.0, stream)
            assert rc == 0, lib.ldm_last_error()
        return fn

    def then_lerp(fn):
        def both():
            fn()
            ema.lerp_(p, 1e-3)
        return both
    this, hs = libs["this"], [h0]
    libs["this"].ldm_model_load_params_flat(h0, p.data_ptr(), stream)
    legs = {"adam": (adam(this, h0), 30), "adam_ema": (adam_ema(this, h0), 38), "adam_then_lerp": (then_lerp(adam(this, h0)), 42)}
    if "baseline" in libs:
        base = libs["baseline"]
        for tag in ("baseline_adam_1", "baseline_adam_2"):
            hs.append(handle(base))
            legs[tag] = (adam(base, hs[-1]), 30)
        legs["baseline_adam_then_lerp"] = (then_lerp(adam(base, hs[-1])), 42)
    for fn, _ in legs.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, (fn, _) in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / args.launches)
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(ema).all()) and float(sq[1]) == 0.0
    rec = {"device": torch.cuda.get_device_name(0), "config": args.config, "params": n, "rounds": args.rounds, "launches_per_window": args.launches,
           "legs": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        nbytes = legs[name][1] * n
        rec["legs"][name] = {"ms_per_launch_windows": [round(t, 5) for t in ts], "ms_median": med, "ms_min": min(ts), "ms_max": max(ts),
                             "bytes": nbytes, "TBps_at_median": nbytes / (med * 1e-3) / 1e12}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    for lib, h in zip([this] + [libs.get("baseline")] * (len(hs) - 1), hs):
        lib.ldm_model_destroy(h)


if __name__ == "__main__":
    main()
