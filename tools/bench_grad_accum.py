#!/usr/bin/env python3
"""What gradient accumulation costs (beside bench.py, never instead of it):

    python tools/bench_grad_accum.py [--k 4] [--steps 40] [--warmup 8] [--rounds 2] [--parent DIR]

Three things, on the 24^3 training step of the benchmark UNet (UNET_FULL, B = 1, bf16; forward + MSE + backward + clip + fused Adam):
  1. the time of one call with accumulation off and with K micro-batches per optimizer step (HIP events around every call, median after
     warm-up; at K the calls that close a window and the others separately, and the whole window).  --parent DIR names a built checkout of
     the PARENT commit: the same un-accumulated step is timed there too, in processes of its own that alternate with this tree's, because
     the yardstick of the step time is the parent on the same box, never this code;
  2. the accumulate launches of one backward from the library's own launch timeline (ldm_profile_start(LDM_PROFILE_GRAD_ACCUM)), in
     assign and in add mode, and the kernel as one launch over the whole buffer;
  3. hipMemcpyDtoDAsync of the same bytes on the same box: a copy whose read + write traffic equals the pass's (8 bytes per parameter in
     assign mode, 12 in add mode), as one call and cut at the plan's bucket boundaries.
Every process prints one JSON line; the driver prints the merged record last."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (24, 24, 24)


def _median(v):
    return statistics.median(v) if v else None


def child(args):
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import torch
    import torch.nn.functional as F
    import cfgs
    from ldm3d import _lib
    from ldm3d.networks import DiffusionModelUNet
    from ldm3d.optim import FlatAdam

    assert os.path.abspath(_lib.LIB_PATH).startswith(root), (_lib.LIB_PATH, root)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = _lib.lib()
    new_code = hasattr(L, "ldm_model_set_grad_accum") and "ldm_model_set_grad_accum" in _lib.SIGNATURES
    m = DiffusionModelUNet(**cfgs.UNET_FULL)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for _, p in m.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 / p[0].numel() ** 0.5))
    m = m.to(dev).train()
    gen = torch.Generator(device=dev).manual_seed(1)
    xs = [torch.randn((1, 4, *DIMS), device=dev, generator=gen) for _ in range(4)]
    noise = torch.randn((1, 4, *DIMS), device=dev, generator=gen)
    t = torch.randint(0, 1000, (1,), device=dev, generator=gen).float()
    out = {"root": root, "new_code": new_code, "device": torch.cuda.get_device_name(0), "params": None}

    def timed_calls(opt, n_calls, warmup):
        """HIP events around every call: forward, loss, [arm,] backward, [the optimizer step on a call that closes a window]."""
        ms, closing = [], []
        for i in range(warmup + n_calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            loss = F.mse_loss(m(x=xs[i % 4], timesteps=t).float(), noise)
            if new_code:
                opt.arm()
            loss.backward()
            done = opt.micro_done() if new_code else True
            if done:
                opt.step()
            b.record()
            b.synchronize()
            if i >= warmup:
                ms.append(a.elapsed_time(b))
                closing.append(done)
        assert bool(torch.isfinite(loss))
        return ms, closing

    K = args.k
    warm = (args.warmup + K - 1) // K * K                       # whole windows, so the timed calls start at a window's first
    calls = (args.steps + K - 1) // K * K
    opt = FlatAdam(m, lr=5e-6, max_grad_norm=1.0)
    out["params"] = int(m.flat_params.numel())
    ms, _ = timed_calls(opt, calls, warm)
    out["off"] = {"calls": len(ms), "median_ms": _median(ms), "min_ms": min(ms), "max_ms": max(ms)}
    if not new_code:
        print(json.dumps(out), flush=True)
        return

    optk = FlatAdam(m, lr=5e-6, max_grad_norm=1.0, grad_accum_steps=K)
    ms, closing = timed_calls(optk, calls, warm)
    inner = [v for v, c in zip(ms, closing) if not c]
    last = [v for v, c in zip(ms, closing) if c]
    windows = [sum(ms[i:i + K]) for i in range(0, len(ms), K)]
    out["k"] = {"K": K, "calls": len(ms), "median_ms_inner_call": _median(inner), "median_ms_closing_call": _median(last),
                "median_ms_window": _median(windows), "median_ms_per_micro_step": _median(windows) / K, "min_ms_window": min(windows)}

    # 2. the accumulate launches of ONE backward, from the library's launch timeline
    n = out["params"]
    acc = optk.grad_accum
    st = torch.cuda.current_stream().cuda_stream

    def backward_timeline(micro):
        loss = F.mse_loss(m(x=xs[0], timesteps=t).float(), noise)
        m.set_grad_accum(acc, micro, K)
        _lib.check(L.ldm_profile_start(-1, 0, 0, 4096))       # -1 = LDM_PROFILE_GRAD_ACCUM (include/ldm3d.h)
        loss.backward()
        torch.cuda.synchronize()
        fl, tms = (C.c_double * 4096)(), (C.c_double * 4096)()
        cnt = L.ldm_profile_detail(fl, tms, 4096)
        stats = (C.c_double * 5)()
        _lib.check(L.ldm_profile_stop(stats))
        m.set_grad_accum(None)
        return {"launches": cnt, "total_ms": sum(tms[k] for k in range(cnt)), "bytes": sum(fl[k] for k in range(cnt)),
                "launch_ms": [round(tms[k], 5) for k in range(cnt)]}

    timeline = {}
    for mode, micro in (("assign", 0), ("add", 1)):
        backward_timeline(micro)                                     # warm
        runs = [backward_timeline(micro) for _ in range(args.timeline_reps)]
        best = min(runs, key=lambda r: r["total_ms"])
        timeline[mode] = {"launches": best["launches"], "bytes": best["bytes"], "median_total_ms": _median([r["total_ms"] for r in runs]),
                          "min_total_ms": best["total_ms"], "launch_ms_of_min": best["launch_ms"]}
    out["timeline"] = timeline

    # the kernel as ONE launch over the whole buffer (no bucket boundaries)
    def timed(fn, reps=20):
        for _ in range(3):
            fn()
        v = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            v.append(a.elapsed_time(b))
        return {"median_ms": _median(v), "min_ms": min(v)}
    gbuf = m.flat_grads
    gbuf.normal_()
    out["one_launch"] = {mode: timed(lambda: _lib.check(L.ldm_op_grad_accumulate(acc.data_ptr(), gbuf.data_ptr(), n, 0.25, assign, st)))
                         for mode, assign in (("assign", 1), ("add", 0))}

    # 3. hipMemcpyDtoDAsync of the same bytes: payload = half the pass's traffic (a copy reads and writes every byte once)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoDAsync.restype = C.c_int
    hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    src = torch.empty(n * 6 // 4 + 16, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)

    def copy(nbytes, off=0):
        rc = hip.hipMemcpyDtoDAsync(dst.data_ptr() + off, src.data_ptr() + off, nbytes, st)
        assert rc == 0, rc
    sched = (C.c_int * 4096)(), (C.c_int64 * 4096)(), (C.c_int64 * 4096)(), (C.c_int * 4096)()
    cnt = L.ldm_model_grad_schedule(m._h, 1, *DIMS, *sched, 4096)
    buckets = [int(sched[2][k]) for k in range(min(cnt, 4096)) if sched[0][k] == 1]
    assert sum(buckets) == n
    out["buckets"] = {"count": len(buckets), "largest_mb": max(buckets) * 4 / 2 ** 20, "smallest_mb": min(buckets) * 4 / 2 ** 20}
    memcpy = {}
    for mode, per in (("assign", 4), ("add", 6)):                   # payload bytes per parameter
        memcpy[f"{mode}_one_call"] = dict(timed(lambda: copy(n * per)), traffic_bytes=2 * n * per)

        def chunks():
            off = 0
            for b in buckets:
                copy(b * per, off)
                off += b * per
        memcpy[f"{mode}_per_bucket"] = dict(timed(chunks), traffic_bytes=2 * n * per)
    out["memcpy_dtod"] = memcpy
    print(json.dumps(out), flush=True)


def driver(args):
    roots = [("this", HERE)] + ([("parent", os.path.abspath(args.parent))] if args.parent else [])
    runs = {name: [] for name, _ in roots}
    for r in range(args.rounds):                                    # alternate the two trees, one process each
        for name, root in (roots if r % 2 == 0 else roots[::-1]):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--k", str(args.k), "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--timeline-reps", str(args.timeline_reps)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"bench child for the {name} tree failed with status {p.returncode}")
            rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            print(json.dumps({"tree": name, "round": r, **rec}), flush=True)
            runs[name].append(rec)
    this = runs["this"]
    summary = {"metric": "24^3 UNet training call, ms (median of per-process medians)", "K": args.k,
               "off_ms": _median([x["off"]["median_ms"] for x in this]),
               "k_per_micro_step_ms": _median([x["k"]["median_ms_per_micro_step"] for x in this]),
               "k_window_ms": _median([x["k"]["median_ms_window"] for x in this]),
               "k_inner_call_ms": _median([x["k"]["median_ms_inner_call"] for x in this]),
               "k_closing_call_ms": _median([x["k"]["median_ms_closing_call"] for x in this]),
               "parent_off_ms": _median([x["off"]["median_ms"] for x in runs.get("parent", [])]),
               "per_process_off_ms": {name: [x["off"]["median_ms"] for x in v] for name, v in runs.items()}}
    print(json.dumps(summary), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40, help="timed calls per configuration (rounded up to whole windows; at least 20)")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2, help="processes per tree, alternating")
    ap.add_argument("--timeline-reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its own libldm3d.so): the step-time yardstick")
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 20 or args.k < 2:
        ap.error("--steps must be at least 20 and --k at least 2")
    child(args) if args.child else driver(args)


if __name__ == "__main__":
    main()
