#!/usr/bin/env python3
"""Cost of a measurement-guided denoising step (DiffusionModelUNet.denoise_step_measured: training forward, residual kernel, data-only
input backward, sampler step, update kernel) on UNET_FULL with a 4-channel condition at 1 x 4 x 24^3, same box, ONE process, the
variants measured alternately in rounds.  A HIP event pair per call; medians of the per-call times after warm-up.

    python tools/bench_guided_step.py [--steps 60] [--warmup 10] [--rounds 3] [--size 24] [--precision bf16]

(a) the guided step against the plain denoise_step (graph mode and eager) and against the full training step's forward + backward;
(b) the data-only input backward against the full backward (ldm_unet_train_backward_input with and without flat_grads);
(c) the thin data gradient of conv_in (conv3_dgrad_thin_kernel alone, ldm_op_conv3d_dgrad_thin_packed on weights packed once outside
    the timed region: 8 real channels over 256 dy channels, bf16 mode) against the same gradient through the general data-gradient
    path as emit_dgrad plans it: ldm_op_conv3d on the flip-transposed weights (ldm_op_weight_flip_transpose, once, outside the timed
    region), 32 stored input channels on a 64-column tile, the planner's own configuration.  The general path writes bf16 NDHWC and
    would still need an unpack into the caller's fp32 (dx | dcond), which is not timed: that only flatters it.  The per-backward
    re-pack of the thin kernel's weights is timed on its own.

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(call, steps, warmup, before=None):
    """Per-call milliseconds of ``steps`` timed calls after ``warmup`` untimed ones; ``before()`` runs untimed in front of every call."""
    import torch
    for _ in range(warmup):
        if before:
            before()
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    torch.cuda.synchronize()
    for a, b in ev:
        if before:
            before()
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=24)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args()
    import torch
    import bench
    import cfgs
    from ldm3d import _lib
    from ldm3d.guidance import ConsistencyGuidance
    from ldm3d.schedulers import DDIMScheduler
    dev = torch.device("cuda:0")
    s, B = args.size, 1
    m = bench.make_unet(dev, in_channels=8)
    mg = bench.make_unet(dev, in_channels=8).enable_graph_replay(True)
    for u in (m, mg):
        u.set_precision(args.precision)
    sch = DDIMScheduler(**cfgs.SCHED)
    sch.set_timesteps(1000)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((B, 4, s, s, s), device=dev, generator=g)
    cond = torch.randn((B, 4, s, s, s), device=dev, generator=g)
    x0 = x.clone()
    tbuf = torch.empty((B,), device=dev)
    smp, smp_g, smp_p = sch.device_sampler(1), sch.device_sampler(1), sch.device_sampler(1)
    meas = ConsistencyGuidance(torch.nn.functional.avg_pool3d(cond, 2), pool=2, scale=0.1)
    state = meas.device_state(x.shape, dev, len(sch.timesteps))
    L = _lib.lib()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    total = int(L.ldm_model_param_numel_total(m._h))
    flat = torch.empty((total,), device=dev)
    gout = torch.randn((B, 4, s, s, s), device=dev, generator=g)
    dx = torch.empty_like(x)
    t = torch.full((B,), 500.0, device=dev)
    out = torch.empty_like(x)
    m._sync_weights()
    ws = m._sized_workspace(("train", B, s, s, s), dev, L.ldm_unet_train_input_workspace_bytes, (B, s, s, s))

    def fwd():
        _lib.check(L.ldm_unet_train_forward(m._h, x0.data_ptr(), 4, cond.data_ptr(), 4, t.data_ptr(), out.data_ptr(), B, s, s, s, ws.data_ptr(),
                                            ws.numel(), stream()))

    def bwd(flat_t, dx_t):
        _lib.check(L.ldm_unet_train_backward_input(m._h, gout.data_ptr(), _lib.ptr(flat_t), _lib.ptr(dx_t), None, B, s, s, s, ws.data_ptr(),
                                                   ws.numel(), stream()))

    def reset(sampler):
        x.copy_(x0)
        sampler.reset(tbuf)

    # (c) the thin dgrad's op entry: 8 real channels, 256 dy channels (UNET_FULL's channels[0])
    c0 = cfgs.UNET_FULL["channels"][0]
    dy = torch.randn((B * s * s * s, c0), device=dev, generator=g).to(torch.bfloat16)
    w = torch.randn((c0, 8, 3, 3, 3), device=dev, generator=g)
    d4, c4 = torch.empty_like(x), torch.empty_like(x)

    wp = torch.empty((27 * 32 * c0,), dtype=torch.bfloat16, device=dev)

    def thin_pack():
        _lib.check(L.ldm_op_conv3d_dgrad_thin_pack(w.data_ptr(), c0, c0, 8, 0, wp.data_ptr(), stream()))

    def thin():
        _lib.check(L.ldm_op_conv3d_dgrad_thin_packed(dy.data_ptr(), c0, wp.data_ptr(), 4, 4, d4.data_ptr(), c4.data_ptr(), B, s, s, s, 0, stream()))

    thin_pack()
    # the general path: the forward arena layout [27][cout_pad = 256][cin_s = 32] of the same weights, flip-transposed once
    warena = torch.zeros((27, c0, 32), dtype=torch.bfloat16, device=dev)
    warena[:, :, :8] = w.reshape(c0, 8, 27).permute(2, 0, 1).to(torch.bfloat16)
    wt = torch.empty((27, 64, c0), dtype=torch.bfloat16, device=dev)
    _lib.check(L.ldm_op_weight_flip_transpose(warena.data_ptr(), wt.data_ptr(), 3, c0, c0, 32, stream()))
    gen_out = torch.empty((B, s, s, s, 32), dtype=torch.bfloat16, device=dev)
    gen_scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=dev)
    zero_bias = torch.zeros((64,), device=dev)

    def general():
        _lib.check(L.ldm_op_conv3d(dy.data_ptr(), c0, None, 0, wt.data_ptr(), zero_bias.data_ptr(), None, 0, None, 0, None, None, None, 0, None,
                                   gen_out.data_ptr(), None, B, s, s, s, 3, 1, 1, 0, 32, 64, 0, 0, gen_scratch.data_ptr(), gen_scratch.numel(), stream()))

    res = {k: [] for k in ("guided_step", "denoise_step_graph", "denoise_step_eager", "train_forward", "backward_full", "backward_full_dx",
                           "backward_data_only", "dgrad_thin_kernel", "dgrad_thin_pack", "dgrad_general_path")}
    with torch.no_grad():
        for _ in range(args.rounds):
            reset(smp)
            res["guided_step"].append(timed(lambda: m.denoise_step_measured(x, tbuf, smp, state, cond=cond), args.steps, args.warmup))
            reset(smp_g)
            res["denoise_step_graph"].append(timed(lambda: mg.denoise_step(x, tbuf, smp_g, cond=cond), args.steps, args.warmup))
            reset(smp_p)
            res["denoise_step_eager"].append(timed(lambda: m.denoise_step(x, tbuf, smp_p, cond=cond), args.steps, args.warmup))
            res["train_forward"].append(timed(fwd, args.steps, args.warmup))
            res["backward_full"].append(timed(lambda: bwd(flat, None), args.steps, args.warmup, before=fwd))
            res["backward_full_dx"].append(timed(lambda: bwd(flat, dx), args.steps, args.warmup, before=fwd))
            res["backward_data_only"].append(timed(lambda: bwd(None, dx), args.steps, args.warmup, before=fwd))
            res["dgrad_thin_kernel"].append(timed(thin, args.steps, args.warmup))
            res["dgrad_thin_pack"].append(timed(thin_pack, args.steps, args.warmup))
            res["dgrad_general_path"].append(timed(general, args.steps, args.warmup))
    # the two paths computed the same gradient (the general one rounds its output to bf16)
    torch.cuda.synchronize()
    ga = torch.cat([d4, c4], dim=1)
    gb = gen_out[..., :8].permute(0, 4, 1, 2, 3).float()
    agree = float((ga - gb).norm() / ga.norm())
    assert agree < 1e-2, agree
    assert torch.isfinite(dx).all()
    chain_finite = bool(torch.isfinite(x).all())            # a random-weight chain may leave [-inf, inf]: reported, the timings do not depend on it
    med = {k: statistics.median(v) for k, v in res.items()}
    print(json.dumps({"size": s, "precision": args.precision, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                      "ms": {k: [round(v, 4) for v in vs] for k, vs in res.items()},
                      "guided_over_denoise_graph": round(med["guided_step"] / med["denoise_step_graph"], 3),
                      "guided_over_denoise_eager": round(med["guided_step"] / med["denoise_step_eager"], 3),
                      "guided_over_train_fwd_bwd": round(med["guided_step"] / (med["train_forward"] + med["backward_full"]), 3),
                      "data_only_over_full_backward": round(med["backward_data_only"] / med["backward_full"], 3),
                      "thin_over_general_dgrad": round(med["dgrad_thin_kernel"] / med["dgrad_general_path"], 3),
                      "thin_vs_general_rel_l2": round(agree, 5), "chain_finite": chain_finite}))


if __name__ == "__main__":
    main()
