#!/usr/bin/env python3
"""train_diffusion.py - same command line, JSON schema, checkpoint names and per-step order as the reference's
3d_ldm/train_diffusion.py (:24-38 flags, :58-64 config merge, :90-124 autoencoder + scale factor, :127-156 UNet /
scheduler / inferer / Adam / MultiStepLR, :166-305 epoch loop with validation and rank-0 checkpoints), on the
MI355X-native path.

    python train_diffusion.py -e config/environment.json -c config/config_train_16g.json -g 1
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 train_diffusion.py ... -g 8

Opt-in extras (never on by default): --random-init (no autoencoder checkpoint: smoke / benchmark runs),
--synthetic N (write N synthetic NPZ pairs into npz_dir first), --max-steps K (stop after K optimizer steps),
--reference-rng-order (also run the label encode the reference uses only to learn the latent shape),
--sample-steps N (reverse-diffusion steps of the periodic validation sample; 0 = the scheduler's full chain as in the reference).
"scheduler": "rflow" in the config's NoiseScheduler section (default "ddpm", the reference's) trains a rectified-flow model instead: the
noising, the velocity target and the timestep draw of ldm3d.schedulers.RFlowScheduler, everything else unchanged.
--ema-decay F (also diffusion_train.ema_decay in the config; the flag wins) keeps an exponential moving average of the UNet weights
inside the fused Adam launch (warm-up min(F, (1 + n) / (10 + n)) unless --no-ema-warmup): the validation loss, the "best" decision,
the periodic sample and --val-metrics then use the EMA weights, and every save also writes diffusion_unet_ema.pt /
diffusion_unet_ema_last.pt (load them with inference.py --ema); the live files keep their meaning.  Every save also writes
diffusion_train_state.pt (optimizer moments, step and skip counters, EMA, lr schedule, epoch, total_step, best_val), and --resume
continues from it and diffusion_unet_last.pt (loader order and RNG streams are NOT restored).
--cache-latents encodes the training and the validation files once with the frozen autoencoder (every rank the whole set), keeps their
latent means and sigmas on the device (ldm3d/latents.py) and runs every training and validation step from there: the step then holds no
autoencoder call, no loader copy and no host-side randn; the draws come from the kernel (ldm_latent_batch), keyed by the seed, the step
count and the dataset index.  The loaders' batch samplers still decide which samples a rank sees.
--loss-weighting min_snr (--snr-gamma F, default 5) weights each sample's loss by the Min-SNR-gamma weight of its timestep, and
--timestep-sampling loss_aware (--timestep-bins K, default 20) draws the timesteps in proportion to a running per-bin loss estimate with
the importance weights that keep the objective unbiased (ldm3d/loss_weighting.py; config keys diffusion_train.loss_weighting, snr_gamma,
timestep_sampling, timestep_bins; the flags win).  With either on, train_diffusion_loss_iter_unweighted is logged beside the loss that
is minimised and every validation appends the per-bin loss table to <tfevent_path>/diffusion/loss_by_timestep.jsonl; validation itself
stays uniform and unweighted.  Not for "scheduler": "rflow".
--grad-accum-steps K (also diffusion_train.grad_accum_steps in the config; the flag wins; default 1) takes one optimizer step per K
batches on the mean of their gradients, accumulated inside the backward's buckets (ldm_model_set_grad_accum): the effective batch is
K * batch_size * gpus, and the data-parallel exchange runs once per K backward passes.  --max-steps keeps counting optimizer steps;
train_diffusion_loss_iter is logged per batch and train_diffusion_loss_window (the mean over the window) per optimizer step.  A window left
open at a save is not part of the resume state: a resumed run starts a fresh window.
Scalars go to <tfevent_path>/diffusion/scalars.jsonl (tensorboard is not a dependency here); the periodic conditional sample of
:308-359 (every 2 * val_interval epochs on rank 0) goes to <tfevent_path>/diffusion/samples/epoch_<n>.npz as centre slices."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def centre_slices(vol):
    """The three centre slices of a [D, H, W] volume (visualize_one_slice_in_3d_image of 3d_ldm/utils.py at the centre of each axis)."""
    d, h, w = vol.shape
    return [vol[d // 2].float().cpu().numpy(), vol[:, h // 2].float().cpu().numpy(), vol[:, :, w // 2].float().cpu().numpy()]


def sample_validation_volume(trainer, val_loader, device, out_dir, epoch, sample_steps, scalar, schedule_args=None, val_metrics=False,
                             use_ema=False, cfg=None, cfg_fill_value=-1.0):
    """3d_ldm/train_diffusion.py:306-359: noise in the shape of the label latents (:309-310), image latents of the first sample of the
    last validation batch (:324), ``inferer.sample(input_noise, autoencoder, unet, scheduler, conditioning=image_latents,
    mode="concat")`` (:326-333), then the centre slices of low-count input, high-count ground truth and the conditional sample
    (:335-359) -- written as one NPZ per epoch instead of TensorBoard images.  The chain runs on the device-resident sampler (one HIP
    graph launch per step) seeded from torch's RNG; ``--sample-steps N`` (an extra) replaces the full DDPM chain by N DDIM steps
    over the same beta schedule; a rectified-flow model (``"scheduler": "rflow"``) samples N Euler steps of an RFlowScheduler, all T
    without the flag, with the latent's spatial size as ``input_img_size_numel`` of the timestep transform.  ``val_metrics`` (--val-metrics) also logs val_psnr / val_ssim / val_nrmse of the sample against the
    ground truth (ldm3d/metrics.py: one launch, data_range 1 as the loaders scale).  ``use_ema``: the UNet samples with the optimizer's
    EMA weights.  ``cfg`` (--sample-cfg W): the sample is drawn under classifier-free guidance, the unconditional half conditioned on
    ``cfg_fill_value``."""
    import numpy as np
    import torch
    from ldm3d.schedulers import DDIMScheduler, RFlowScheduler
    batch = None
    for batch in val_loader:                                  # the reference uses whatever batch the validation loop ended on
        pass
    if batch is None:
        return None
    images, labels = batch["image"].to(device).float(), batch["label"].to(device).float()
    unet, autoencoder, inferer = trainer.unet, trainer.autoencoder, trainer.inferer
    was_training = unet.training
    unet.eval()
    import contextlib
    ema = trainer.optimizer.ema_weights() if use_ema else contextlib.nullcontext()
    with torch.no_grad(), ema:
        shape = autoencoder.encode_stage_2_inputs(labels[0:1]).shape
        test_noise = torch.randn(shape, dtype=torch.float32).to(device)
        image_latents = autoencoder.encode_stage_2_inputs(images[0:1])
        sch = inferer.scheduler
        if getattr(sch, "kind", None) == 3:                 # rectified flow: Euler steps on a scheduler of the sample's own
            sch = RFlowScheduler(**schedule_args)
            numel = 1
            for s in shape[2:]:
                numel *= int(s)
            sch.set_timesteps(sample_steps or sch.num_train_timesteps, input_img_size_numel=numel)
        elif sample_steps and sample_steps < sch.num_train_timesteps and schedule_args:
            sch = DDIMScheduler(**schedule_args)
            sch.set_timesteps(sample_steps)
        t0 = time.perf_counter()
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        sample = inferer.sample(input_noise=test_noise, autoencoder_model=autoencoder, diffusion_model=unet, scheduler=sch,
                                conditioning=image_latents, mode="concat", fused_seed=seed, cfg=cfg, cfg_fill_value=cfg_fill_value)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    unet.train(was_training)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"epoch_{epoch}.npz")
    arrays = {}
    for name, vol in (("val_lowcount_input", images[0, 0]), ("val_highcount_gt", labels[0, 0]), ("val_denoised_cond", sample[0, 0])):
        for axis, sl in enumerate(centre_slices(vol)):
            arrays[f"{name}_{axis}"] = sl
    np.savez_compressed(path, **arrays)
    err = float((sample[0, 0] - labels[0, 0]).abs().mean())
    scalar("val_denoised_cond_l1", err, epoch)
    if val_metrics:
        from ldm3d.metrics import image_metrics
        m = image_metrics(sample[0:1].float(), labels[0:1], data_range=1.0)
        vals = torch.stack([m["psnr"][0], m["ssim"][0], m["nrmse"][0]]).cpu().tolist()      # one host read
        for tag, v in zip(("val_psnr", "val_ssim", "val_nrmse"), vals):
            scalar(tag, v, epoch)
        print(f"Epoch {epoch}: conditional sample vs ground truth: PSNR {vals[0]:.2f} dB, SSIM {vals[1]:.4f}, NRMSE {vals[2]:.4f}")
    print(f"Epoch {epoch}: conditional sample ({len(sch.timesteps)} steps, {dt:.2f} s) -> {path}, L1 vs ground truth {err:.4f}")
    return path


def scheduler_args(noise_scheduler: dict) -> dict:
    """Keyword arguments of every scheduler built from the config's NoiseScheduler section (3d_ldm/train_diffusion.py:140-145):
    the training DDPM schedule and the DDIM schedule of the validation sample.  ``prediction_type`` is optional ("epsilon")."""
    return dict(num_train_timesteps=noise_scheduler["num_train_timesteps"], schedule="scaled_linear_beta",
                beta_start=noise_scheduler["beta_start"], beta_end=noise_scheduler["beta_end"],
                prediction_type=noise_scheduler.get("prediction_type", "epsilon"))


def build_noise_scheduler(noise_scheduler: dict):
    """-> (the training scheduler of the config's NoiseScheduler section, the keyword arguments that rebuild one like it for the
    validation sample).  ``"scheduler"``: "ddpm" (default, the reference's behaviour) or "rflow" (rectified flow: RFlowScheduler with the
    section's use_discrete_timesteps, sample_method, loc, scale, use_timestep_transform, transform_scale, base_img_size_numel)."""
    from ldm3d.schedulers import DDPMScheduler, RFlowScheduler, noise_scheduler_name, rflow_config_args
    if noise_scheduler_name(noise_scheduler) == "rflow":
        kw = rflow_config_args(noise_scheduler)
        return RFlowScheduler(**kw), kw
    kw = scheduler_args(noise_scheduler)
    return DDPMScheduler(**kw), kw


def merge_grad_accum_steps(flag, train_cfg: dict) -> int:
    """--grad-accum-steps if given, else diffusion_train.grad_accum_steps of the config, else 1."""
    k = flag if flag is not None else train_cfg.get("grad_accum_steps", 1)
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise SystemExit(f"grad_accum_steps must be an integer >= 1, got {k!r}")
    return k


def build_parser():
    parser = argparse.ArgumentParser(description="Latent diffusion model training (MI355X-native)")
    parser.add_argument("-e", "--environment-file", default="./config/environment.json")
    parser.add_argument("-c", "--config-file", default="./config/config_train_32g.json")
    parser.add_argument("-g", "--gpus", default=1, type=int, help="number of gpus per node")
    parser.add_argument("--random-init", action="store_true")
    parser.add_argument("--synthetic", type=int, default=0)
    parser.add_argument("--max-steps", type=int, default=0)
    parser.add_argument("--reference-rng-order", action="store_true")
    parser.add_argument("--gpu-transforms", action="store_true",
                        help="percentile intensity scaling on the GPU (ldm_op_scale_intensity_percentiles) instead of in the host loader")
    parser.add_argument("--precision", default=None, choices=["bf16", "fp32"],
                        help="arithmetic of the networks: bf16 (default, the fast path) or fp32 (the reference's own arithmetic, 1e-5 from its CPU path; also LDM_PRECISION)")
    parser.add_argument("--val-metrics", action="store_true",
                        help="log val_psnr / val_ssim / val_nrmse of the periodic validation sample against its ground truth (ldm_op_image_metrics)")
    parser.add_argument("--sample-steps", type=int, default=0,
                        help="steps of the periodic validation sample (0 = all num_train_timesteps, as 3d_ldm/train_diffusion.py:326-333)")
    parser.add_argument("--grad-allreduce-dtype", default="fp32", choices=["fp32", "bf16"],
                        help="wire format of the data-parallel gradient all-reduce (the reference's DDP uses fp32)")
    parser.add_argument("--ema-decay", type=float, default=None,
                        help="keep an exponential moving average of the UNet weights with this decay (e.g. 0.999) inside the fused Adam step; "
                             "validation, the best-checkpoint decision and the periodic sample use it, and diffusion_unet_ema*.pt are written "
                             "(default: diffusion_train.ema_decay of the config, else off)")
    parser.add_argument("--no-ema-warmup", action="store_true",
                        help="use --ema-decay from the first step instead of the warm-up min(decay, (1 + n) / (10 + n)) over applied steps")
    parser.add_argument("--cond-drop-prob", type=float, default=None,
                        help="train for classifier-free guidance: replace each training sample's condition by --cfg-fill-value with this "
                             "probability (default: diffusion_train.cond_drop_prob of the config, else 0 = off); validation never drops")
    parser.add_argument("--cfg-fill-value", type=float, default=-1.0,
                        help="value of the dropped (unconditional) condition, MONAI's cfg_fill_value")
    parser.add_argument("--sample-cfg", type=float, default=None,
                        help="guidance scale of the periodic validation sample (inferer.sample(cfg=W)); default: unguided")
    parser.add_argument("--loss-weighting", default=None, choices=["none", "min_snr"],
                        help="per-timestep loss weights: min_snr = Min-SNR-gamma for the scheduler's prediction type "
                             "(default: diffusion_train.loss_weighting of the config, else none)")
    parser.add_argument("--snr-gamma", type=float, default=None, help="gamma of --loss-weighting min_snr (default: diffusion_train.snr_gamma, else 5)")
    parser.add_argument("--timestep-sampling", default=None, choices=["uniform", "loss_aware"],
                        help="how training timesteps are drawn: uniform (the reference's randint) or loss_aware (in proportion to a running "
                             "per-bin loss estimate, importance-weighted; default: diffusion_train.timestep_sampling, else uniform)")
    parser.add_argument("--timestep-bins", type=int, default=None,
                        help="bins of the per-timestep loss tracker (default: diffusion_train.timestep_bins, else 20)")
    parser.add_argument("--cache-latents", action="store_true",
                        help="encode the training and validation sets once, keep (mu, sigma) of every latent on the device and train / validate "
                             "from that cache (one launch per step instead of two autoencoder encodes); not with --reference-rng-order")
    parser.add_argument("--resume", action="store_true",
                        help="continue from model_dir/diffusion_train_state.pt (optimizer moments, step / skip counters, EMA, lr schedule, epoch, "
                             "total_step, best_val) and diffusion_unet_last.pt; loader order and RNG state are NOT restored")
    parser.add_argument("--grad-accum-steps", type=int, default=None,
                        help="optimizer step once per K batches on the mean of their gradients, accumulated inside the backward's buckets; "
                             "--max-steps still counts optimizer steps (default: diffusion_train.grad_accum_steps of the config, else 1).  "
                             "A partly filled window is not saved: --resume starts a fresh one")
    return parser


def main():
    parser = build_parser()
    args = parser.parse_args()
    if args.cache_latents and args.reference_rng_order:
        raise SystemExit("--cache-latents and --reference-rng-order exclude each other: the cached step runs no autoencoder encode and draws "
                         "inside its kernel, so the reference's RNG order cannot be kept")
    if args.cond_drop_prob is not None and not 0.0 <= args.cond_drop_prob <= 1.0:
        parser.error("--cond-drop-prob must lie in [0, 1]")
    if args.precision:
        os.environ["LDM_PRECISION"] = args.precision     # read by every network at construction (networks.py)

    import torch
    from ldm3d import parallel
    from ldm3d.config import define_instance
    from ldm3d.data import prepare_dataloader, write_synthetic_pairs
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.trainer import DiffusionTrainer, GradSync, compute_scale_factor

    ddp = args.gpus > 1
    rank = int(os.environ.get("LOCAL_RANK", "0")) if ddp else 0
    world = int(os.environ.get("WORLD_SIZE", "1")) if ddp else 1
    if ddp:
        parallel.setup_ddp(int(os.environ.get("RANK", rank)), world)
    device = torch.device("cuda", rank)
    torch.cuda.set_device(device)
    torch.set_num_threads(4)

    for path in (args.environment_file, args.config_file):
        for k, v in json.load(open(path)).items():
            setattr(args, k, v)
    torch.manual_seed(42)                               # set_determinism(42), train_diffusion.py:66

    tcfg = args.diffusion_train
    accum = merge_grad_accum_steps(args.grad_accum_steps, tcfg)
    if args.synthetic and rank == 0:
        write_synthetic_pairs(args.npz_dir, args.synthetic, tcfg["patch_size"], seed=int(getattr(args, "seed", 0)))
    if ddp:
        torch.distributed.barrier()
    train_loader, val_loader = prepare_dataloader(args, tcfg["batch_size"], tcfg["patch_size"], randcrop=False, rank=rank,
                                                  world_size=world, scale_on_host=not args.gpu_transforms)
    # what --cache-latents encodes and iterates: the datasets, and the loaders' own batch samplers (lists of dataset indices)
    train_set, val_set, train_batches, val_batches = train_loader.dataset, val_loader.dataset, train_loader.batch_sampler, val_loader.batch_sampler
    if args.gpu_transforms:                                # raw crops from the loader; the scaling runs on the device, batch by batch
        from ldm3d.data import gpu_scale_batch

        class _OnDevice:
            def __init__(self, loader):
                self.loader, self.sampler = loader, getattr(loader, "sampler", None)

            def __iter__(self):
                return (gpu_scale_batch(b, device) for b in self.loader)

            def __len__(self):
                return len(self.loader)
        train_loader, val_loader = _OnDevice(train_loader), _OnDevice(val_loader)
    log = None
    if rank == 0:
        tb = os.path.join(getattr(args, "tfevent_path", os.path.join(args.model_dir, "tfevent")), "diffusion")
        Path(tb).mkdir(parents=True, exist_ok=True)
        Path(args.model_dir).mkdir(parents=True, exist_ok=True)
        log = open(os.path.join(tb, "scalars.jsonl"), "a")

    def scalar(tag, value, step):
        if log:
            log.write(json.dumps({"tag": tag, "value": float(value), "step": int(step), "time": time.time()}) + "\n")
            log.flush()

    autoencoder = define_instance(args, "autoencoder_def")
    if not args.random_init:
        autoencoder.load_state_dict(torch.load(os.path.join(args.model_dir, "autoencoder.pt"), map_location="cpu", weights_only=True))
    else:
        with torch.no_grad():
            for p in autoencoder.parameters():
                if p.dim() > 1 and float(p.abs().max()) == 0.0:
                    p.normal_(0.0, 0.02)
    autoencoder = autoencoder.to(device).eval()

    train_cache = val_cache = None
    if args.cache_latents:
        from ldm3d.latents import LatentCache, describe
        train_cache = LatentCache.build(autoencoder, train_set, device)
        print(f"Rank {rank}: {describe('train', train_cache)}")
        val_cache = LatentCache.build(autoencoder, val_set, device)
        print(f"Rank {rank}: {describe('val', val_cache)}")

    first = next(iter(train_loader))
    scale_factor = compute_scale_factor(autoencoder, first["label"].to(device).float(), GradSync())
    print(f"Rank {rank}: scale_factor -> {float(scale_factor):.6f}")
    if rank == 0:                                   # kept next to the checkpoints: inference.py reads it back (the reference
        # hard-codes 1.0 there, inference.py:85)
        os.makedirs(args.model_dir, exist_ok=True)
        with open(os.path.join(args.model_dir, "scale_factor.json"), "w") as fh:
            json.dump({"scale_factor": float(scale_factor)}, fh)

    unet = define_instance(args, "diffusion_def")
    best_path = os.path.join(args.model_dir, "diffusion_unet.pt")
    last_path = os.path.join(args.model_dir, "diffusion_unet_last.pt")
    if getattr(args, "resume_ckpt", False) and os.path.exists(best_path):
        unet.load_state_dict(torch.load(best_path, map_location="cpu", weights_only=True))
        print(f"Rank {rank}: loaded {best_path}")
    elif args.random_init:
        with torch.no_grad():
            for p in unet.parameters():
                if p.dim() > 1 and float(p.abs().max()) == 0.0:
                    p.normal_(0.0, 0.02)
    unet = unet.to(device)
    ns = args.NoiseScheduler
    scheduler, sample_args = build_noise_scheduler(ns)
    inferer = LatentDiffusionInferer(scheduler, scale_factor=float(scale_factor))
    ema_decay = args.ema_decay if args.ema_decay is not None else tcfg.get("ema_decay")
    use_ema = ema_decay is not None
    ema_best_path = os.path.join(args.model_dir, "diffusion_unet_ema.pt")
    ema_last_path = os.path.join(args.model_dir, "diffusion_unet_ema_last.pt")
    state_path = os.path.join(args.model_dir, "diffusion_train_state.pt")
    state = None
    if args.resume:                                     # every rank loads the same files before the optimizer flattens the parameters
        for path in (state_path, last_path):
            if not os.path.exists(path):
                raise SystemExit(f"--resume: {path} not found (written at every save of an earlier run)")
        unet.load_state_dict(torch.load(last_path, map_location=device, weights_only=True))
        state = torch.load(state_path, map_location=device, weights_only=True)
    trainer = DiffusionTrainer(unet, autoencoder, inferer, lr=tcfg["lr"], reference_rng_order=args.reference_rng_order,
                               grad_dtype=torch.bfloat16 if args.grad_allreduce_dtype == "bf16" else torch.float32,
                               ema_decay=ema_decay, ema_warmup=not args.no_ema_warmup,
                               cond_drop_prob=float(args.cond_drop_prob if args.cond_drop_prob is not None else tcfg.get("cond_drop_prob", 0.0)),
                               cfg_fill_value=args.cfg_fill_value,
                               loss_weighting=args.loss_weighting if args.loss_weighting is not None else tcfg.get("loss_weighting", "none"),
                               snr_gamma=float(args.snr_gamma if args.snr_gamma is not None else tcfg.get("snr_gamma", 5.0)),
                               timestep_sampling=(args.timestep_sampling if args.timestep_sampling is not None
                                                  else tcfg.get("timestep_sampling", "uniform")),
                               timestep_bins=int(args.timestep_bins if args.timestep_bins is not None else tcfg.get("timestep_bins", 20)),
                               grad_accum_steps=accum)

    total_step, best_val, done, first_epoch = 0, float("inf"), False, 0
    n_calls = 0                                         # train_step* calls (micro-batches); == total_step + NaN-skips without accumulation
    if state is not None:
        trainer.optimizer.load_state_dict(state["optimizer"])
        trainer.lr_scheduler.load_state_dict(state["lr_scheduler"])
        total_step, best_val, first_epoch = int(state["total_step"]), float(state["best_val"]), int(state["epoch"]) + 1
        # a state file from before these keys existed: the tracker starts empty and the uncached draw counter at total_step
        trainer.load_objective_state_dict(state, default_draws=total_step)
        n_calls = int(state.get("calls", total_step))
        print(f"Rank {rank}: resumed from {state_path}: epoch {first_epoch}, total_step {total_step}, best_val {best_val}")
        if int(state.get("open_micro_batches", 0)):
            print(f"Rank {rank}: the state was saved with {int(state['open_micro_batches'])} micro-batch(es) of an accumulation window open; "
                  "their gradients were not saved, this run starts a fresh window")
    # --cache-latents: the kernel's draws are keyed by the seed of set_determinism(42) above and the count of cached steps, which a resumed run
    # continues from its own total instead of repeating the draws of the first steps
    trainer.cache_seed, trainer.cached_steps = 42, (total_step if accum == 1 else n_calls)
    n_epochs = tcfg["max_epochs"]
    if state is not None and args.max_steps > total_step:   # stopped by --max-steps in its last epoch: the new limit gets at least one more
        n_epochs = max(n_epochs, first_epoch + 1)
    for epoch in range(first_epoch, n_epochs):
        if ddp:
            train_loader.sampler.set_epoch(epoch)
            val_loader.sampler.set_epoch(epoch)
        t0, n_steps = time.perf_counter(), 0
        for step, batch in enumerate(train_batches if train_cache is not None else train_loader):
            if train_cache is not None:                     # batch = the dataset indices the loader would have fetched
                loss, skipped = trainer.train_step_cached(train_cache, batch)
            else:
                loss, skipped = trainer.train_step(batch["image"].to(device), batch["label"].to(device))
            n_calls += 1
            if accum > 1:                                   # per call; the optimizer step (if this call closed a window) below
                scalar("train_diffusion_loss_iter", loss, n_calls)
                if trainer.tracker is not None:
                    scalar("train_diffusion_loss_iter_unweighted", trainer.last_unweighted_loss, n_calls)
                if not trainer.stepped:                     # host bool: no device read on the calls inside a window
                    continue
            if skipped:
                print(f"NaN loss detected at epoch {epoch}, step {step}: skipped on every rank")
                continue
            total_step += 1
            n_steps += 1
            if accum > 1:
                scalar("train_diffusion_loss_window", trainer.window_loss, total_step)
            else:
                scalar("train_diffusion_loss_iter", loss, total_step)
                if trainer.tracker is not None:             # the plain mean beside the weighted loss that is minimised
                    scalar("train_diffusion_loss_iter_unweighted", trainer.last_unweighted_loss, total_step)
            if args.max_steps and total_step >= args.max_steps:
                done = True
                break
        trainer.end_epoch()
        torch.cuda.synchronize()
        if rank == 0:
            print(f"Epoch {epoch}: {n_steps} steps in {time.perf_counter() - t0:.2f} s, lr {trainer.optimizer.param_groups[0]['lr']:.3g}")
        if epoch % tcfg["val_interval"] == 0 or done:
            if val_cache is not None:
                val = trainer.validate_cached(val_cache, val_batches, use_ema=use_ema)
            else:
                val = trainer.validate(val_loader, device, use_ema=use_ema)
            if rank == 0:
                scalar("val_diffusion_loss", val, epoch)
                if trainer.tracker is not None:             # the tracker's one host read
                    with open(os.path.join(tb, "loss_by_timestep.jsonl"), "a") as fh:
                        fh.write(json.dumps({"epoch": int(epoch), "step": int(total_step), "time": time.time(),
                                             "bins": trainer.tracker.report()}) + "\n")
                print(f"Epoch {epoch} val_diffusion_loss{' (EMA weights)' if use_ema else ''}: {val}")
                torch.save(unet.state_dict(), last_path)
                if use_ema:
                    torch.save(trainer.optimizer.ema_state_dict(), ema_last_path)
                if val < best_val:
                    best_val = val
                    torch.save(unet.state_dict(), best_path)
                    if use_ema:
                        torch.save(trainer.optimizer.ema_state_dict(), ema_best_path)
                    print("Got best val noise pred loss. Saved", best_path)
                torch.save({"optimizer": trainer.optimizer.state_dict(), "lr_scheduler": trainer.lr_scheduler.state_dict(),
                            "epoch": epoch, "total_step": total_step, "best_val": best_val, "calls": n_calls,
                            "open_micro_batches": int(trainer.optimizer.micro), **trainer.objective_state_dict()}, state_path)
                # "Test denoising capability" (3d_ldm/train_diffusion.py:306-359): every 2 * val_interval epochs rank 0 samples one
                # high-count volume conditioned on the low-count latents of the last validation batch (mode="concat") and logs the
                # centre slices of input / ground truth / sample along the three axes
                if epoch % (2 * tcfg["val_interval"]) == 0:
                    sample_validation_volume(trainer, val_loader, device, os.path.join(tb, "samples"), epoch, args.sample_steps, scalar,
                                             sample_args, val_metrics=args.val_metrics, use_ema=use_ema, cfg=args.sample_cfg,
                                             cfg_fill_value=args.cfg_fill_value)
        if done:
            break
    if log:
        log.close()
    if ddp:
        parallel.cleanup_ddp()


if __name__ == "__main__":
    main()
