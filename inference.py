#!/usr/bin/env python3
"""Sampling harness on the MI355X-native path: the command line and JSON schema of the reference's 3d_ldm/inference.py
(flags :32-52, config merge :61-67, networks / scheduler / inferer :71-85, sampling loop :88-102).

    python inference.py -e config/environment.json -c config/config_train_16g.json -n 1 [--steps 1000] [--random-init]

Extensions, all opt-in: --steps N switches to an N-step DDIM schedule (the reference always runs the full DDPM chain);
--sampler ddpm | ddim | pndm | dpm picks the scheduler by name (auto = the rule above): pndm with --steps N is PLMS, the 4th-order linear
multistep sampler (N + 1 UNet calls; skip_prk_steps=True, set_alpha_to_one=True), with --pndm-prk MONAI's default PNDM with its
Runge-Kutta warm-up (N + 9 calls); dpm with --steps N is DPM-Solver++ (the 2M multistep solver in its data-prediction form, N UNet
calls, built from the config's DDPM NoiseScheduler section like pndm): --dpm-order 1 | 2 (default 2), --dpm-sde for its stochastic
variant (fresh noise every step, drawn on the device from --seed) and --dpm-spacing linspace | leading | trailing (default linspace);
it composes with --condition, --cfg, --sliding-window, --ensemble, --metrics and --ema and is refused with --init-from-condition and
--inpaint; rflow with --steps N samples a rectified-flow model (a config whose NoiseScheduler section says
"scheduler": "rflow"; auto resolves to it there) by N Euler steps, and any other sampler against such a config is refused, as is the reverse;
--random-init skips the checkpoints (synthetic smoke runs); under torchrun with -g > 1 the -n samples are dealt to the
ranks round-robin (independent chains, no collective: the reference is single process); --batch B denoises B volumes
per chain in one forward and --chains K advances K independent chains concurrently, each on its own stream
(tools/bench_chains.py: 1.6x the latent-steps/s of one-at-a-time at B = 4, 1.9x with 2 chains x B = 4); --condition FILE
runs the conditional sampling the trained model is for: the low-count volume of an NPZ pair is
cropped / percentile-scaled like the training data (3d_ldm/utils.py:94-143), encoded by the autoencoder and concatenated
to the noisy latent at every step (mode="concat", 3d_ldm/train_diffusion.py:326-333), with the scale factor that
train_diffusion.py saved (model_dir/scale_factor.json, or --scale-factor).  Volumes are written as NIfTI-1 by this
package's own writer (nibabel is not a dependency).  --sliding-window (with --condition) denoises the WHOLE scan instead of its
central patch: the scaled scan is padded to a multiple of the VAE factor (at least the patch), encoded whole, and every denoising
step runs the UNet on overlapping patch-size windows of the latent and blends them (--sw-overlap, --sw-batch, --sw-mode); the
NIfTI has the scan's own shape.  --metrics (with --condition) scores every written sample, and the scaled low-count input, against the
pair's high-count volume prepared the same way: 3-D SSIM, PSNR, MSE, MAE and NRMSE from one launch of ldm_op_image_metrics each
(ldm3d/metrics.py), one JSON object per sample in output_dir/metrics.jsonl.  --likelihood (with --condition) samples nothing: it scores
the pair's high-count crop under the model given the low-count latent (LatentDiffusionInferer.get_likelihood, MONAI's variational
bound over the DDPM timesteps, --steps N of them), once per -n noise draw (seed + index), one JSON object per draw in
output_dir/likelihood.jsonl (nats and bits per latent dimension, the t = 0 term); --likelihood-map adds the per-voxel map as NIfTI.
--ema loads the EMA weights that train_diffusion.py
--ema-decay saved (diffusion_unet_ema.pt) in place of diffusion_unet.pt and composes with every other flag.  --ensemble K (with
--condition) draws K samples of the scan, --ensemble-batch M of them per chain, and writes their per-voxel mean (the denoised estimate)
and standard deviation (where the model is unsure) as ensemble_mean_*.nii / ensemble_std_*.nii plus one record in
output_dir/ensemble.jsonl, reduced on the device as the members are decoded (LatentDiffusionInferer.sample_ensemble); --ensemble-keep N
also writes the first N members; with --sliding-window every member is a whole scan; with --metrics the record carries bias_sq and
mean_var_ddof0 (their sum is the members' mean MSE) and the image metrics of the mean, of member 0 and of the input.
--init-from-condition (with --condition) warm-starts every chain from the low-count scan's own scaled latent, the tensor that already
conditions it, instead of pure noise: --strength S in (0, 1] picks the start step k0 = n - int(n S) of the n-step chain (diffusers'
image-to-image convention), the latent is noised to that timestep and only the last n - k0 steps are denoised; --init-invert reaches the
timestep by n - 1 - k0 steps of DDIM inversion instead (--sampler ddim, or auto with --steps).  It composes with --sliding-window, --cfg,
--ensemble (not with --init-invert: the members would be identical), --metrics and --sampler ddpm | ddim | rflow; every written volume
gets a line in output_dir/warm_start.jsonl (start_step, unet_calls = n - k0, mode noised | inverted, inversion_calls) and the same
fields join the metrics.jsonl / ensemble.jsonl records.
--inpaint PAIR.npz keeps the trusted part of a scan and regenerates a region (RePaint on the device sampler): the known latent is the
pair's high-count volume, prepared and encoded as the --condition volume is; --regenerate-box d0:d1,h0:h1,w0:w1 or --regenerate-mask
FILE.npy (1 = regenerate) mark the region in the voxels of the prepared volume (the crop, or the whole scan with --sliding-window); a
latent voxel is kept only if every image voxel under it is kept.  --resample R > 1 with --jump-length J re-denoises every J levels R
times (n + (R - 1) J ((n - 1) // J) UNet calls); --inpaint-paste also copies the original image wherever the image-space mask keeps it.
It composes with --condition, --sliding-window, --cfg, --ensemble, --metrics and --sampler ddpm | ddim | rflow and is refused with pndm,
--init-from-condition, --likelihood and --chains > 1; every run appends one record per scan to output_dir/inpaint.jsonl (n_calls,
jump_length, n_resample, the kept fraction in latent and in image space).
--data-consistency K (with --condition) steers every step by the gradient of a data-consistency loss on the model's own prediction of the
clean latent (diffusion posterior sampling, ldm3d/guidance.py): the denoised latent keeps the --condition latent's means over K^3 cubes.
--dc-scale ZETA is the step size, divided by the residual's norm per step unless --dc-no-normalize.  It runs on the device sampler with
--sampler ddpm | ddim, composes with --init-from-condition and --metrics, and is refused with pndm, dpm, rflow, --cfg, --inpaint,
--sliding-window, --ensemble, --likelihood and --chains > 1.  Every volume gets a line in output_dir/guidance.jsonl (pool, scale, the
first and last per-step residual norm); with --metrics the same record joins metrics.jsonl as "data_consistency".
--data-consistency-image K (with --condition; exclusive with --data-consistency) holds the DECODED prediction to the low-count IMAGE
instead (ldm3d.guidance.ImageConsistencyGuidance): the target is the condition file's low-count volume as the loader normalises it,
averaged once over K^3 image cubes (K must divide the image dims); every step differentiates through the AutoencoderKL decoder
(its data-only backward) and the UNet.  It shares --dc-scale and --dc-no-normalize, allows the same samplers and combinations, and writes
the same guidance.jsonl record plus "space": "image".  Not built: image gradients through the encoder, measurements other than the
pooled quadratic (PSF blur, projections), and data consistency together with --cfg, --inpaint, --sliding-window, --ensemble,
--likelihood or --chains > 1."""
import argparse
import json
import logging
import os
import sys
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
log = logging.getLogger("inference")


def parse_cli():
    ap = argparse.ArgumentParser(description="3D latent diffusion sampling (MI355X-native)")
    ap.add_argument("-e", "--environment-file", default="./config/environment.json", help="JSON with data / model / output paths")
    ap.add_argument("-c", "--config-file", default="./config/config_train_32g.json", help="JSON with network and training hyper-parameters")
    ap.add_argument("-n", "--num", type=int, default=1, help="volumes to generate")
    ap.add_argument("-g", "--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=0, help="0 = all training timesteps with DDPM (reference behaviour); N = N-step DDIM")
    ap.add_argument("--sampler", default="auto", choices=["auto", "ddpm", "ddim", "pndm", "dpm", "rflow"],
                    help="auto: DDPM over all training timesteps, DDIM with --steps N, rflow for a config with \"scheduler\": \"rflow\"; "
                         "ddim / pndm / dpm / rflow need --steps N")
    ap.add_argument("--pndm-prk", action="store_true",
                    help="--sampler pndm: run the Runge-Kutta warm-up (MONAI's PNDMScheduler defaults) instead of PLMS alone")
    ap.add_argument("--dpm-order", type=int, default=None, choices=[1, 2],
                    help="--sampler dpm: 2 = the 2M multistep solver (default), 1 = its first-order step alone")
    ap.add_argument("--dpm-sde", action="store_true", help="--sampler dpm: the stochastic variant (sde-dpmsolver++), noise keyed by --seed")
    ap.add_argument("--dpm-spacing", default=None, choices=["linspace", "leading", "trailing"],
                    help="--sampler dpm: the timestep grid (default linspace)")
    ap.add_argument("--random-init", action="store_true", help="no checkpoints: random weights")
    ap.add_argument("--ema", action="store_true",
                    help="sample with the EMA weights of train_diffusion.py --ema-decay: model_dir/diffusion_unet_ema.pt instead of diffusion_unet.pt")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--batch", type=int, default=1, help="volumes denoised together in one chain")
    ap.add_argument("--chains", type=int, default=1, help="independent chains advanced concurrently on this GPU (own stream + module instance each)")
    ap.add_argument("--eager", action="store_true", help="launch every kernel from the host instead of replaying the UNet's HIP graph")
    ap.add_argument("--condition", default=None, help="NPZ pair whose low-count volume conditions the sampling (mode='concat')")
    ap.add_argument("--cfg", type=float, default=None,
                    help="with --condition: classifier-free guidance scale W (the step takes u + W (c - u) from one UNet call on a doubled "
                         "batch; the model should have been trained with --cond-drop-prob)")
    ap.add_argument("--cfg-fill-value", type=float, default=-1.0, help="--cfg: value of the unconditional half's condition (MONAI's cfg_fill_value)")
    ap.add_argument("--precision", default=None, choices=["bf16", "fp32"],
                        help="arithmetic of the networks: bf16 (default, the fast path) or fp32 (the reference's own arithmetic, 1e-5 from its CPU path; also LDM_PRECISION)")
    ap.add_argument("--scale-factor", type=float, default=None, help="latent scale (default: model_dir/scale_factor.json, else 1.0)")
    ap.add_argument("--sliding-window", action="store_true",
                    help="with --condition: denoise the whole scan, the UNet running on overlapping training-size windows of its latent every step")
    ap.add_argument("--sw-overlap", type=float, default=0.25, help="--sliding-window: overlap of neighbouring windows, in [0, 1)")
    ap.add_argument("--sw-batch", type=int, default=0, help="--sliding-window: windows per UNet call (0 = all that fit in half the free memory)")
    ap.add_argument("--sw-mode", default="gaussian", choices=["gaussian", "constant"], help="--sliding-window: importance map of a window")
    ap.add_argument("--metrics", action="store_true",
                    help="with --condition: score every sample (and the low-count input) against the pair's high-count volume -> output_dir/metrics.jsonl")
    ap.add_argument("--likelihood", action="store_true",
                    help="with --condition: score the pair's high-count volume under the model instead of sampling (get_likelihood: the "
                         "variational bound in nats / bits per latent dimension) -> output_dir/likelihood.jsonl, one record per -n noise draw")
    ap.add_argument("--likelihood-map", action="store_true",
                    help="--likelihood: also write the per-voxel map (sum over timesteps of the channel-mean term, resized to the crop) as NIfTI")
    ap.add_argument("--ensemble", type=int, default=0, metavar="K",
                    help="with --condition: draw K >= 2 samples of the scan and write their per-voxel mean and standard deviation "
                         "(ensemble_mean_*.nii, ensemble_std_*.nii, one record in output_dir/ensemble.jsonl) instead of K volumes")
    ap.add_argument("--ensemble-batch", type=int, default=0, metavar="M",
                    help="--ensemble: members denoised together per chain (0 = all that fit in half the free memory)")
    ap.add_argument("--ensemble-keep", type=int, default=0, metavar="N", help="--ensemble: also write the first N members")
    ap.add_argument("--init-from-condition", action="store_true",
                    help="with --condition: warm-start every chain from the low-count scan's own scaled latent (the condition) instead of "
                         "pure noise, noised to the timestep --strength selects; only the remaining steps are denoised")
    ap.add_argument("--strength", type=float, default=1.0, metavar="S",
                    help="--init-from-condition: fraction of the chain to run, in (0, 1]: start step k0 = n - int(n S), n - k0 UNet calls")
    ap.add_argument("--init-invert", action="store_true",
                    help="--init-from-condition: reach the start timestep by DDIM inversion of the latent (n - 1 - k0 more UNet calls) instead "
                         "of noising it; needs the DDIM sampler")
    ap.add_argument("--inpaint", default=None, metavar="PAIR.npz",
                    help="keep the high-count volume of this NPZ pair outside the region --regenerate-box / --regenerate-mask marks and "
                         "regenerate the region (RePaint) -> output_dir/inpaint.jsonl")
    ap.add_argument("--regenerate-box", default=None, metavar="d0:d1,h0:h1,w0:w1", help="--inpaint: the region to regenerate, in image voxels")
    ap.add_argument("--regenerate-mask", default=None, metavar="FILE.npy", help="--inpaint: the region to regenerate as a 0 / 1 volume, 1 = regenerate")
    ap.add_argument("--jump-length", type=int, default=1, metavar="J", help="--inpaint: levels a resampling jump goes back")
    ap.add_argument("--resample", type=int, default=1, metavar="R", help="--inpaint: times every J levels are denoised (1 = the plain chain)")
    ap.add_argument("--inpaint-paste", action="store_true",
                    help="--inpaint: the written volume takes the original image wherever the image-space mask keeps it")
    ap.add_argument("--data-consistency", type=int, default=0, metavar="K",
                    help="with --condition: measurement-guided sampling (ldm3d/guidance.py) that holds the denoised latent to the condition "
                         "latent's means over K^3 cubes (1 = voxel-wise) -> output_dir/guidance.jsonl")
    ap.add_argument("--data-consistency-image", type=int, default=0, metavar="K",
                    help="with --condition: measurement-guided sampling that holds the DECODED prediction to the low-count volume's means "
                         "over K^3 image cubes (1 = voxel-wise), through the decoder's input gradients -> output_dir/guidance.jsonl")
    ap.add_argument("--dc-scale", type=float, default=1.0, metavar="ZETA",
                    help="--data-consistency / --data-consistency-image: the guidance step size")
    ap.add_argument("--dc-no-normalize", action="store_true",
                    help="--data-consistency / --data-consistency-image: use ZETA itself instead of ZETA / |residual| per step")
    ns = ap.parse_args()
    if ns.data_consistency and ns.data_consistency_image:
        ap.error("--data-consistency and --data-consistency-image are exclusive: one measurement per chain")
    if not ns.data_consistency and not ns.data_consistency_image and (ns.dc_scale != 1.0 or ns.dc_no_normalize):
        ap.error("--dc-scale and --dc-no-normalize belong to --data-consistency K or --data-consistency-image K")
    for flag, k, what in (("--data-consistency", ns.data_consistency, "latent"), ("--data-consistency-image", ns.data_consistency_image, "low-count volume")):
        if not k:
            continue
        if k < 1:
            ap.error(f"{flag} K needs K >= 1")
        if not ns.condition:
            ap.error(f"{flag} holds the sample to the --condition scan's {what}: it needs --condition FILE")
        if ns.sampler in ("pndm", "dpm", "rflow"):
            ap.error(f"{flag} is built on the DDPM / DDIM step: --sampler {ns.sampler} is refused")
        for on, other in ((ns.cfg is not None, "--cfg"), (bool(ns.inpaint), "--inpaint"), (ns.sliding_window, "--sliding-window"),
                          (bool(ns.ensemble), "--ensemble"), (ns.chains > 1, "--chains > 1"), (ns.likelihood, "--likelihood")):
            if on:
                ap.error(f"{flag} together with {other} is not implemented")
    if not ns.inpaint and (ns.regenerate_box or ns.regenerate_mask or ns.jump_length != 1 or ns.resample != 1 or ns.inpaint_paste):
        ap.error("--regenerate-box, --regenerate-mask, --jump-length, --resample and --inpaint-paste belong to --inpaint")
    ns.regenerate = None
    if ns.inpaint:
        if bool(ns.regenerate_box) == bool(ns.regenerate_mask):
            ap.error("--inpaint needs the region to regenerate: exactly one of --regenerate-box and --regenerate-mask")
        if ns.regenerate_box:
            try:
                ns.regenerate = parse_box(ns.regenerate_box)
            except ValueError as e:
                ap.error(f"--regenerate-box: {e}")
        if ns.jump_length < 1 or ns.resample < 1:
            ap.error("--jump-length and --resample must be at least 1")
        if ns.sampler == "pndm":
            ap.error("--inpaint: a PNDM chain's multistep history is not defined across jumps, --sampler pndm is refused")
        if ns.sampler == "dpm":
            ap.error("--inpaint: a DPM-Solver++ chain's multistep history is not defined across jumps, --sampler dpm is refused")
        if ns.init_from_condition:
            ap.error("--inpaint starts from noise: --init-from-condition (a warm or inverted start) is refused")
        if ns.likelihood:
            ap.error("--inpaint samples: --likelihood is refused")
        if ns.chains > 1:
            ap.error("--inpaint is not implemented for concurrent chains: --chains must be 1")
    if (ns.strength != 1.0 or ns.init_invert) and not ns.init_from_condition:
        ap.error("--strength and --init-invert belong to --init-from-condition")
    if ns.init_from_condition:
        if not ns.condition:
            ap.error("--init-from-condition starts from the --condition scan's latent: it needs --condition FILE")
        if ns.sampler == "pndm":
            ap.error("--init-from-condition: a PNDM chain is defined from its first timestep, --sampler pndm is refused")
        if ns.sampler == "dpm":
            ap.error("--init-from-condition: a DPM-Solver++ chain is defined from its first timestep, --sampler dpm is refused")
        if ns.likelihood:
            ap.error("--init-from-condition warm-starts sampling: --likelihood is refused")
        if ns.chains > 1:
            ap.error("--init-from-condition is not implemented for concurrent chains: --chains must be 1")
        if ns.init_invert and ns.ensemble:
            ap.error("--init-invert is deterministic: the members of an --ensemble would be identical")
    if not ns.ensemble and (ns.ensemble_batch or ns.ensemble_keep):
        ap.error("--ensemble-batch and --ensemble-keep belong to --ensemble K")
    if ns.ensemble:
        if ns.ensemble < 2:
            ap.error("--ensemble K needs K >= 2 members")
        if not ns.condition:
            ap.error("--ensemble samples the posterior of a given scan: it needs --condition FILE")
        if ns.num != 1:
            ap.error("--ensemble K sets the number of draws: -n must be 1")
        if ns.chains > 1 or ns.batch > 1:
            ap.error("--ensemble batches its members itself (--ensemble-batch): --chains and --batch must be 1")
        if ns.likelihood:
            ap.error("--ensemble samples, --likelihood scores: pass one of them")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            ap.error("--ensemble runs in one process (merging accumulators across ranks is not implemented): WORLD_SIZE must be 1")
        if ns.ensemble_batch < 0 or ns.ensemble_batch > ns.ensemble:
            ap.error(f"--ensemble-batch must be in 1 .. {ns.ensemble}")
        if ns.ensemble_batch and ns.sliding_window:
            ap.error("--sliding-window denoises one whole scan per chain: --ensemble-batch is refused (use --sw-batch)")
        if not 0 <= ns.ensemble_keep <= ns.ensemble:
            ap.error(f"--ensemble-keep must be in 0 .. {ns.ensemble}")
    if ns.likelihood_map and not ns.likelihood:
        ap.error("--likelihood-map belongs to --likelihood")
    if ns.likelihood:
        if not ns.condition:
            ap.error("--likelihood scores the high-count volume of a pair: it needs --condition FILE")
        if ns.sampler not in ("auto", "ddpm"):
            ap.error(f"--likelihood is defined for the DDPM posterior only: --sampler {ns.sampler} is refused")
        if ns.cfg is not None:
            ap.error("--likelihood scores the model's own prediction: --cfg is refused")
        if ns.sliding_window:
            ap.error("--likelihood scores one training-size crop: --sliding-window is refused")
        if ns.chains > 1:
            ap.error("--likelihood runs one loop at a time: --chains must be 1")
    if ns.sampler in ("ddim", "pndm", "dpm", "rflow") and ns.steps < 1:
        ap.error(f"--sampler {ns.sampler} needs --steps N")
    if ns.sampler == "ddpm" and ns.steps:
        ap.error("--sampler ddpm runs all training timesteps: drop --steps")
    if ns.pndm_prk and ns.sampler != "pndm":
        ap.error("--pndm-prk belongs to --sampler pndm")
    if ns.sampler != "dpm" and (ns.dpm_order is not None or ns.dpm_sde or ns.dpm_spacing is not None):
        ap.error("--dpm-order, --dpm-sde and --dpm-spacing belong to --sampler dpm")
    if ns.sampler == "pndm" and ns.pndm_prk and ns.steps < 4:
        ap.error("--pndm-prk needs --steps >= 4")
    if ns.cfg is not None and not ns.condition:
        ap.error("--cfg guides towards a condition: it needs --condition FILE")
    if ns.cfg is not None and ns.chains > 1:
        ap.error("--cfg is not implemented for concurrent chains: --chains must be 1")
    if ns.metrics and not ns.condition:
        ap.error("--metrics scores against the high-count volume of a pair: it needs --condition FILE")
    if ns.sliding_window:
        if not ns.condition:
            ap.error("--sliding-window denoises a given scan: it needs --condition FILE")
        if ns.chains > 1 or ns.batch > 1:
            ap.error("--sliding-window samples one whole scan at a time: --chains and --batch must be 1")
    if ns.precision:
        os.environ["LDM_PRECISION"] = ns.precision     # read by every network at construction (networks.py)
    for path in (ns.environment_file, ns.config_file):           # both JSON files land on the namespace, config last
        with open(path) as fh:
            vars(ns).update(json.load(fh))
    # a flow model sampled on a beta schedule (or the reverse) is garbage, not a variant: the config decides the family
    from ldm3d.schedulers import noise_scheduler_name
    try:
        flow = noise_scheduler_name(ns.NoiseScheduler) == "rflow"
    except ValueError as e:
        ap.error(str(e))
    if ns.sampler == "auto" and flow:
        ns.sampler = "rflow"
        if ns.steps < 1:
            ap.error("the config trains a rectified-flow model (NoiseScheduler.scheduler = rflow): sampling needs --steps N")
    if flow and ns.sampler != "rflow":
        ap.error(f"--sampler {ns.sampler} against a rectified-flow config (NoiseScheduler.scheduler = rflow): use --sampler rflow --steps N")
    if not flow and ns.sampler == "rflow":
        ap.error("--sampler rflow needs a config whose NoiseScheduler section says \"scheduler\": \"rflow\"")
    ns.start_step = 0
    if ns.init_from_condition:
        from ldm3d.schedulers import start_step_for_strength
        T = int(ns.NoiseScheduler["num_train_timesteps"])
        ddim = ns.sampler == "ddim" or (ns.sampler == "auto" and 0 < ns.steps < T)
        if ns.init_invert and not ddim:
            ap.error("--init-invert is DDIM inversion: it needs --sampler ddim, or auto with --steps N")
        try:
            ns.start_step = start_step_for_strength(ns.steps if ns.sampler == "rflow" or ddim else T, ns.strength)
        except ValueError as e:
            ap.error(f"--strength: {e}")
    return ns


def parse_box(text):
    """"d0:d1,h0:h1,w0:w1" -> ((d0, d1), (h0, h1), (w0, w1)), 0 <= lo < hi per axis"""
    parts = text.split(",")
    if len(parts) != 3:
        raise ValueError(f"three ranges d0:d1,h0:h1,w0:w1 are needed, got {text!r}")
    box = []
    for part in parts:
        lo, sep, hi = part.partition(":")
        if not sep:
            raise ValueError(f"a range is lo:hi, got {part!r}")
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi:
            raise ValueError(f"a range needs 0 <= lo < hi, got {part!r}")
        box.append((lo, hi))
    return tuple(box)


def inpaint_setup(ns, autoencoder, inferer, scheduler, device, whole):
    """--inpaint -> (the keyword arguments that make ``sample`` / ``sample_sliding_window`` / ``sample_ensemble`` inpaint, the run's
    record, (the prepared original image, its image-space keep mask) [1, 1, D, H, W] for --inpaint-paste).  The known latent is the
    pair's high-count volume prepared as the --condition volume is (the centre crop, or the whole padded scan); the region comes in
    the voxels of that volume before padding (padding is kept: it holds nothing to regenerate); the latent mask is its min-pool."""
    import numpy as np
    import torch
    from ldm3d.inferer import latent_keep_mask
    from ldm3d.schedulers import repaint_schedule
    if not ns.inpaint:
        return {}, {}, None
    patch = [int(p) for p in ns.diffusion_train["patch_size"]]
    f = autoencoder.factor
    if whole:
        vol, shape = prepared_scan(ns.inpaint, patch, f, high_count=True)
    else:
        vol = prepared_patch(ns.inpaint, patch, f, high_count=True)
        shape = tuple(vol.shape)
    regen = np.zeros(vol.shape, dtype=np.float32)
    if ns.regenerate is not None:
        if any(hi > d for (lo, hi), d in zip(ns.regenerate, shape)):
            raise SystemExit(f"--regenerate-box {ns.regenerate_box} does not fit the volume {shape}")
        (d0, d1), (h0, h1), (w0, w1) = ns.regenerate
        regen[d0:d1, h0:h1, w0:w1] = 1.0
    else:
        m = np.load(ns.regenerate_mask)
        if tuple(m.shape) != tuple(shape) or not np.isin(m, (0, 1)).all():
            raise SystemExit(f"--regenerate-mask must be a 0 / 1 volume of shape {shape}, got {tuple(m.shape)}")
        regen[:shape[0], :shape[1], :shape[2]] = m
    x = torch.from_numpy(np.ascontiguousarray(vol))[None, None].to(device)
    keep_img = torch.from_numpy(1.0 - regen).to(device)
    with torch.no_grad():
        known = autoencoder.encode_stage_2_inputs(x) * inferer.scale_factor
    keep_lat = latent_keep_mask(keep_img, f)
    if tuple(keep_lat.shape) != tuple(known.shape[2:]):
        raise SystemExit(f"the latent {tuple(known.shape[2:])} is not the image {tuple(vol.shape)} over the autoencoder's factor {f}")
    rec = {"n_calls": len(repaint_schedule(len(scheduler.timesteps), ns.jump_length, ns.resample)), "jump_length": ns.jump_length,
           "n_resample": ns.resample, "kept_latent": float(keep_lat.mean()), "kept_image": float(keep_img.mean()),
           "paste": bool(ns.inpaint_paste)}
    kw = dict(inpaint_latent=known, keep_mask=keep_lat, jump_length=ns.jump_length, n_resample=ns.resample)
    return kw, rec, (x, keep_img[None, None])


def inpaint_paste(ns, vol, paste):
    """--inpaint-paste: ``vol`` [B, 1, D, H, W] (or a leading corner of it) with the original image wherever the image-space mask keeps it"""
    import torch
    if not (ns.inpaint and ns.inpaint_paste):
        return vol
    image, keep = (t[:, :, :vol.shape[2], :vol.shape[3], :vol.shape[4]] for t in paste)
    return torch.where(keep != 0, image.to(vol.dtype), vol)


def write_inpaint_record(out_dir, written, rec):
    """One line per scan in output_dir/inpaint.jsonl: what the chain cost and how much of the scan it kept."""
    if rec:
        with open(os.path.join(str(out_dir), "inpaint.jsonl"), "a") as fh:
            fh.write(json.dumps(dict(file=os.path.basename(str(written)), **rec)) + "\n")


def warm_start(ns, inferer, unet, scheduler, latent, **window_kw):
    """--init-from-condition -> (the keyword arguments that warm-start ``sample`` / ``sample_sliding_window`` / ``sample_ensemble`` from
    ``latent``, the fields of the run's record).  Noised: the chain's own start noise at ``timesteps[start_step]``.  --init-invert:
    n - 1 - start_step reversed DDIM steps reach that timestep (``LatentDiffusionInferer.invert``, conditioned as the sampling is)."""
    if not ns.init_from_condition:
        return {}, {}
    n, k0 = len(scheduler.timesteps), ns.start_step
    rec = {"start_step": k0, "unet_calls": n - k0, "mode": "inverted" if ns.init_invert else "noised", "strength": ns.strength}
    if not ns.init_invert:
        return dict(init_latent=latent, start_step=k0), rec
    rec["inversion_calls"] = n - 1 - k0
    if n - 1 - k0 > 0:
        latent = inferer.invert(latent, unet, scheduler=scheduler, conditioning=latent, mode="concat", n_steps=n - 1 - k0, cfg=ns.cfg,
                                cfg_fill_value=ns.cfg_fill_value, **window_kw)
    return dict(init_latent=latent, start_step=k0, init_inverted=True), rec


def write_warm_record(out_dir, written, rec):
    """One line per written volume in output_dir/warm_start.jsonl: where the chain started and what it cost."""
    if rec:
        with open(os.path.join(str(out_dir), "warm_start.jsonl"), "a") as fh:
            fh.write(json.dumps(dict(file=os.path.basename(str(written)), **rec)) + "\n")


def load_networks(ns, device, only_unet=False, like=None):
    import torch
    from ldm3d.config import define_instance
    if only_unet:                                                  # another instance with the same weights
        net = define_instance(ns, "diffusion_def")
        net.load_state_dict(like.state_dict())
        return net.to(device).eval()
    nets = {}
    unet_ckpt = "diffusion_unet_ema.pt" if getattr(ns, "ema", False) else "diffusion_unet.pt"
    if getattr(ns, "ema", False) and not os.path.exists(os.path.join(ns.model_dir, unet_ckpt)):
        raise SystemExit(f"--ema: {os.path.join(ns.model_dir, unet_ckpt)} not found (train_diffusion.py --ema-decay F writes it)")
    for key, ckpt in (("autoencoder_def", "autoencoder.pt"), ("diffusion_def", unet_ckpt)):
        net = define_instance(ns, key)
        if ns.random_init:
            with torch.no_grad():                                  # MONAI zero-initialises some convs: give them values
                for p in net.parameters():
                    if p.dim() > 1 and not bool(p.any()):
                        p.normal_(0.0, 0.02)
        else:
            net.load_state_dict(torch.load(os.path.join(ns.model_dir, ckpt), weights_only=True))
        nets[key] = net.to(device).eval()
    return nets["autoencoder_def"], nets["diffusion_def"]


def latent_numel(ns, spatial=None, factor=4) -> int:
    """Voxels of the latent a chain denoises (``input_img_size_numel`` of RFlowScheduler's timestep transform): ``spatial`` or the
    training patch over the autoencoder's factor."""
    spatial = spatial if spatial is not None else [int(p) // factor for p in ns.diffusion_train["patch_size"]]
    n = 1
    for s in spatial:
        n *= int(s)
    return n


def make_scheduler(ns, spatial=None):
    from ldm3d.schedulers import (DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, PNDMScheduler, RFlowScheduler,
                                  rflow_config_args)
    cfg = ns.NoiseScheduler
    if getattr(ns, "sampler", "auto") == "rflow":
        sch = RFlowScheduler(**rflow_config_args(cfg))
        sch.set_timesteps(ns.steps, input_img_size_numel=latent_numel(ns, spatial))
        return sch
    kw = dict(num_train_timesteps=cfg["num_train_timesteps"], schedule="scaled_linear_beta", beta_start=cfg["beta_start"],
              beta_end=cfg["beta_end"], prediction_type=cfg.get("prediction_type", "epsilon"))
    sampler = getattr(ns, "sampler", "auto")
    if sampler == "pndm":
        prk = bool(getattr(ns, "pndm_prk", False))    # without the warm-up: PLMS as it is commonly sampled with (ends at abar = 1)
        sch = PNDMScheduler(**kw) if prk else PNDMScheduler(skip_prk_steps=True, set_alpha_to_one=True, **kw)
        sch.set_timesteps(ns.steps)
        return sch
    if sampler == "dpm":
        sch = DPMSolverMultistepScheduler(solver_order=getattr(ns, "dpm_order", None) or 2,
                                          algorithm_type="sde-dpmsolver++" if getattr(ns, "dpm_sde", False) else "dpmsolver++",
                                          timestep_spacing=getattr(ns, "dpm_spacing", None) or "linspace", **kw)
        sch.set_timesteps(ns.steps)
        return sch
    if sampler == "ddim" or (sampler == "auto" and 0 < ns.steps < cfg["num_train_timesteps"]):
        sch = DDIMScheduler(**kw)
        sch.set_timesteps(ns.steps)
        return sch
    return DDPMScheduler(**kw)


def resolve_scale_factor(ns) -> float:
    if ns.scale_factor is not None:
        return float(ns.scale_factor)
    path = os.path.join(getattr(ns, "model_dir", "."), "scale_factor.json")
    if os.path.exists(path):
        with open(path) as fh:
            return float(json.load(fh)["scale_factor"])
    return 1.0                                                   # the reference's hard-coded value (inference.py:85)


def prepared_patch(path, patch, f, high_count=False):
    """The low-count (or high-count) volume of an NPZ pair -> centre crop, 0..99.5 percentile scaling (numpy [D, H, W])."""
    from ldm3d.data import crop, crop_start, load_pair, scale_percentiles
    image = load_pair(path)[1 if high_count else 0]
    # a volume smaller than the patch is used whole (the loaders clip the roi the same way), cut to a multiple of the VAE factor
    roi = [min(int(p), int(d)) // f * f for p, d in zip(patch, image.shape)]
    return scale_percentiles(crop(image, crop_start(image.shape, roi, None), roi))


def prepared_scan(path, patch, f, high_count=False):
    """The low-count (or high-count) volume of an NPZ pair, whole: 0..99.5 percentile scaling, padding with b_min (0) at the far end of
    every axis to max(a multiple of the VAE factor, the patch) -> (numpy [D, H, W], the scan's own shape)."""
    import numpy as np
    from ldm3d.data import load_pair, scale_percentiles
    image = load_pair(path)[1 if high_count else 0]
    shape = tuple(int(d) for d in image.shape)
    padded = [max(-(-d // f) * f, int(p)) for d, p in zip(shape, patch)]
    return np.pad(scale_percentiles(image), [(0, pd - d) for d, pd in zip(shape, padded)], constant_values=0.0), shape


def condition_latent(path, patch, autoencoder, scale_factor, device):
    """Low-count volume of an NPZ pair -> centre crop, 0..99.5 percentile scaling -> scaled image latent [1, C, d, h, w]."""
    import numpy as np
    import torch
    image = prepared_patch(path, patch, autoencoder.factor)
    x = torch.from_numpy(np.ascontiguousarray(image))[None, None].to(device)
    return autoencoder.encode_stage_2_inputs(x) * scale_factor


def whole_scan_latent(path, patch, autoencoder, scale_factor, device):
    """Low-count volume of an NPZ pair, whole: 0..99.5 percentile scaling, padding with b_min (0) at the far end of every axis to
    max(a multiple of the VAE factor, the patch) -> (scaled image latent [1, C, d, h, w], the scan's own shape)."""
    import numpy as np
    import torch
    image, shape = prepared_scan(path, patch, autoencoder.factor)
    x = torch.from_numpy(np.ascontiguousarray(image))[None, None].to(device)
    return autoencoder.encode_stage_2_inputs(x) * scale_factor, shape


METRIC_NAMES = ("ssim", "psnr", "mse", "mae", "nrmse")
SSIM_SETTINGS = dict(data_range=1.0, kernel_type="gaussian", win_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03)


def metric_volumes(path, patch, factor, device, whole):
    """The pair's (low-count, high-count) volumes [1, 1, D, H, W] on the device, prepared as the conditioning is: the patch path's centre
    crop (same start for both) or the whole scan, each scaled by its own 0..99.5 percentiles."""
    import numpy as np
    import torch
    from ldm3d.data import crop, crop_start, load_pair, scale_percentiles
    image, label = load_pair(path)
    if not whole:
        roi = [min(int(p), int(d)) // factor * factor for p, d in zip(patch, image.shape)]
        start = crop_start(image.shape, roi, None)
        image, label = crop(image, start, roi), crop(label, start, roi)
    return tuple(torch.from_numpy(np.ascontiguousarray(scale_percentiles(v)))[None, None].to(device) for v in (image, label))


def write_metrics(out_dir, written, vol, image, label, extra=None):
    """Score `vol` (a view is fine: only W must be contiguous) and the low-count input against the label; append one line to metrics.jsonl
    (`extra`: more fields of the record, such as a warm start's)."""
    from ldm3d.metrics import image_metrics
    rec = {"file": os.path.basename(str(written)), "shape": [int(d) for d in label.shape[2:]], **(extra or {})}
    for name, pred in (("denoised", vol), ("input", image)):
        m = image_metrics(pred, label, **SSIM_SETTINGS)
        rec[name] = {k: float(m[k][0]) for k in METRIC_NAMES}
    rec["ssim_settings"] = dict(SSIM_SETTINGS)
    with open(os.path.join(str(out_dir), "metrics.jsonl"), "a") as fh:
        fh.write(json.dumps(rec) + "\n")
    log.info("metrics %s: denoised %s | input %s", rec["file"], rec["denoised"], rec["input"])
    return rec


def sample_whole_scans(ns, autoencoder, unet, inferer, scheduler, device, rank, world):
    """--sliding-window: every requested sample denoises the whole --condition scan (sample_sliding_window, device sampler)."""
    import torch
    from ldm3d import parallel
    from ldm3d.nifti import save_nifti
    patch = [int(p) for p in ns.diffusion_train["patch_size"]]
    f = autoencoder.factor
    with torch.no_grad():
        cond, shape = whole_scan_latent(ns.condition, patch, autoencoder, inferer.scale_factor, device)
    roi = [p // f for p in patch]
    out_dir = Path(ns.output_dir)
    pair = metric_volumes(ns.condition, patch, f, device, whole=True) if ns.metrics else None
    if getattr(scheduler, "use_timestep_transform", False):      # rectified flow: the transform sees the whole latent's size
        scheduler = make_scheduler(ns, list(cond.shape[2:]))
    with torch.no_grad():                                        # --init-from-condition: the whole scan's latent is the start, noised once
        warm, warm_rec = warm_start(ns, inferer, unet, scheduler, cond, roi_size=roi, overlap=ns.sw_overlap,
                                    sw_batch_size=ns.sw_batch or None, sw_mode=ns.sw_mode)
    inp, inp_rec, paste = inpaint_setup(ns, autoencoder, inferer, scheduler, device, whole=True)
    warm = dict(warm, **inp)
    for idx in parallel.shard_indices(ns.num, rank, world):
        z = torch.randn([1, autoencoder.latent_channels] + list(cond.shape[2:]), dtype=torch.float32).to(device)
        t0 = time.perf_counter()
        with torch.no_grad():
            vol = inferer.sample_sliding_window(z, autoencoder, unet, roi, overlap=ns.sw_overlap, sw_batch_size=ns.sw_batch or None,
                                                mode=ns.sw_mode, conditioning=cond, scheduler=scheduler, fused_seed=ns.seed + idx,
                                                cfg=ns.cfg, cfg_fill_value=ns.cfg_fill_value, **warm)
        torch.cuda.synchronize()
        scan = vol[:, :, :shape[0], :shape[1], :shape[2]]          # the scan's own shape: a strided view of the padded volume
        scan = inpaint_paste(ns, scan, paste)
        vol = scan[0, 0]
        stem = out_dir / time.strftime(f"synimg_%Y%m%d_%H%M%S_r{rank}_{idx}")
        written = save_nifti(vol.unsqueeze(-1).cpu().numpy(), str(stem))
        write_warm_record(out_dir, written, warm_rec)
        write_inpaint_record(out_dir, written, inp_rec)
        if pair is not None:
            write_metrics(out_dir, written, scan, *pair, extra=dict(warm_rec, **inp_rec))
        log.info("rank %d: %s %s (latent %s, windows of %s) in %.2f s", rank, written, tuple(vol.shape), tuple(cond.shape[2:]),
                 tuple(roi), time.perf_counter() - t0)


def sample_ensemble(ns, autoencoder, unet, inferer, scheduler, device):
    """--ensemble K: K draws of the --condition scan (its central patch, or the whole scan with --sliding-window) reduced on the device
    to a mean and a standard-deviation volume (LatentDiffusionInferer.sample_ensemble); one record in output_dir/ensemble.jsonl."""
    import torch
    from ldm3d.ensemble import default_member_batch
    from ldm3d.metrics import image_metrics
    from ldm3d.nifti import save_nifti
    patch = [int(p) for p in ns.diffusion_train["patch_size"]]
    f = autoencoder.factor
    whole = bool(ns.sliding_window)
    with torch.no_grad():
        if whole:
            cond, shape = whole_scan_latent(ns.condition, patch, autoencoder, inferer.scale_factor, device)
        else:
            cond, shape = condition_latent(ns.condition, patch, autoencoder, inferer.scale_factor, device), None
    spatial = list(cond.shape[2:])
    if getattr(scheduler, "use_timestep_transform", False):      # rectified flow: the transform sees the size of the latent sampled
        scheduler = make_scheduler(ns, spatial)
    K = ns.ensemble
    if whole:
        batch, kw = 1, dict(roi_size=[p // f for p in patch], overlap=ns.sw_overlap, sw_batch_size=ns.sw_batch or None, sw_mode=ns.sw_mode,
                            output_crop=shape)
    else:
        batch = ns.ensemble_batch or default_member_batch(unet, K, spatial, device, guided=ns.cfg is not None)
        kw = dict(member_batch=batch)
    pair = metric_volumes(ns.condition, patch, f, device, whole=whole) if ns.metrics else None
    keep = max(ns.ensemble_keep, 1) if pair is not None else ns.ensemble_keep      # member 0 is scored next to the mean
    warm, warm_rec = warm_start(ns, inferer, unet, scheduler, cond)      # --init-from-condition: every member starts from the scan's latent
    inp, inp_rec, paste = inpaint_setup(ns, autoencoder, inferer, scheduler, device, whole=whole)      # --inpaint: every member keeps the same region
    warm = dict(warm, **inp)
    t0 = time.perf_counter()
    with torch.no_grad():
        res = inferer.sample_ensemble(K, [autoencoder.latent_channels] + spatial, autoencoder, unet, scheduler=scheduler, conditioning=cond,
                                      mode="concat", seed=ns.seed, cfg=ns.cfg, cfg_fill_value=ns.cfg_fill_value, keep_members=keep,
                                      target=None if pair is None else pair[1], ddof=1, **warm, **kw)
    torch.cuda.synchronize()
    if ns.inpaint and ns.inpaint_paste:                            # the pasted region is the same in every member: its spread is 0
        res = res._replace(mean=inpaint_paste(ns, res.mean, paste), std=inpaint_paste(ns, res.std, (torch.zeros_like(paste[0]), paste[1])),
                           members=None if res.members is None else inpaint_paste(ns, res.members, paste))
    out_dir = Path(ns.output_dir)
    stamp = time.strftime("%Y%m%d_%H%M%S")
    files = {"mean": save_nifti(res.mean[0, 0].unsqueeze(-1).cpu().numpy(), str(out_dir / f"ensemble_mean_{stamp}")),
             "std": save_nifti(res.std[0, 0].unsqueeze(-1).cpu().numpy(), str(out_dir / f"ensemble_std_{stamp}"))}
    members = [save_nifti(res.members[k, 0].unsqueeze(-1).cpu().numpy(), str(out_dir / f"ensemble_member{k}_{stamp}"))
               for k in range(ns.ensemble_keep)]
    rec = {"members": res.count, "member_batch": batch, "seed": ns.seed, "sampler": ns.sampler, "steps": len(scheduler.timesteps), "ddof": 1,
           "shape": [int(d) for d in res.mean.shape[2:]],
           "mean_std": res.stats["mean_std"], "max_std": res.stats["max_std"], "mean_var": res.stats["mean_var"],
           "files": {"mean": os.path.basename(str(files["mean"])), "std": os.path.basename(str(files["std"])),
                     "members": [os.path.basename(str(m)) for m in members]}}
    rec.update(warm_rec)                                         # unet_calls: per member
    rec.update(inp_rec)                                          # n_calls: per member
    write_inpaint_record(out_dir, files["mean"], inp_rec)
    if pair is not None:
        image, label = pair
        rec["bias_sq"] = res.stats["bias_sq"]
        rec["mean_var_ddof0"] = res.stats["mean_var"] * (K - 1) / K      # bias_sq + mean_var_ddof0 = the members' mean MSE
        rec["image_metrics"] = {}
        for name, vol in (("mean", res.mean), ("member0", res.members[0:1]), ("input", image)):
            m = image_metrics(vol, label, **SSIM_SETTINGS)
            rec["image_metrics"][name] = {k: float(m[k][0]) for k in METRIC_NAMES}
        rec["ssim_settings"] = dict(SSIM_SETTINGS)
    with open(out_dir / "ensemble.jsonl", "a") as fh:
        fh.write(json.dumps(rec) + "\n")
    log.info("ensemble of %d (batch %d): %s in %.2f s", K, batch, rec, time.perf_counter() - t0)
    return rec


def score_likelihood(ns, autoencoder, unet, inferer, device, cond, rank, world):
    """--likelihood: the pair's high-count volume (cropped and scaled as ``metric_volumes`` does) scored under the model given the
    low-count latent ``cond`` (None: an unconditional UNet), once per noise draw (seed + idx, the device-resident loop); one JSON
    record per draw in output_dir/likelihood.jsonl, with --likelihood-map the per-voxel map as NIfTI."""
    import math
    import torch
    from ldm3d import parallel
    from ldm3d.inferer import resize_nearest
    from ldm3d.nifti import save_nifti
    from ldm3d.schedulers import DDPMScheduler
    cfg = ns.NoiseScheduler
    scheduler = DDPMScheduler(num_train_timesteps=cfg["num_train_timesteps"], schedule="scaled_linear_beta", beta_start=cfg["beta_start"],
                              beta_end=cfg["beta_end"], prediction_type=cfg.get("prediction_type", "epsilon"))
    if ns.steps:
        scheduler.set_timesteps(ns.steps)
    patch = [int(p) for p in ns.diffusion_train["patch_size"]]
    _, label = metric_volumes(ns.condition, patch, autoencoder.factor, device, whole=False)
    out_dir = Path(ns.output_dir)
    ts = [int(t) for t in scheduler.timesteps.tolist()]
    recs = []
    for idx in parallel.shard_indices(ns.num, rank, world):
        seed = ns.seed + idx
        kw = {} if cond is None else dict(conditioning=cond, mode="concat")
        t0 = time.perf_counter()
        with torch.no_grad():
            res = inferer.get_likelihood(label, autoencoder, unet, scheduler=scheduler, save_intermediates=ns.likelihood_map, verbose=False,
                                         fused_seed=seed, return_terms=True, **kw)
        total, terms = res[0], res[-1]
        nll = float(total[0])
        rec = {"nll_nats_per_dim": nll, "bits_per_dim": nll / math.log(2.0),
               "t0_term": float(terms[ts.index(0), 0]) if 0 in ts else None, "timesteps": len(ts), "seed": seed,
               "latent_shape": [autoencoder.latent_channels] + [int(d) // autoencoder.factor for d in label.shape[2:]]}
        if ns.likelihood_map:
            lat = torch.stack([m.mean(dim=1, keepdim=True) for m in res[1]]).sum(dim=0).to(device)      # [1, 1, d, h, w]
            vol = resize_nearest(lat, label.shape[2:])
            rec["map"] = os.path.basename(str(save_nifti(vol[0, 0].unsqueeze(-1).cpu().numpy(),
                                                         str(out_dir / time.strftime(f"likelihood_%Y%m%d_%H%M%S_r{rank}_{idx}")))))
        with open(out_dir / "likelihood.jsonl", "a") as fh:
            fh.write(json.dumps(rec) + "\n")
        log.info("rank %d: likelihood %s in %.2f s", rank, rec, time.perf_counter() - t0)
        recs.append(rec)
    return recs


def main():
    ns = parse_cli()
    import torch
    from ldm3d import parallel
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.nifti import save_nifti

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        parallel.setup_ddp(rank, world)
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    torch.manual_seed(ns.seed + rank)

    autoencoder, unet = load_networks(ns, device)
    unets = [unet]
    for _ in range(1, max(1, ns.chains)):                          # every chain owns its module instance (workspace + launch graph)
        unets.append(load_networks(ns, device, only_unet=True, like=unet))
    if not ns.eager:
        for u in unets:
            u.enable_graph_replay(True)
    scheduler = make_scheduler(ns)
    inferer = LatentDiffusionInferer(scheduler, scale_factor=resolve_scale_factor(ns))
    out_dir = Path(ns.output_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    patch = [int(p) for p in ns.diffusion_train["patch_size"]]
    cond = None
    if ns.ensemble:
        if unet.in_channels != 2 * autoencoder.latent_channels:
            raise SystemExit(f"--condition needs a concat-conditioned UNet (in_channels {2 * autoencoder.latent_channels}), got {unet.in_channels}")
        sample_ensemble(ns, autoencoder, unet, inferer, scheduler, device)
        return
    if ns.sliding_window:
        if unet.in_channels != 2 * autoencoder.latent_channels:
            raise SystemExit(f"--condition needs a concat-conditioned UNet (in_channels {2 * autoencoder.latent_channels}), got {unet.in_channels}")
        sample_whole_scans(ns, autoencoder, unet, inferer, scheduler, device, rank, world)
        if world > 1:
            parallel.cleanup_ddp()
        return
    if ns.likelihood:
        if unet.in_channels == 2 * autoencoder.latent_channels:
            with torch.no_grad():
                cond = condition_latent(ns.condition, patch, autoencoder, inferer.scale_factor, device)
        elif unet.in_channels != unet.out_channels:
            raise SystemExit(f"--likelihood: a UNet of in_channels {unet.in_channels} is neither unconditional nor concat-conditioned")
        score_likelihood(ns, autoencoder, unet, inferer, device, cond, rank, world)
        if world > 1:
            parallel.cleanup_ddp()
        return
    if ns.condition:
        with torch.no_grad():
            cond = condition_latent(ns.condition, patch, autoencoder, inferer.scale_factor, device)
        if getattr(scheduler, "use_timestep_transform", False):  # rectified flow: the transform sees the size of the latent sampled
            scheduler = inferer.scheduler = make_scheduler(ns, list(cond.shape[2:]))
        if unet.in_channels != 2 * autoencoder.latent_channels:
            raise SystemExit(f"--condition needs a concat-conditioned UNet (in_channels {2 * autoencoder.latent_channels}), got {unet.in_channels}")
    elif unet.in_channels != unet.out_channels:
        raise SystemExit(f"this UNet is concat-conditioned (in_channels {unet.in_channels}, out_channels {unet.out_channels}): pass --condition FILE")
    lat_ch = autoencoder.latent_channels if cond is not None else unet.in_channels
    pair = metric_volumes(ns.condition, patch, autoencoder.factor, device, whole=False) if ns.metrics else None
    with torch.no_grad():                                        # --init-from-condition: the condition latent is also the chains' start
        warm, warm_rec = warm_start(ns, inferer, unet, scheduler, cond)
    inp, inp_rec, paste = inpaint_setup(ns, autoencoder, inferer, scheduler, device, whole=False)
    measurement = None
    if ns.data_consistency:                                      # the target: the condition latent's means over K^3 cubes, pooled once
        from ldm3d.guidance import ConsistencyGuidance
        k = ns.data_consistency
        if any(d % k for d in cond.shape[2:]):
            raise SystemExit(f"--data-consistency {k} does not divide the latent dims {tuple(cond.shape[2:])}")
        target = cond if k == 1 else torch.nn.functional.avg_pool3d(cond, k)
        measurement = ConsistencyGuidance(target, pool=k, scale=ns.dc_scale, normalize=not ns.dc_no_normalize)
    if ns.data_consistency_image:                                # the target: the low-count volume's means over K^3 image cubes, pooled once
        from ldm3d.guidance import ImageConsistencyGuidance
        k = ns.data_consistency_image
        import numpy as np                                       # the very volume condition_latent encodes
        low = torch.from_numpy(np.ascontiguousarray(prepared_patch(ns.condition, patch, autoencoder.factor)))[None, None].to(device)
        if any(d % k for d in low.shape[2:]):
            raise SystemExit(f"--data-consistency-image {k} does not divide the image dims {tuple(low.shape[2:])}")
        target = low if k == 1 else torch.nn.functional.avg_pool3d(low, k)
        measurement = ImageConsistencyGuidance(target, pool=k, scale=ns.dc_scale, normalize=not ns.dc_no_normalize)
    todo = list(parallel.shard_indices(ns.num, rank, world))
    bsz, nch = max(1, ns.batch), max(1, ns.chains)
    for lo in range(0, len(todo), bsz * nch):                     # one round = up to `chains` batches of up to `batch` volumes
        groups = [todo[g:g + bsz] for g in range(lo, min(lo + bsz * nch, len(todo)), bsz)]
        spatial = list(cond.shape[2:]) if cond is not None else [p // autoencoder.factor for p in patch]
        zs = [torch.randn([len(ids), lat_ch] + spatial, dtype=torch.float32).to(device) for ids in groups]   # host draw then move, as the reference does
        cs = [None if cond is None else cond.expand(len(ids), -1, -1, -1, -1).contiguous() for ids in groups]
        t0 = time.perf_counter()
        with torch.no_grad():
            if len(groups) == 1:
                kw = {} if cond is None else dict(conditioning=cs[0], mode="concat")
                if ns.sampler in ("pndm", "rflow"):               # draws nothing: the device sampler's chain is the host loop's, bit for bit
                    kw["fused_seed"] = ns.seed
                if ns.sampler == "dpm":                           # the device sampler: the ODE form draws nothing, the SDE form per batch
                    kw["fused_seed"] = ns.seed + (groups[0][0] if ns.dpm_sde else 0)
                if ns.cfg is not None:
                    kw.update(cfg=ns.cfg, cfg_fill_value=ns.cfg_fill_value)
                kw.update(warm)                                   # the start noise of a warm chain is zs[0], the draw a full chain starts from
                if inp:                                           # the repaint chain runs on the device sampler, keyed per batch
                    kw.update(inp, fused_seed=ns.seed + groups[0][0])
                if measurement is not None:                       # the guided step runs on the device sampler, keyed per batch
                    kw.update(measurement=measurement, fused_seed=ns.seed + groups[0][0])
                vols = [inferer.sample(input_noise=zs[0], autoencoder_model=autoencoder, diffusion_model=unet, scheduler=scheduler, **kw)]
            else:
                vols = inferer.sample_concurrent(zs, autoencoder, unets, scheduler=scheduler, conditionings=cs,
                                                 mode="concat" if cond is not None else "crossattn")
        torch.cuda.synchronize()
        for ids, vol in zip(groups, vols):
            vol = inpaint_paste(ns, vol, paste)
            for j, idx in enumerate(ids):
                stem = out_dir / time.strftime(f"synimg_%Y%m%d_%H%M%S_r{rank}_{idx}")
                written = save_nifti(vol[j, 0].unsqueeze(-1).cpu().numpy(), str(stem))
                log.info("rank %d: %s %s", rank, written, tuple(vol.shape[1:]))
                write_warm_record(out_dir, written, warm_rec)
                write_inpaint_record(out_dir, written, inp_rec)
                dc_rec = {} if measurement is None else {"data_consistency": measurement.record(j)}
                if dc_rec:
                    with open(os.path.join(str(out_dir), "guidance.jsonl"), "a") as fh:
                        fh.write(json.dumps({"file": os.path.basename(str(written)), **dc_rec["data_consistency"]}) + "\n")
                if pair is not None:
                    write_metrics(out_dir, written, vol[j:j + 1], *pair, extra=dict(warm_rec, **inp_rec, **dc_rec))
        log.info("rank %d: %d volume(s) in %.2f s", rank, sum(len(g) for g in groups), time.perf_counter() - t0)
    if world > 1:
        parallel.cleanup_ddp()


if __name__ == "__main__":
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format="%(asctime)s %(levelname)s %(name)s: %(message)s")
    main()
