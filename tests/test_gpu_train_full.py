"""The full-width training plans, gradient by gradient (-m gpu): the benchmark UNet at 1x4x24^3 (bench.py's train_step_24cube),
the configs[3] concat-conditioned UNet at the 36x44x28 latent, and AutoencoderKL training at 64^3 and 48^3
(tools/bench_train_vae.py) -- the shapes at which the planner's shape-dependent choices (wgrad_ksplit > 1 and grad_export's fold over
split copies, the wgrad_pair forms, gnb_fold_chunks, gn8_slabs, the batched descriptor tables at their full counts, the unsplit halo /
block convolutions) are the ones that are trained and timed.  The oracle is too slow to run here at these sizes, so the checker is the
committed fixtures of tests/golden/make_golden.py (torch autograd through the CPU oracle, fp32 and bf16-emulating; format and comparer
in tests/train_full_ref.py): every parameter tensor's gradient is compared on 256 seeded elements and in norm, so a wrong offset in
one export descriptor -- finite, non-zero garbage in one tensor -- fails on that tensor.

bf16 mode gates each tensor at 2.5 x its own bf16-vs-fp32 oracle floor + 5e-3 (the per-family form of tests/test_gpu_train.py, per
tensor; the factor covers the spread of a sampled rel-L2 around the whole-tensor figure: 0.53 - 1.33 x over 128 indices, 0.81 - 1.24 x over 512), fp32 mode at the 1e-3 global /
2e-3 worst-tensor bars of the fp32-mode gradient tests.  The attention key biases have a true gradient of zero (a key bias shifts every
logit of a softmax row equally): they are the only tensors left out of the relative gates, their count is asserted, and their norm is
bounded by the bf16-emulating oracle's own rounding noise in the same tensor.  Measured figures: profiles/train_full_errors_vs_oracle.txt."""
import os

import pytest
import torch
import torch.nn.functional as F

import train_full_ref as tf

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# Norm of a key-bias gradient (true value zero) over the bf16-emulating oracle's norm of the same tensor.  The oracle rounds to bf16 in
# the forward only (autograd differentiates through its rounding points in fp32), the HIP attention backward feeds dS to the matrix
# instruction as bf16 (csrc/attention.h), which breaks the exact sum_j dS_ij = 0 at the 2^-9 level: measured 5.2 - 15.0 over the 22 key
# biases of the two UNet cases, i.e. ~0.5 % of the to_q.bias gradient next to it (which is 1000 - 3000 x that noise, so a key bias that
# received another tensor's gradient fails).  fp32 mode: measured 4.3e-4 - 2.7e-3.  Bounds = measured maximum x 3.3 / x 7.4
# (profiles/train_full_errors_vs_oracle.txt).
ZERO_MARGIN = {"bf16": 50.0, "fp32": 0.02}
_cache = {}


def _case(case):
    """Fixture + seeded weights / inputs of one case, built once for both precision modes."""
    if case not in _cache:
        _cache.clear()                                        # one case's 191 M-parameter state dict at a time
        _cache[case] = (torch.load(os.path.join(HERE, "golden", case + ".pt"), weights_only=True), tf.case_inputs(case))
    return _cache[case]


def _report(case, mode, loss, fx, res, bad):
    ex = tf.exempt(fx)
    med, p90, mx, mxn = tf.floor_ratio_stats(res, fx)
    worst = max((e, n) for e, n in zip(res["err"], fx["names"]) if n not in ex)
    wnorm = max((abs(r - 1.0), n) for r, n in zip(res["norm_ratio"], fx["names"]) if n not in ex)
    zr = [g / nb for n, g, nb in zip(fx["names"], res["norm"], fx["norm_bf16"].tolist()) if n in ex]
    print(f"{case} {mode}: loss {loss:.6f} (fp32 oracle {fx['loss_fp32']:.6f}, bf16 oracle {fx['loss_bf16']:.6f}); gradients vs fp32 oracle "
          f"{res['e32']:.3e} (oracle's own bf16 floor {fx['global_floor_sampled']:.3e} on the samples, {fx['global_floor']:.3e} whole), cosine "
          f"{res['cos']:.6f}, |g| {res['total_norm']:.5f} / {fx['total_grad_norm_fp32']:.5f}; per-tensor error / floor median {med:.2f} p90 {p90:.2f} "
          f"max {mx:.2f} ({mxn}); worst tensor {worst[0]:.3e} ({worst[1]}), worst norm ratio off by {wnorm[0]:.3e} ({wnorm[1]}); "
          f"{len(ex)} key biases, |g| / oracle bf16 noise {' '.join(f'{v:.2e}' for v in zr) or '-'}; failing {bad}")


def _check(case, mode, loss, got, fx, kind):
    res = tf.compare(got, fx)
    bad = tf.failing_tensors(res, fx, mode, ZERO_MARGIN[mode])
    _report(case, mode, loss, fx, res, bad)
    assert len(tf.exempt(fx)) == (11 if kind == "unet" else 0)
    # bf16: 2e-3 as the committed tiny golden step has it.  fp32 mode: |d loss| / loss <= 2 |d out| / |out - target| for MSE (Cauchy-Schwarz),
    # <= |d out|_2 / (sqrt(N) mean|out - x|) for L1; with the project's 1e-4 output bar of the fp32 mode and |out| <~ |out - target| that is 2e-4
    tol = 2e-3 if mode == "bf16" else 2e-4
    assert abs(loss - fx["loss_fp32"]) <= tol * abs(fx["loss_fp32"]), (loss, fx["loss_fp32"])
    assert tf.global_ok(res, fx, mode, kind), (res["e32"], res["cos"], fx["global_floor_sampled"])
    assert bad == [], bad
    return res


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("case", ["train_step_full_24", "train_step_cfg3_latent"])
def test_full_width_unet_gradients_match_the_oracle_fixture(cuda, case, mode):
    from ldm3d.networks import DiffusionModelUNet
    from ldm3d.optim import FlatAdam
    fx, (cfg, sd, x, t, target) = _case(case)
    assert fx["torch_version"] and fx["names"] == list(sd.keys())
    m = DiffusionModelUNet(**cfg)
    m.load_state_dict(sd)
    m = m.to(cuda).train().set_precision(mode)
    opt = FlatAdam(m, lr=1e-3, max_grad_norm=1.0)
    xd, nc = x.to(cuda), cfg["in_channels"] - cfg["out_channels"]
    if nc:                                                    # mode="concat" of train_diffusion.py:197-205
        out = m(x=xd[:, :-nc].contiguous(), timesteps=t.to(cuda), cond=xd[:, -nc:].contiguous())
    else:
        out = m(x=xd, timesteps=t.to(cuda))
    loss = F.mse_loss(out.float(), target.to(cuda))
    loss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad for k, p in m.named_parameters()}
    _check(case, mode, float(loss.detach()), got, fx, "unet")
    if "param_abs_sum_after_adam_fp32" not in fx:
        return
    # one clipped Adam step, with the tolerances of test_training_step_matches_committed_golden
    total = float(opt.grad_norm())
    assert abs(total - fx["total_grad_norm_fp32"]) <= 2e-2 * fx["total_grad_norm_fp32"], (total, fx["total_grad_norm_fp32"])
    opt.step()
    torch.cuda.synchronize()
    s, sa = float(m.flat_params.double().sum()), float(m.flat_params.double().abs().sum())
    print(f"{case} {mode}: clip norm {total:.5f} / {fx['total_grad_norm_fp32']:.5f}; after Adam sum {s:.4f} / {fx['param_sum_after_adam_fp32']:.4f}, "
          f"abs sum {sa:.3f} / {fx['param_abs_sum_after_adam_fp32']:.3f}")
    assert abs(sa - fx["param_abs_sum_after_adam_fp32"]) <= 1e-4 * fx["param_abs_sum_after_adam_fp32"]
    assert abs(s - fx["param_sum_after_adam_fp32"]) <= 0.02 * m.flat_params.numel() * 1e-3 + 1e-3 * abs(fx["param_sum_after_adam_fp32"])


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("case", ["vae_train_step_full_64", "vae_train_step_full_48"])
def test_full_width_autoencoder_gradients_match_the_oracle_fixture(cuda, case, mode):
    from ldm3d.networks import AutoencoderKL
    from oracle import autoencoder as oa
    fx, (cfg, sd, x, eps) = _case(case)
    assert fx["names"] == list(sd.keys())
    m = AutoencoderKL(**cfg)
    m.load_state_dict(sd)
    m = m.to(cuda).train().set_precision(mode)
    recon, mu, sigma = m(x.to(cuda), eps=eps.to(cuda))
    loss = F.l1_loss(recon.float(), x.to(cuda)) + tf.KL_WEIGHT * oa.kl_loss(mu, sigma).mean()
    loss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad for k, p in m.named_parameters()}
    _check(case, mode, float(loss.detach()), got, fx, "vae")
