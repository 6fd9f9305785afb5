"""Ensemble statistics on the GPU (-m gpu): ldm_ensemble_update / ldm_ensemble_finalize against the fp64 restatement
(tests/ensemble_ref.py) under gates set by the fp32 CPU recurrence's own error, chunk invariance bit for bit, layout edges, the scalar
statistics, refusals, LatentDiffusionInferer.sample_ensemble against the members it is made of, and `inference.py --ensemble`."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import cfgs
import ensemble_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
BAD_ARG = -1                                                            # LDM_ERR_BAD_ARG, include/ldm3d.h
SIZES = [1, 3, 1003, 4 * 256 * 1024 + 5]                                # the last: every thread of the capped grid wraps, and a tail
ULP = 2.0 ** -24


def _update(members, mean, m2, count, n=None, stride=None):
    from ldm3d import _lib
    B = members.shape[0]
    n = members.shape[1] if n is None else n
    stride = (members.stride(0) if B > 1 else n) if stride is None else stride
    _lib.check(_lib.lib().ldm_ensemble_update(members.data_ptr(), B, stride, n, mean.data_ptr(), m2.data_ptr(), count, _lib.current_stream()))
    return count + B


def _fold(x, splits, dev):
    """x [K, n] on the device folded in chunks of `splits`; the state starts uninitialised"""
    mean, m2 = torch.empty((x.shape[1],), device=dev), torch.empty((x.shape[1],), device=dev)
    count, at = 0, 0
    for s in splits:
        count = _update(x[at:at + s], mean, m2, count)
        at += s
    assert at == x.shape[0] == count
    return mean, m2


def _finalize(mean, m2, count, ddof, target=None, want_std=True):
    from ldm3d import _lib
    L = _lib.lib()
    n = mean.numel()
    std = torch.empty_like(mean) if want_std else None
    stats = torch.full((8,), float("nan"), device=mean.device)
    scratch = torch.empty((L.ldm_ensemble_stats_scratch_bytes(n),), dtype=torch.uint8, device=mean.device)
    _lib.check(L.ldm_ensemble_finalize(mean.data_ptr(), m2.data_ptr(), count, ddof, _lib.ptr(target), _lib.ptr(std), stats.data_ptr(),
                                       scratch.data_ptr(), scratch.numel(), n, _lib.current_stream()))
    return std, stats


# ---- G1: accuracy against fp64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unit", "offset"])
@pytest.mark.parametrize("K", [1, 2, 5, 16])
@pytest.mark.parametrize("n", SIZES)
def test_update_matches_fp64_within_the_fp32_recurrence_error(cuda, n, K, name):
    """mean: |err| <= 2 x yardstick + 2 * 2^-24 * max|x|; m2: |err| <= 2 x yardstick + 2 * 2^-24 * max(m2_fp64), the yardstick being the fp32
    CPU recurrence's max-abs error against fp64 on the same inputs (an FMA or a reciprocal would reorder roundings, not add any).  The std
    map equals sqrt(max(m2, 0) / (K - ddof)) of the GPU's own m2 to rtol 2^-22.  K = 1 is bitwise."""
    x = ref.family(name, K, n, 1000 * K + n % 997)
    gate_mean, gate_m2, ym, ys, m64, s64 = ref.gates(x)
    mean, m2 = _fold(x.to(cuda), [K], cuda)
    em = float((mean.cpu().double() - m64).abs().max())
    es = float((m2.cpu().double() - s64).abs().max())
    print(f"{name} n={n} K={K}: mean err {em:.3e} (yardstick {ym:.3e}, gate {gate_mean:.3e}); m2 err {es:.3e} (yardstick {ys:.3e}, gate {gate_m2:.3e})")
    assert em <= gate_mean and es <= gate_m2
    if K == 1:
        assert torch.equal(mean.cpu(), x[0]) and bool((m2 == 0).all())
    for ddof in (0, 1):
        if K - ddof < 1:
            continue
        std, _ = _finalize(mean, m2, K, ddof)
        want = (m2.cpu().double().clamp_min(0.0) / (K - ddof)).sqrt()
        assert bool(((std.cpu().double() - want).abs() <= 2.0 ** -22 * want).all()), ddof
        assert bool((std >= 0).all())


# ---- G2: chunk invariance --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1003, 4 * 256 * 1024 + 5])
def test_chunking_does_not_change_a_bit(cuda, n):
    x = ref.family("unit", 5, n, 7).to(cuda)
    want = _fold(x, [5], cuda)
    for splits in ([1, 1, 1, 1, 1], [2, 3], [4, 1]):
        got = _fold(x, splits, cuda)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), splits
    xo = torch.empty((5 * n + 1,), device=cuda)[1:].view(5, n)          # 4 bytes past a 16-byte boundary: the scalar path
    xo.copy_(x)
    got = _fold(xo, [2, 3], cuda)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- G3: layout edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 1003, 4100])
def test_layout_edges(cuda, n):
    K = 5
    x = ref.family("offset", K, n, 11).to(cuda)
    want = _fold(x, [2, 3], cuda)
    # state and members offset by one float
    xo = torch.empty((K * n + 1,), device=cuda)[1:].view(K, n)
    xo.copy_(x)
    mean, m2 = torch.empty((n + 1,), device=cuda)[1:], torch.empty((n + 1,), device=cuda)[1:]
    assert mean.data_ptr() % 16 == 4 and xo.data_ptr() % 16 == 4
    c = _update(xo[:2], mean, m2, 0)
    _update(xo[2:], mean, m2, c)
    assert torch.equal(mean, want[0]) and torch.equal(m2, want[1])
    # member_stride > n: the leading columns of a [K, n + 3] buffer (rows misaligned) and of a [K, n + 4 - n % 4 ...] aligned one
    for pad in (3, 8 - n % 4):
        wide = torch.full((K, n + pad), float("nan"), device=cuda)
        wide[:, :n] = x
        mean, m2 = torch.empty((n,), device=cuda), torch.empty((n,), device=cuda)
        c = _update(wide[:2, :n], mean, m2, 0, n=n, stride=n + pad)
        _update(wide[2:, :n], mean, m2, c, n=n, stride=n + pad)
        assert torch.equal(mean, want[0]) and torch.equal(m2, want[1]), pad
    # count == 0: the state is not read
    for fill in (float("nan"), 0.0):
        mean, m2 = torch.full((n,), fill, device=cuda), torch.full((n,), fill, device=cuda)
        c = _update(x[:2], mean, m2, 0)
        _update(x[2:], mean, m2, c)
        assert torch.equal(mean, want[0]) and torch.equal(m2, want[1]), fill


def test_accumulator_takes_strided_members_and_resets(cuda):
    from ldm3d import _lib
    from ldm3d.ensemble import EnsembleAccumulator
    x = ref.family("unit", 4, 6 * 5 * 7, 5).to(cuda)
    acc = EnsembleAccumulator((6, 5, 7), cuda)
    with pytest.raises(ValueError):
        acc.mean()
    acc.update(x[:1].view(1, 6, 5, 7))
    acc.update(x[1:].view(3, 6, 5, 7))
    want = _fold(x, [4], cuda)
    assert acc.count == 4 and torch.equal(acc.mean().reshape(-1), want[0]) and torch.equal(acc.m2().reshape(-1), want[1])
    std1, _ = _finalize(want[0], want[1], 4, 1)
    assert torch.equal(acc.std().reshape(-1), std1)
    wide = torch.zeros((4, 6 * 5 * 7 + 2), device=cuda)
    wide[:, :210] = x
    acc.reset()
    assert acc.count == 0
    acc.update(wide[:, :210].unflatten(1, (6, 5, 7)))                    # rows contiguous, 212 floats apart: passed with its stride
    assert torch.equal(acc.mean().reshape(-1), want[0])
    with pytest.raises(ValueError):
        acc.update(torch.zeros((4, 6, 5, 14), device=cuda)[..., ::2])    # a member that is not contiguous
    with pytest.raises(ValueError):
        acc.update(x.view(4, 6, 7, 5))                                   # another shape
    with pytest.raises(_lib.LdmError):
        acc.update(x.cpu().view(4, 6, 5, 7))
    with pytest.raises(_lib.LdmError):
        acc.update(x[:1].view(1, 6, 5, 7).expand(2, 6, 5, 7))           # stride 0 < n: refused by the library


# ---- G4: the scalars -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 1003, 4 * 256 * 1024 + 5])
def test_stats_match_fp64_and_repeat_bit_for_bit(cuda, n):
    """The reductions against fp64 sums over the GPU's own state: rtol 1e-5 (double partials) with a floor of 1e-7, the gate of
    test_gpu_metrics.py's scalar reductions; max_std is the std map's maximum exactly; a second run gives the same bits."""
    K = 5
    x = ref.family("unit", K, n, 21)
    y = ref.family("unit", 1, n, 22)[0]
    mean, m2 = _fold(x.to(cuda), [K], cuda)
    for ddof in (0, 1):
        std, stats = _finalize(mean, m2, K, ddof, target=y.to(cuda))
        std2, stats2 = _finalize(mean, m2, K, ddof, target=y.to(cuda))
        assert torch.equal(stats, stats2) and torch.equal(std, std2)
        want = ref.stats(mean.cpu(), m2.cpu(), K, ddof, target=y)
        got = dict(zip(("mean_std", "max_std", "mean_var", "bias_sq"), stats.tolist()))
        print(f"n={n} ddof={ddof}: got {got}, fp64 {want}")
        for k in ("mean_std", "mean_var", "bias_sq"):
            assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]) + 1e-7, (k, got[k], want[k])
        assert got["max_std"] == float(std.max())
        assert stats.tolist()[4:] == [0.0] * 4
        _, nostd = _finalize(mean, m2, K, ddof, target=y.to(cuda), want_std=False)
        assert torch.equal(nostd, stats)
        _, notgt = _finalize(mean, m2, K, ddof)
        assert notgt.tolist()[3] == 0.0 and torch.equal(notgt[:3], stats[:3])


def test_non_finite_members_reach_the_maps_and_the_scalars(cuda):
    x = ref.family("unit", 3, 1003, 4)
    x[1, 17] = float("nan")
    x[2, 500] = float("inf")
    mean, m2 = _fold(x.to(cuda), [3], cuda)
    std, stats = _finalize(mean, m2, 3, 1)
    bad = torch.zeros((1003,), dtype=torch.bool)
    bad[17] = bad[500] = True
    assert torch.equal(~torch.isfinite(mean.cpu()), bad) and torch.equal(~torch.isfinite(std.cpu()), bad)
    assert not any(v == v and abs(v) != float("inf") for v in stats.tolist()[:3]), stats.tolist()


def test_decomposition_identity_against_image_metrics(cuda):
    """mean over the members of image_metrics' MSE against the target == bias_sq + mean_var(ddof = 0), rtol 1e-4"""
    from ldm3d.ensemble import EnsembleAccumulator
    from ldm3d.metrics import image_metrics
    K, shape = 5, (1, 12, 13, 14)
    n = 12 * 13 * 14
    x = ref.family("unit", K, n, 31).to(cuda).view((K,) + shape)
    y = ref.family("unit", 1, n, 32).to(cuda).view((1,) + shape)
    acc = EnsembleAccumulator(shape, cuda)
    acc.update(x[:2])
    acc.update(x[2:])
    s = acc.stats(target=y, ddof=0)
    mse = sum(float(image_metrics(x[k:k + 1], y)["mse"][0]) for k in range(K)) / K
    print(f"members' mean MSE {mse:.8e}, bias_sq + mean_var {s['bias_sq'] + s['mean_var']:.8e}")
    assert abs(mse - (s["bias_sq"] + s["mean_var"])) <= 1e-4 * mse
    assert set(s) == {"mean_std", "max_std", "mean_var", "bias_sq"} and all(isinstance(v, float) for v in s.values())


# ---- G5: refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(cuda, built_lib):
    from ldm3d import _lib
    L = built_lib
    n, B = 1003, 3
    S = -7.0
    buf = torch.full((B * n + 2 * n,), S, device=cuda)
    members = torch.rand((B, n), device=cuda)
    mean, m2 = torch.full((n,), S, device=cuda), torch.full((n,), S, device=cuda)
    std, stats = torch.full((n,), S, device=cuda), torch.full((8,), S, device=cuda)
    scratch = torch.empty((L.ldm_ensemble_stats_scratch_bytes(n),), dtype=torch.uint8, device=cuda)
    assert scratch.numel() > 0 and L.ldm_ensemble_stats_scratch_bytes(0) == 0
    st = _lib.current_stream()
    P = lambda t: t.data_ptr()

    def upd(mem=P(members), B=B, stride=n, n=n, mean=P(mean), m2=P(m2), count=0):
        return L.ldm_ensemble_update(mem, B, stride, n, mean, m2, count, st)

    def fin(mean=P(mean), m2=P(m2), count=3, ddof=1, target=None, std=P(std), stats=P(stats), scr=P(scratch), nbytes=scratch.numel(), n=n):
        return L.ldm_ensemble_finalize(mean, m2, count, ddof, target, std, stats, scr, nbytes, n, st)

    inside = buf[n:n + B * n]                                            # a members range with the state arrays laid over its two ends
    refused = [upd(mem=None), upd(mean=None), upd(m2=None), upd(B=0), upd(n=0), upd(count=-1), upd(count=2 ** 31 - 2), upd(stride=n - 1),
               upd(mem=P(inside), mean=P(buf[1:])), upd(mem=P(inside), m2=P(buf[n + B * n - 1:])), upd(mem=P(inside), mean=P(inside[n:])),
               fin(mean=None), fin(m2=None), fin(stats=None), fin(scr=None), fin(n=0), fin(count=1, ddof=1), fin(count=0, ddof=0),
               fin(ddof=2), fin(ddof=-1), fin(nbytes=scratch.numel() - 1)]
    for k, r in enumerate(refused):
        assert r == BAD_ARG, (k, r)
        with pytest.raises(_lib.LdmError):
            _lib.check(r)
    torch.cuda.synchronize()
    for t in (buf, mean, m2, std, stats):
        assert bool((t == S).all())
    assert upd() == 0 and fin() == 0                                      # the same buffers, accepted
    torch.cuda.synchronize()
    assert bool(torch.isfinite(stats).all()) and bool((std >= 0).all())


# ---- G6: sample_ensemble == the members it is made of ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _models():
    from ldm3d.networks import AutoencoderKL, DiffusionModelUNet
    from oracle import autoencoder as oa
    from oracle import unet as ou
    dev = torch.device("cuda:0")
    m = DiffusionModelUNet(**cfgs.UNET_TINY_COND)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfgs.UNET_TINY_COND), 3))
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith("out.2.conv."):                           # a random-weight UNet under large steps: keep the chain tame
                p.mul_(0.1)
    m = m.to(dev).eval()
    m.set_precision("fp32")
    vcfg = dict(cfgs.VAE_TINY, in_channels=1, out_channels=1, latent_channels=4)
    v = AutoencoderKL(**vcfg)
    v.load_state_dict(ou.init_state_dict(oa.ae_param_shapes(vcfg), 2))
    v = v.to(dev).eval()
    v.set_precision("fp32")
    return m, v


def _scheduler(kind):
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler
    if kind == "ddpm":
        return DDPMScheduler(**dict(cfgs.SCHED, num_train_timesteps=3))
    sch = DDIMScheduler(**cfgs.SCHED)
    sch.set_timesteps(3)
    return sch


K6, SEED6 = 4, 40


@functools.lru_cache(maxsize=None)
def _direct_members(kind, member_batch, cfg, latent):
    """The K volumes from direct inferer.sample / sample_sliding_window calls: the same start noises, seeds and chunking."""
    from ldm3d.ensemble import plan_chunks
    from ldm3d.inferer import LatentDiffusionInferer
    m, v = _models()
    dev = torch.device("cuda:0")
    inf = LatentDiffusionInferer(_scheduler(kind))
    cond = torch.randn((1, 4) + latent, generator=torch.Generator().manual_seed(5)).to(dev)
    vols = []
    with torch.no_grad():
        for first, nb in plan_chunks(K6, member_batch):
            z = torch.stack([torch.randn((4,) + latent, generator=torch.Generator().manual_seed(SEED6 + first + j)) for j in range(nb)]).to(dev)
            if latent != (8, 8, 8):
                vols.append(inf.sample_sliding_window(z, v, m, (8, 8, 8), conditioning=cond, fused_seed=SEED6 + first, cfg=cfg))
            else:
                vols.append(inf.sample(z, v, m, conditioning=cond.expand(nb, -1, -1, -1, -1).contiguous(), mode="concat",
                                       fused_seed=SEED6 + first, cfg=cfg))
    return inf, cond, torch.cat(vols)


def _check_maps(res, vols, ddof, what):
    """G1's gates on the maps; the std map carries the rounding of its division and square root on top (each at most 2^-24 relative,
    doubled by squaring it back to an m2): 4 * 2^-24 * max(m2_fp64) more."""
    K = vols.shape[0]
    x = vols.reshape(K, -1).cpu()
    gate_mean, gate_m2, ym, ys, m64, s64 = ref.gates(x)
    em = float((res.mean.reshape(-1).cpu().double() - m64).abs().max())
    m2_got = res.std.reshape(-1).cpu().double() ** 2 * (K - ddof)
    es = float((m2_got - s64).abs().max())
    gate_std = gate_m2 + 4 * ULP * float(s64.max())
    print(f"{what}: mean err {em:.3e} (gate {gate_mean:.3e}), m2-from-std err {es:.3e} (gate {gate_std:.3e}), max|x| {float(x.abs().max()):.3f}")
    assert res.count == K and torch.isfinite(res.mean).all() and float(res.std.max()) > 0
    assert em <= gate_mean and es <= gate_std
    want = ref.stats(m64, s64, K, ddof)
    for k in ("mean_std", "mean_var"):
        assert abs(res.stats[k] - want[k]) <= 1e-4 * abs(want[k]) + 1e-7, (k, res.stats[k], want[k])


@pytest.mark.parametrize("kind,member_batch,cfg", [("ddim", 1, None), ("ddim", 2, None), ("ddim", 4, None), ("ddim", 2, 2.0), ("ddpm", 2, None)])
def test_sample_ensemble_equals_its_members(cuda, kind, member_batch, cfg):
    m, v = _models()
    inf, cond, vols = _direct_members(kind, member_batch, cfg, (8, 8, 8))
    assert tuple(vols.shape) == (K6, 1, 32, 32, 32) and not torch.equal(vols[0], vols[1])
    with torch.no_grad():
        res = inf.sample_ensemble(K6, (4, 8, 8, 8), v, m, conditioning=cond, member_batch=member_batch, seed=SEED6, cfg=cfg, keep_members=2)
    _check_maps(res, vols, 1, f"{kind} member_batch={member_batch} cfg={cfg}")
    assert tuple(res.mean.shape) == tuple(res.std.shape) == (1, 1, 32, 32, 32)
    assert tuple(res.members.shape) == (2, 1, 32, 32, 32) and torch.equal(res.members, vols[:2])


def test_sample_ensemble_crop_target_and_ddof(cuda):
    m, v = _models()
    inf, cond, vols = _direct_members("ddim", 2, None, (8, 8, 8))
    crop = (20, 32, 17)
    cropped = vols[:, :, :20, :32, :17].contiguous()
    target = torch.rand((1, 1) + crop, generator=torch.Generator().manual_seed(9)).to(cuda)
    with torch.no_grad():
        res = inf.sample_ensemble(K6, (4, 8, 8, 8), v, m, conditioning=cond, member_batch=2, seed=SEED6, output_crop=crop, target=target, ddof=0)
    assert tuple(res.mean.shape) == (1, 1) + crop and res.members is None
    _check_maps(res, cropped, 0, "crop (20, 32, 17), ddof 0")
    mse = float(((cropped.double() - target.double()) ** 2).mean())
    assert abs(res.stats["bias_sq"] + res.stats["mean_var"] - mse) <= 1e-4 * mse
    with pytest.raises(ValueError):
        inf.sample_ensemble(1, (4, 8, 8, 8), v, m, conditioning=cond)
    with pytest.raises(ValueError):
        inf.sample_ensemble(4, (4, 8, 8, 8), v, m, cfg=2.0)              # _check_cfg: guidance needs a condition
    with pytest.raises(ValueError):
        inf.sample_ensemble(4, (4, 12, 8, 8), v, m, conditioning=torch.zeros((1, 4, 12, 8, 8), device=cuda), roi_size=(8, 8, 8), member_batch=2)


def test_sample_ensemble_of_whole_scans(cuda):
    """roi_size: a 12 x 8 x 8 latent in 8^3 windows, every member one sample_sliding_window chain"""
    m, v = _models()
    inf, cond, vols = _direct_members("ddim", 1, None, (12, 8, 8))
    assert tuple(vols.shape) == (K6, 1, 48, 32, 32)
    with torch.no_grad():
        res = inf.sample_ensemble(K6, (4, 12, 8, 8), v, m, conditioning=cond, seed=SEED6, roi_size=(8, 8, 8), keep_members=1)
    _check_maps(res, vols, 1, "whole scan 12x8x8")
    assert torch.equal(res.members[0], vols[0])


# ---- G7: the command line --------------------------------------------------------------------------------------------------------
def _nii(path, shape):
    """the voxels of a NIfTI-1 file written by ldm3d.nifti (x fastest), flattened in C order of `shape`"""
    import numpy as np
    data = np.fromfile(path, dtype=np.float32, offset=352)
    assert data.size == shape[0] * shape[1] * shape[2], (path, data.size, shape)
    return np.ascontiguousarray(data.reshape(shape, order="F")).reshape(-1)


@pytest.mark.parametrize("whole", [False, True])
def test_inference_cli_ensemble(tmp_path, whole):
    import numpy as np
    from ldm3d.data import write_synthetic_pairs
    shape = (100, 96, 120)
    pair = write_synthetic_pairs(str(tmp_path / "pairs"), 1, shape)[0]
    env = {"npz_dir": str(tmp_path / "pairs"), "model_dir": str(tmp_path / "ckpt"), "output_dir": str(tmp_path / "out"),
           "tfevent_path": str(tmp_path / "tfevent"), "resume_ckpt": False, "seed": 0}
    env_file = str(tmp_path / "environment.json")
    with open(env_file, "w") as fh:
        json.dump(env, fh)
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-e", env_file, "-c", os.path.join(ROOT, "config", "config_synthetic_train.json"),
           "--random-init", "--steps", "2", "--condition", pair]
    cmd += ["--ensemble", "2", "--sliding-window"] if whole else ["--ensemble", "3", "--ensemble-batch", "2", "--ensemble-keep", "1", "--metrics"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = tmp_path / "out"
    recs = [json.loads(l) for l in open(out / "ensemble.jsonl")]
    assert len(recs) == 1
    rec = recs[0]
    K = 2 if whole else 3
    vox = shape if whole else (96, 96, 96)
    assert rec["members"] == K and rec["member_batch"] == (1 if whole else 2) and rec["steps"] == 2 and rec["ddof"] == 1 and rec["seed"] == 0      # the environment file's seed
    assert rec["sampler"] == "auto" and rec["shape"] == (list(shape) if whole else [96, 96, 96])
    for k in ("mean_std", "max_std", "mean_var"):
        assert isinstance(rec[k], float) and rec[k] == rec[k] and 0 < rec[k] < float("inf"), (k, rec[k])
    mean = _nii(out / rec["files"]["mean"], vox)
    std = _nii(out / rec["files"]["std"], vox)
    assert rec["files"]["mean"].startswith("ensemble_mean_") and rec["files"]["std"].startswith("ensemble_std_")
    assert np.isfinite(mean).all() and np.isfinite(std).all() and (std >= 0).all() and std.max() > 0
    assert abs(float(std.astype(np.float64).mean()) - rec["mean_std"]) <= 1e-5 * rec["mean_std"] and float(std.max()) == rec["max_std"]
    assert len(list(out.glob("synimg_*"))) == 0
    if whole:
        assert rec["files"]["members"] == [] and "bias_sq" not in rec
        return
    assert len(rec["files"]["members"]) == 1 and rec["files"]["members"][0].startswith("ensemble_member0_")
    member0 = _nii(out / rec["files"]["members"][0], vox)
    for name in ("mean", "member0", "input"):
        assert sorted(rec["image_metrics"][name]) == sorted(("ssim", "psnr", "mse", "mae", "nrmse")), name
    # bias_sq + mean_var_ddof0 is the members' mean MSE; from the files: the label, the written mean and std maps
    from ldm3d.data import crop, crop_start, load_pair, scale_percentiles
    raw = load_pair(pair)[1]
    lab = scale_percentiles(crop(raw, crop_start(raw.shape, [96, 96, 96], None), [96, 96, 96])).astype(np.float64).reshape(-1)
    bias = float(((mean.astype(np.float64) - lab) ** 2).mean())
    var0 = float((std.astype(np.float64) ** 2).mean()) * (K - 1) / K
    assert abs(rec["bias_sq"] - bias) <= 1e-4 * bias and abs(rec["mean_var_ddof0"] - var0) <= 1e-4 * var0
    assert abs(rec["bias_sq"] + rec["mean_var_ddof0"] - (bias + var0)) <= 1e-4 * (bias + var0)
    mse0 = float(((member0.astype(np.float64) - lab) ** 2).mean())           # the kept member's own MSE, as image_metrics scored it
    assert abs(rec["image_metrics"]["member0"]["mse"] - mse0) <= 1e-4 * mse0
    assert abs(rec["image_metrics"]["mean"]["mse"] - bias) <= 1e-4 * bias
