"""ldm_op_image_metrics (csrc/metrics.h) on the GPU, through the C ABI and through ldm3d.metrics, against the fp64 yardstick of
tests/metrics_ref.py.

Gates.  For every case |kernel - fp64| <= max(e32, 16 * 2^-24), where e32 is the error of the SAME formula evaluated naively in fp32
on the CPU (raw E[x^2] - mu^2) on the same inputs and the floor is 16 fp32 ulps of 1.0 (where the naive formula is itself at rounding
level, a different summation order must not fail).  On the nearly flat image the kernel must be strictly better than e32: that is
what the pivot is for.  mse / mae / nrmse / psnr: the same rule on relative errors.  Every figure is printed before it is asserted
(`pytest -s`); DESIGN.md section 3.9 quotes a run."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 16 * 2.0 ** -24
SCALARS = ("mse", "mae", "nrmse", "psnr")


def make_pair(content, shape, seed, data_range=1.0):
    """(x, y) fp32 CPU tensors [B, C, D, H, W]; x is the prediction."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(shape, generator=g, dtype=torch.float32)

    def smooth(v):                                                 # 5^3 box filter, same size
        B, Cn = v.shape[:2]
        v = F.avg_pool3d(F.pad(v.reshape(B * Cn, 1, *v.shape[2:]), (2, 2, 2, 2, 2, 2), mode="replicate"), 5, stride=1)
        return v.reshape(shape)
    if content == "noise":
        x, y = r(), r()
    elif content == "smooth":
        x, y = smooth(r()), smooth(r())
    elif content == "flat":
        x, y = 0.9 + 1e-3 * r(), 0.9 + 1e-3 * r()
    elif content == "noisy5":                                      # the denoising situation: x = y + 5 % Gaussian noise
        y = smooth(r())
        y = (y - y.min()) / (y.max() - y.min())
        x = y + 0.05 * torch.randn(shape, generator=g, dtype=torch.float32)
    elif content == "identical":
        y = smooth(r())
        x = y.clone()
    else:
        raise KeyError(content)
    return (x * data_range).contiguous(), (y * data_range).contiguous()


def run_kernel(x, y, dev, full=True, **kw):
    from ldm3d.metrics import image_metrics
    m = image_metrics(x.to(dev), y.to(dev), return_full_image=full, **kw)
    return {k: v.cpu() for k, v in m.items()}


def check_against_yardstick(tag, got, x, y, strict_ssim=False, **kw):
    """The gates of the module docstring; returns the naive fp32 formula's largest error on the map (None without a map)."""
    r64 = metrics_ref.metrics(x, y, dtype=torch.float64, **kw)
    r32 = metrics_ref.metrics(x, y, dtype=torch.float32, **kw)
    e32 = float((r32["ssim"].double() - r64["ssim"]).abs().max())
    err = float((got["ssim"].double() - r64["ssim"]).abs().max())
    m32 = None
    line = f"[metrics] {tag}: ssim {float(r64['ssim'][0]):.6f} kernel err {err:.3e} e32 {e32:.3e}"
    if "ssim_map" in got:
        assert got["ssim_map"].shape == r64["ssim_map"].shape, (got["ssim_map"].shape, r64["ssim_map"].shape)
        m32 = float((r32["ssim_map"].double() - r64["ssim_map"]).abs().max())
        merr = float((got["ssim_map"].double() - r64["ssim_map"]).abs().max())
        line += f" | map err {merr:.3e} e32 {m32:.3e}"
    rel = {}
    for k in SCALARS:
        den = r64[k].abs().clamp_min(1e-300)
        rel[k] = (float(((got[k].double() - r64[k]).abs() / den).max()), float(((r32[k].double() - r64[k]).abs() / den).max()))
        line += f" | {k} rel {rel[k][0]:.2e} e32 {rel[k][1]:.2e}"
    print(line)
    assert err <= max(e32, FLOOR), (tag, err, e32)
    if strict_ssim:
        assert err < e32, (tag, err, e32)
    if "ssim_map" in got:
        assert merr <= max(m32, FLOOR), (tag, merr, m32)
        if strict_ssim:
            assert merr < m32, (tag, merr, m32)
    for k in SCALARS:
        assert rel[k][0] <= max(rel[k][1], FLOOR), (tag, k, rel[k])
    return m32


CASES = [
    # tag, content, shape [B, C, D, H, W], kwargs
    ("11^3 single voxel", "noise", (1, 1, 11, 11, 11), {}),
    ("12x37x53 noise", "noise", (1, 1, 12, 37, 53), {}),
    ("24x40x56 noise", "noise", (1, 1, 24, 40, 56), {}),
    ("24x40x56 smooth", "smooth", (1, 1, 24, 40, 56), {}),
    ("24x40x56 noisy5", "noisy5", (1, 1, 24, 40, 56), {}),
    ("96^3 smooth", "smooth", (1, 1, 96, 96, 96), {}),
    ("96^3 noisy5", "noisy5", (1, 1, 96, 96, 96), {}),
    ("160x224x160 noisy5", "noisy5", (1, 1, 160, 224, 160), {}),
    ("B2 C2 12x37x53 smooth", "smooth", (2, 2, 12, 37, 53), {}),
    ("B2 C2 24x40x56 noisy5", "noisy5", (2, 2, 24, 40, 56), {}),
    ("win 7 24x40x56 smooth", "smooth", (1, 1, 24, 40, 56), dict(win_size=7)),
    ("win 3 12x37x53 noise", "noise", (1, 1, 12, 37, 53), dict(win_size=3)),
    ("uniform 24x40x56 noise", "noise", (1, 1, 24, 40, 56), dict(kernel_type="uniform")),
    ("uniform win 7 24x40x56 noisy5", "noisy5", (1, 1, 24, 40, 56), dict(kernel_type="uniform", win_size=7)),
    ("data_range 4 24x40x56 noisy5", "noisy5", (1, 1, 24, 40, 56), dict(data_range=4.0)),
    ("data_range 4 24x40x56 noise", "noise", (1, 1, 24, 40, 56), dict(data_range=4.0)),
]


@pytest.mark.parametrize("tag,content,shape,kw", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_metrics_match_the_fp64_yardstick(cuda, tag, content, shape, kw):
    x, y = make_pair(content, shape, seed=len(tag) + shape[2], data_range=kw.get("data_range", 1.0))
    got = run_kernel(x, y, cuda, **kw)
    check_against_yardstick(tag, got, x, y, **kw)


@pytest.mark.parametrize("shape", [(1, 1, 24, 40, 56), (1, 1, 96, 96, 96), (2, 2, 12, 37, 53)], ids=["24x40x56", "96^3", "B2C2_12x37x53"])
def test_nearly_flat_image_beats_the_naive_fp32_formula(cuda, shape):
    """0.9 + 1e-3 U: raw E[x^2] - mu^2 in fp32 loses the variance; the kernel's pivot must keep it (strictly below e32)."""
    x, y = make_pair("flat", shape, seed=5)
    got = run_kernel(x, y, cuda)
    m32 = check_against_yardstick(f"flat {shape}", got, x, y, strict_ssim=True)
    assert m32 > 100 * FLOOR, m32          # the case does show the cancellation it is here for: voxel by voxel (the errors have both signs and
                                           # mostly cancel in the mean), the naive formula is off by several 1e-4


@pytest.mark.parametrize("shape,kw", [((1, 1, 24, 40, 56), {}), ((2, 2, 12, 37, 53), dict(win_size=7)), ((1, 1, 11, 11, 11), {}),
                                      ((1, 1, 96, 96, 96), dict(kernel_type="uniform"))])
def test_identical_inputs_are_exact(cuda, shape, kw):
    x, y = make_pair("identical", shape, seed=9)
    got = run_kernel(x, y, cuda, **kw)
    assert torch.equal(got["ssim"], torch.ones(shape[0])), got["ssim"]
    assert torch.equal(got["ssim_map"], torch.ones_like(got["ssim_map"]))
    assert torch.equal(got["mse"], torch.zeros(shape[0])) and torch.equal(got["mae"], torch.zeros(shape[0]))
    assert torch.equal(got["nrmse"], torch.zeros(shape[0]))
    assert torch.isposinf(got["psnr"]).all(), got["psnr"]          # MONAI's 10 log10 of a zero MSE gives the same


@pytest.mark.parametrize("win", [3, 7, 11])
@pytest.mark.parametrize("shape", [(1, 1, 11, 11, 11), (1, 1, 12, 37, 53), (1, 1, 17, 16, 33), (1, 1, 24, 40, 56), (1, 1, 27, 49, 65),
                                   (2, 2, 12, 37, 53), (1, 3, 45, 26, 43), (1, 1, 96, 27, 42)])
def test_every_voxel_is_counted_once(cuda, shape, win):
    """x - y == 1 everywhere (exactly: y on a grid of eighths): mse == mae == 1 exactly, whatever the tiles' halos overlap."""
    g = torch.Generator().manual_seed(3)
    y = torch.randint(0, 8, shape, generator=g).float() / 8
    got = run_kernel(y + 1.0, y, cuda, full=False, win_size=win)
    assert torch.equal(got["mse"], torch.ones(shape[0])) and torch.equal(got["mae"], torch.ones(shape[0])), (got["mse"], got["mae"])
    ref = torch.sqrt(float(y[0].numel()) / (y.double() ** 2).reshape(shape[0], -1).sum(dim=1))
    assert torch.allclose(got["nrmse"].double(), ref, rtol=2 ** -22, atol=0)
    assert torch.equal(got["y_min"], y.reshape(shape[0], -1).min(dim=1).values)
    assert torch.equal(got["y_max"], y.reshape(shape[0], -1).max(dim=1).values)


def test_strided_crop_of_a_padded_buffer_is_scored_in_place(cuda):
    x, y = make_pair("noisy5", (2, 1, 24, 40, 56), seed=21)
    pad = torch.full((2, 1, 32, 48, 64), 7.0)                      # what the sliding-window path leaves around the scan
    pad[:, :, :24, :40, :56] = x
    view = pad.to(cuda)[:, :, :24, :40, :56]
    assert not view.is_contiguous() and view.stride(4) == 1
    from ldm3d.metrics import image_metrics
    got = {k: v.cpu() for k, v in image_metrics(view, y.to(cuda), return_full_image=True).items()}
    check_against_yardstick("strided crop view", got, x, y)
    same = run_kernel(x, y, cuda)
    for k in same:
        assert torch.equal(got[k], same[k]), k                     # the view and its contiguous copy: the same bits
    pad_y = torch.zeros((2, 1, 30, 50, 70))                        # both operands strided, crops that start inside their buffers
    pad_y[:, :, 3:27, 5:45, 7:63] = y
    pad[:, :, 8:32, 8:48, 8:64] = x
    got = {k: v.cpu() for k, v in image_metrics(pad.to(cuda)[:, :, 8:32, 8:48, 8:64], pad_y.to(cuda)[:, :, 3:27, 5:45, 7:63],
                                                return_full_image=True).items()}
    for k in same:
        assert torch.equal(got[k], same[k]), k


def test_two_calls_give_the_same_bits(cuda):
    from ldm3d.metrics import image_metrics
    x, y = make_pair("noisy5", (2, 2, 40, 56, 72), seed=4)
    xd, yd = x.to(cuda), y.to(cuda)
    a = image_metrics(xd, yd, return_full_image=True)
    b = image_metrics(xd, yd, return_full_image=True)
    c = image_metrics(xd, yd)                                      # without the map buffer: the same scalars
    assert "ssim_map" not in c
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for k in c:
        assert torch.equal(a[k], c[k]), k


def test_metric_classes_follow_monai(cuda):
    from ldm3d.metrics import PSNRMetric, SSIMMetric, image_metrics
    x, y = make_pair("noisy5", (2, 1, 24, 40, 56), seed=8)
    xd, yd = x.to(cuda), y.to(cuda)
    ref = image_metrics(xd, yd)
    ssim = SSIMMetric(spatial_dims=3, data_range=1.0, kernel_type="gaussian", win_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03)
    v = ssim(y_pred=xd, y=yd)
    assert v.shape == (2, 1) and torch.equal(v[:, 0], ref["ssim"])
    ssim(xd, yd)
    assert torch.equal(ssim.aggregate(), torch.cat([v, v]).mean()) and ssim.aggregate("none").shape == (4, 1)
    psnr = PSNRMetric(max_val=1.0)
    p = psnr(xd, yd)
    assert p.shape == (2, 1) and torch.equal(p[:, 0], ref["psnr"])
    assert torch.equal(PSNRMetric(max_val=2.0, reduction="none")(xd, yd)[:, 0], image_metrics(xd, yd, data_range=2.0)["psnr"])


def test_error_paths_fail_with_a_message(cuda, built_lib):
    """Through the C ABI on real device buffers: nothing is launched, nothing faults."""
    from ldm3d import _lib
    L = built_lib
    x = torch.rand((1, 1, 24, 40, 56), device=cuda)
    y = torch.rand((1, 1, 24, 40, 56), device=cuda)
    out = torch.full((1, 8), -7.0, device=cuda)
    scratch = torch.empty((1 << 20,), dtype=torch.uint8, device=cuda)
    w = (C.c_float * 13)(*([1.0 / 13] * 13))

    def call(win=11, D=24, H=40, W=56, xs=None):
        st = (C.c_int64 * 5)(*(xs or x.stride()))
        ys = (C.c_int64 * 5)(*y.stride())
        return L.ldm_op_image_metrics(x.data_ptr(), st, y.data_ptr(), ys, 1, 1, D, H, W, w, win, 1.0, 0.01, 0.03, out.data_ptr(), None,
                                      scratch.data_ptr(), scratch.numel(), _lib.current_stream())

    for kw, word in ((dict(win=8), "odd"), (dict(win=13), "odd"), (dict(H=9), "at least win"),
                     (dict(W=28, xs=(24 * 40 * 56, 24 * 40 * 56, 40 * 56, 56, 2)), "contiguous")):
        assert call(**kw) < 0, kw
        with pytest.raises(_lib.LdmError, match=word):
            _lib.check(call(**kw))
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                               # no kernel ran
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[0, :7]).all())
    from ldm3d.metrics import image_metrics
    with pytest.raises(ValueError, match="smaller than"):
        image_metrics(x[:, :, :, :10], y[:, :, :, :10])
    with pytest.raises(ValueError, match="win_size"):
        image_metrics(x, y, win_size=13)
    with pytest.raises(_lib.LdmError):
        image_metrics(x, y.cpu())
    strided = image_metrics(x[..., ::2], y[..., ::2])              # the wrapper makes a W-strided view contiguous itself
    dense = image_metrics(x[..., ::2].contiguous(), y[..., ::2].contiguous())
    assert all(torch.equal(strided[k], dense[k]) for k in dense)


def _prepared(pair, patch, whole):
    import numpy as np
    from ldm3d.data import crop, crop_start, load_pair, scale_percentiles
    image, label = load_pair(pair)
    if not whole:
        roi = [min(p, d) // 4 * 4 for p, d in zip(patch, image.shape)]
        start = crop_start(image.shape, roi, None)
        image, label = crop(image, start, roi), crop(label, start, roi)
    return tuple(torch.from_numpy(np.ascontiguousarray(scale_percentiles(v)))[None, None] for v in (image, label))


def test_inference_metrics_end_to_end(tmp_path):
    from ldm3d.data import write_synthetic_pairs
    pair = write_synthetic_pairs(str(tmp_path / "pairs"), 1, (100, 104, 118))[0]
    env = {"npz_dir": str(tmp_path / "pairs"), "model_dir": str(tmp_path / "ckpt"), "output_dir": str(tmp_path / "out"),
           "tfevent_path": str(tmp_path / "tfevent"), "resume_ckpt": False, "seed": 0}
    env_file = str(tmp_path / "environment.json")
    with open(env_file, "w") as fh:
        json.dump(env, fh)
    cfg_file = os.path.join(ROOT, "config", "config_synthetic_train.json")
    with open(cfg_file) as fh:
        patch = [int(p) for p in json.load(fh)["diffusion_train"]["patch_size"]]
    base = [sys.executable, os.path.join(ROOT, "inference.py"), "-e", env_file, "-c", cfg_file, "-n", "1", "--random-init", "--steps", "3",
            "--condition", pair, "--metrics"]
    for whole in (False, True):
        out = tmp_path / "out" / "metrics.jsonl"
        if out.exists():
            out.unlink()
        r = subprocess.run(base + (["--sliding-window"] if whole else []), cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        recs = [json.loads(l) for l in open(out)]
        assert len(recs) == 1
        rec = recs[0]
        image, label = _prepared(pair, patch, whole)
        assert rec["shape"] == list(label.shape[2:]) == ([100, 104, 118] if whole else [96, 96, 96])
        assert rec["file"].endswith(".nii") and (tmp_path / "out" / rec["file"]).exists()
        assert rec["ssim_settings"]["win_size"] == 11 and rec["ssim_settings"]["data_range"] == 1.0
        for side in ("denoised", "input"):
            assert sorted(rec[side]) == sorted(("ssim",) + SCALARS)
            assert all(isinstance(v, float) and v == v and abs(v) != float("inf") for v in rec[side].values()), rec[side]
        got = {k: torch.tensor([rec["input"][k]], dtype=torch.float32) for k in ("ssim",) + SCALARS}
        check_against_yardstick(f"inference.py input vs label, {'whole scan' if whole else 'patch'}", got, image, label)
        assert "metrics " + rec["file"] in r.stdout + r.stderr
    bad = subprocess.run([a for a in base if a not in ("--condition", pair)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--condition" in bad.stderr


def test_trainers_log_validation_metrics(tmp_path):
    """train_autoencoder.py / train_diffusion.py --val-metrics: the new scalars appear, finite, next to the ones logged without the flag."""
    env = {"npz_dir": str(tmp_path / "pairs"), "val_fraction": 0.25, "model_dir": str(tmp_path / "ckpt"),
           "tfevent_path": str(tmp_path / "tfevent"), "output_dir": str(tmp_path / "out"), "resume_ckpt": False, "seed": 0}
    env_file = str(tmp_path / "environment.json")
    with open(env_file, "w") as fh:
        json.dump(env, fh)

    def run(script, *extra):
        cmd = [sys.executable, os.path.join(ROOT, script), "-e", env_file, "-c", os.path.join(ROOT, "config", "config_synthetic_train.json"),
               "--random-init", *extra]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout + r.stderr

    def scalars(stage):
        with open(tmp_path / "tfevent" / stage / "scalars.jsonl") as fh:
            recs = [json.loads(l) for l in fh]
        return {t: [r["value"] for r in recs if r["tag"] == t] for t in {r["tag"] for r in recs}}

    log = run("train_autoencoder.py", "--synthetic", "8", "--max-steps", "4", "--val-metrics")
    s = scalars("autoencoder")
    assert s["val_recon_loss"] and len(s["val_recon_psnr"]) == len(s["val_recon_ssim"]) == len(s["val_recon_loss"])
    assert all(v == v and abs(v) != float("inf") for v in s["val_recon_psnr"] + s["val_recon_ssim"]) and all(-1.0 <= v <= 1.0 for v in s["val_recon_ssim"])
    assert "val_recon_psnr" in log
    log = run("train_diffusion.py", "--max-steps", "6", "--sample-steps", "5", "--val-metrics")
    s = scalars("diffusion")
    assert len(s["val_denoised_cond_l1"]) >= 1
    for tag in ("val_psnr", "val_ssim", "val_nrmse"):
        assert len(s[tag]) == len(s["val_denoised_cond_l1"]) and all(v == v and abs(v) != float("inf") for v in s[tag]), (tag, s.get(tag))
    assert "PSNR" in log and "SSIM" in log
