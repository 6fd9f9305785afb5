"""Image metrics off the GPU: known answers of the yardstick itself (tests/metrics_ref.py), the host-side argument checks of
ldm3d.metrics, and the command line of `inference.py --metrics`."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(shape=(1, 1, 14, 15, 16), seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64), torch.rand(shape, generator=g, dtype=torch.float64)


def test_ssim_of_an_image_with_itself_is_one():
    x, _ = _pair()
    m = metrics_ref.ssim_map(x, x)
    assert m.shape == (1, 1, 4, 5, 6)
    assert torch.allclose(m, torch.ones_like(m), atol=1e-12, rtol=0)


def test_ssim_is_symmetric():
    x, y = _pair(seed=1)
    assert torch.allclose(metrics_ref.ssim_map(x, y, win_size=7), metrics_ref.ssim_map(y, x, win_size=7), atol=1e-14, rtol=0)


@pytest.mark.parametrize("a,b,L", [(0.2, 0.7, 1.0), (0.5, 0.5, 1.0), (1.0, 3.0, 4.0)])
def test_ssim_of_constant_images(a, b, L):
    x = torch.full((1, 1, 11, 12, 13), a, dtype=torch.float64)
    y = torch.full((1, 1, 11, 12, 13), b, dtype=torch.float64)
    c1 = (0.01 * L) ** 2
    m = metrics_ref.ssim_map(x, y, data_range=L)
    assert torch.allclose(m, torch.full_like(m, (2 * a * b + c1) / (a * a + b * b + c1)), atol=1e-12, rtol=0)


def test_psnr_mse_mae_nrmse_of_a_known_error():
    y = torch.full((2, 1, 11, 11, 11), 0.5, dtype=torch.float64)
    x = y + 0.1                                                    # mse 0.01 -> psnr 20 dB at max_val 1
    r = metrics_ref.metrics(x, y)
    assert torch.allclose(r["mse"], torch.full((2,), 0.01, dtype=torch.float64), atol=1e-15)
    assert torch.allclose(r["mae"], torch.full((2,), 0.1, dtype=torch.float64), atol=1e-15)
    assert torch.allclose(r["psnr"], torch.full((2,), 20.0, dtype=torch.float64), atol=1e-10)
    assert torch.allclose(r["nrmse"], torch.full((2,), 0.2, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(metrics_ref.metrics(x, y, data_range=4.0)["psnr"], torch.full((2,), 20.0 + 20 * math.log10(4.0), dtype=torch.float64))
    assert torch.isposinf(metrics_ref.metrics(y, y)["psnr"]).all()


@pytest.mark.parametrize("win", [3, 7, 11])
def test_windows_sum_to_one(win):
    from ldm3d import metrics
    for kind in ("gaussian", "uniform"):
        ref = metrics_ref.window_1d(kind, win, 1.5)
        assert abs(float(ref.sum()) - 1.0) < 1e-15
        mine = torch.tensor(metrics.window_weights(kind, win, 1.5), dtype=torch.float64)
        assert abs(float(mine.sum()) - 1.0) < 1e-15
        assert torch.allclose(mine, ref, atol=1e-16, rtol=1e-14)   # the package's weights are the yardstick's
    g = metrics_ref.window_1d("gaussian", 11, 1.5)
    assert torch.equal(g, g.flip(0)) and float(g[5]) == float(g.max())
    assert abs(float(g[4] / g[5]) - math.exp(-(1 / 1.5) ** 2 / 2)) < 1e-15


def test_host_side_argument_checks():
    from ldm3d import _lib, metrics
    with pytest.raises(NotImplementedError):
        metrics.SSIMMetric(spatial_dims=2)
    with pytest.raises(ValueError):
        metrics.SSIMMetric(win_size=8)
    with pytest.raises(ValueError):
        metrics.SSIMMetric(win_size=13)
    with pytest.raises(ValueError):
        metrics.SSIMMetric(kernel_type="box")
    with pytest.raises(ValueError):
        metrics.SSIMMetric(reduction="median")
    with pytest.raises(ValueError):
        metrics.PSNRMetric(max_val=0.0)
    x = torch.zeros((1, 1, 12, 12, 12))
    with pytest.raises(ValueError, match="same shape"):
        metrics.image_metrics(x, torch.zeros((1, 1, 12, 12, 13)))
    with pytest.raises(ValueError, match="smaller than"):
        metrics.image_metrics(torch.zeros((1, 1, 12, 10, 12)), torch.zeros((1, 1, 12, 10, 12)))
    with pytest.raises(ValueError, match="smaller than"):
        metrics.SSIMMetric()(torch.zeros((1, 1, 12, 10, 12)), torch.zeros((1, 1, 12, 10, 12)))
    with pytest.raises(ValueError):
        metrics.image_metrics(x[0], x[0])                          # [C, D, H, W]: not a batch of volumes
    with pytest.raises(_lib.LdmError, match="GPU only"):           # CPU tensors: no CPU path, as everywhere else
        metrics.image_metrics(x, x)
    with pytest.raises(_lib.LdmError):
        metrics.SSIMMetric()(x, x)
    with pytest.raises(_lib.LdmError):
        metrics.PSNRMetric(1.0)(x, x)


def test_c_abi_rejects_bad_arguments_without_a_gpu(built_lib):
    """ldm_op_image_metrics validates before it launches: these calls never reach a kernel."""
    import ctypes as C
    L = built_lib
    assert L.ldm_op_image_metrics_scratch_bytes(1, 1, 24, 40, 56, 11) > 0
    assert L.ldm_op_image_metrics_scratch_bytes(1, 1, 24, 40, 56, 8) == 0
    st = (C.c_int64 * 5)(24 * 40 * 56, 24 * 40 * 56, 40 * 56, 56, 1)
    w = (C.c_float * 13)(*([1.0 / 13] * 13))
    fake = 4096                                                    # any non-null address: validation fails first

    def call(win=11, D=24, H=40, W=56, strides=st, x=fake):
        return L.ldm_op_image_metrics(x, strides, fake, st, 1, 1, D, H, W, w, win, 1.0, 0.01, 0.03, fake, None, fake, 1 << 20, None)

    for kw, word in ((dict(win=8), b"odd"), (dict(win=13), b"odd"), (dict(D=10), b"at least win"), (dict(W=9), b"at least win"),
                     (dict(x=None), b"null"), (dict(strides=(C.c_int64 * 5)(24 * 40 * 112, 24 * 40 * 112, 40 * 112, 112, 2)), b"contiguous")):
        assert call(**kw) < 0, kw
        assert word in L.ldm_last_error(), (kw, L.ldm_last_error())


def _parse(monkeypatch, *extra):
    import inference
    monkeypatch.setattr(sys, "argv", ["inference.py", "-e", os.path.join(ROOT, "config", "environment_synthetic.json"),
                                      "-c", os.path.join(ROOT, "config", "config_synthetic_24.json"), *extra])
    return inference.parse_cli()


def test_cli_takes_metrics_only_with_condition(monkeypatch, capsys):
    assert _parse(monkeypatch).metrics is False                    # off by default
    ns = _parse(monkeypatch, "--condition", "pair.npz", "--metrics")
    assert ns.metrics is True and ns.condition == "pair.npz"
    assert _parse(monkeypatch, "--condition", "pair.npz", "--sliding-window", "--metrics").metrics is True
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--metrics")
    assert "--condition" in capsys.readouterr().err
