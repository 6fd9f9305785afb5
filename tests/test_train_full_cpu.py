"""The comparer of the full-width training-step fixtures (tests/train_full_ref.py) on a synthetic fixture it builds itself: the
reference gradients pass, and each way a backward plan's wiring can go wrong in ONE tensor -- finite, non-zero garbage that the
finite-only tests let through -- fails on the tensor concerned and only there.  No GPU, no oracle run."""
import pytest
import torch

import train_full_ref as tf

ZERO_MARGIN = 10.0


@pytest.fixture(scope="module")
def synth():
    g32, gbf = tf.synthetic()
    return g32, gbf, tf.build_fixture(g32, gbf, index_seed=5)


def _failing(got, fx, mode="bf16"):
    return tf.failing_tensors(tf.compare(got, fx), fx, mode, ZERO_MARGIN)


def test_fixture_shape_and_exempt_list(synth):
    g32, gbf, fx = synth
    assert fx["names"] == list(g32) and fx["samples"].dtype == torch.float32
    assert fx["samples"].numel() == sum(min(v.numel(), tf.K_SAMPLES) for v in g32.values())
    assert tf.exempt(fx) == ["attn.to_k.bias"]
    assert abs(fx["global_floor"] - 1e-2) < 2e-3 and abs(fx["global_floor_sampled"] / fx["global_floor"] - 1.0) < 0.2
    # the indices come back from the stored seed alone
    a, b = tf.sample_indices(fx["numel"].tolist(), fx["index_seed"]), tf.sample_indices(fx["numel"].tolist(), fx["index_seed"])
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_long_exempt_list_is_a_failure(synth):
    g32, gbf, _ = synth
    noisy = dict(gbf)
    noisy["attn.to_q.weight"] = g32["attn.to_q.weight"] + 0.5 * torch.randn(64, 64, generator=torch.Generator().manual_seed(1))
    with pytest.raises(AssertionError):
        tf.exempt(tf.build_fixture(g32, noisy, index_seed=5))


def test_reference_gradients_pass(synth):
    g32, gbf, fx = synth
    for mode, got in (("fp32", g32), ("bf16", g32), ("bf16", gbf)):
        res = tf.compare(got, fx)
        assert tf.failing_tensors(res, fx, mode, ZERO_MARGIN) == [] and tf.global_ok(res, fx, mode, "unet"), mode
    res = tf.compare(g32, fx)
    assert res["e32"] == 0.0 and abs(res["cos"] - 1.0) < 1e-12 and max(res["err"]) == 0.0
    assert abs(res["total_norm"] - fx["total_grad_norm_fp32"]) < 1e-9 * fx["total_grad_norm_fp32"]
    # the bf16-emulated gradients sit ON their floor: the sampled figure of each tensor within the measured spread of the whole-tensor one
    res = tf.compare(gbf, fx)
    for n, e, f in zip(fx["names"], res["err"], fx["floor"].tolist()):
        assert n in tf.exempt(fx) or 0.5 * f <= e <= 1.5 * f, (n, e, f)
    assert not tf.global_ok(tf.compare({k: 1.05 * v for k, v in gbf.items()}, fx), fx, "bf16", "unet")


def _lost_split_copy(v):
    out = v.clone()
    rows = out.shape[0] // 16
    out[3 * rows: 4 * rows] = 0
    return out


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("what,victims,damage", [
    ("zeroed", ["down.0.conv1.conv.weight"], lambda g: {"down.0.conv1.conv.weight": torch.zeros_like(g["down.0.conv1.conv.weight"])}),
    ("zeroed-small", ["down.0.norm1.bias"], lambda g: {"down.0.norm1.bias": torch.zeros_like(g["down.0.norm1.bias"])}),
    ("swapped", ["down.0.conv1.conv.weight", "down.1.conv1.conv.weight"],
     lambda g: {"down.0.conv1.conv.weight": g["down.1.conv1.conv.weight"], "down.1.conv1.conv.weight": g["down.0.conv1.conv.weight"]}),
    ("swapped-vectors", ["down.0.conv1.conv.bias", "down.1.conv1.conv.bias"],
     lambda g: {"down.0.conv1.conv.bias": g["down.1.conv1.conv.bias"], "down.1.conv1.conv.bias": g["down.0.conv1.conv.bias"]}),
    ("kd-kw-transposed", ["out.2.conv.weight"], lambda g: {"out.2.conv.weight": g["out.2.conv.weight"].transpose(2, 4).contiguous()}),
    ("scaled-1.1", ["time_embed.0.weight"], lambda g: {"time_embed.0.weight": 1.1 * g["time_embed.0.weight"]}),
    ("lost-split-copy", ["down.1.conv1.conv.weight"], lambda g: {"down.1.conv1.conv.weight": _lost_split_copy(g["down.1.conv1.conv.weight"])}),
    ("lost-split-copy-linear", ["attn.to_k.weight"], lambda g: {"attn.to_k.weight": _lost_split_copy(g["attn.to_k.weight"])}),
    ("key-bias-garbage", ["attn.to_k.bias"], lambda g: {"attn.to_k.bias": 1e-3 * torch.ones_like(g["attn.to_k.bias"])}),
])
def test_damage_to_one_tensor_fails_there_and_only_there(synth, mode, what, victims, damage):
    g32, gbf, fx = synth
    base = g32 if mode == "fp32" else gbf                   # bf16 mode: the damage sits on top of the rounding noise the gate allows
    got = dict(base)
    got.update(damage(base))
    assert _failing(got, fx, mode) == victims, what
