"""ldm_latent_batch through the C ABI (-m gpu): the one-launch input side of a stage-2 training step from cached latents.

Bit for bit against the chain it stands in for (ldm_op_vae_heads -> torch multiply by the scale factor -> scheduler.add_noise_and_target),
against the fp64 restatement (tests/latent_batch_ref.py), the contract of the in-kernel draws, and the argument checks."""
import ctypes as C
import math

import pytest
import torch

import cfgs
import latent_batch_ref as R

pytestmark = pytest.mark.gpu
BAD_ARG = -1                                                            # LDM_ERR_BAD_ARG, include/ldm3d.h
SHAPES = [(3, 3, 5, 7), (8, 12, 12, 12)]                                # 315 elements (not a multiple of 4) and 13824
PREDS = ["epsilon", "sample", "v_prediction"]


def _call(cache, idx, sa, sb, scale, pred, draws=None, seed=0, step=0, want_draws=False, outs=None, n=None, per_sample=None, B=None):
    """One ldm_latent_batch call -> (status, noisy, cond, target, draws_out).  ``cache`` = (mu_l, sg_l, mu_i, sg_i), each [N, *shape]."""
    from ldm3d import _lib
    L = _lib.lib()
    dev, shape = cache[0].device, tuple(cache[0].shape[1:])
    nb = len(idx) if B is None else B
    if outs is None:
        outs = [torch.empty((max(nb, 1),) + shape, device=dev) for _ in range(3)]
    dout = torch.empty((3, max(nb, 1)) + shape, device=dev) if want_draws else None
    e = draws if draws is not None else (None, None, None)
    arr = (C.c_int * max(len(idx), 1))(*idx)
    rc = L.ldm_latent_batch(cache[0].data_ptr(), cache[1].data_ptr(), cache[2].data_ptr(), cache[3].data_ptr(),
                            cache[0].shape[0] if n is None else n, cache[0][0].numel() if per_sample is None else per_sample, arr, nb,
                            sa.data_ptr(), sb.data_ptr(), scale, R.PRED.get(pred, pred), _lib.ptr(e[0]), _lib.ptr(e[1]), _lib.ptr(e[2]),
                            seed, step, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), _lib.ptr(dout), _lib.current_stream())
    return rc, outs[0], outs[1], outs[2], dout


def _heads(ml, eps):
    """ldm_op_vae_heads on ONE sample: ml [2L, ...] (mu | log_var), eps [L, ...] or None -> (mu, sigma, z = mu + sigma * eps)."""
    from ldm3d import _lib
    Lc = ml.shape[0] // 2
    dhw = ml[0].numel()
    mu, sg, z = (torch.empty((Lc,) + tuple(ml.shape[1:]), device=ml.device) for _ in range(3))
    _lib.check(_lib.lib().ldm_op_vae_heads(ml.data_ptr(), _lib.ptr(eps), mu.data_ptr(), sg.data_ptr(), z.data_ptr(), 1, Lc, dhw,
                                           _lib.current_stream()))
    return mu, sg, z


@pytest.fixture(scope="module")
def caches(cuda):
    """Per shape: random (mu | log_var) of N = 3 samples for label and image, their heads through ldm_op_vae_heads sample by sample, and
    fixed draws for B = 3.  Built once, never written."""
    out = {}
    for shape in SHAPES:
        g = torch.Generator(device=cuda).manual_seed(sum(shape))
        Lc = shape[0]
        ml_l = torch.randn((3, 2 * Lc) + shape[1:], device=cuda, generator=g) * 1.5
        ml_i = torch.randn((3, 2 * Lc) + shape[1:], device=cuda, generator=g) * 1.5
        mu_l, sg_l = (torch.stack(t) for t in zip(*[_heads(ml_l[n].contiguous(), None)[:2] for n in range(3)]))
        mu_i, sg_i = (torch.stack(t) for t in zip(*[_heads(ml_i[n].contiguous(), None)[:2] for n in range(3)]))
        draws = tuple(torch.randn((3,) + shape, device=cuda, generator=g) for _ in range(3))
        out[shape] = dict(ml_l=ml_l, ml_i=ml_i, cache=(mu_l, sg_l, mu_i, sg_i), draws=draws)
    return out


def _coefs(sch, t):
    return sch._noising_coefs(t, t.device)


CASES = [([2, 0, 2], [0, 999, 417]), ([1], [999]), ([0], [0])]


@pytest.mark.parametrize("scale", [1.0, 0.7311])
@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("idx,ts", CASES)
@pytest.mark.parametrize("shape", SHAPES)
def test_explicit_draws_equal_todays_chain_bit_for_bit(cuda, caches, shape, idx, ts, pred, scale):
    """ldm_op_vae_heads per sample (z = mu + sigma * eps) -> torch's fp32 multiply by the scale factor (skipped at 1.0, as
    LatentDiffusionInferer does) -> scheduler.add_noise_and_target, against one ldm_latent_batch call on the same mu, sigma and draws."""
    from ldm3d.schedulers import DDPMScheduler
    c = caches[shape]
    B = len(idx)
    e_l, e_i, nz = (d[:B].contiguous() for d in c["draws"])
    sch = DDPMScheduler(**cfgs.SCHED, prediction_type=pred)
    t = torch.tensor(ts, device=cuda)
    z = torch.stack([_heads(c["ml_l"][n].contiguous(), e_l[b].contiguous())[2] for b, n in enumerate(idx)])
    want_cond = torch.stack([_heads(c["ml_i"][n].contiguous(), e_i[b].contiguous())[2] for b, n in enumerate(idx)])
    if scale != 1.0:
        z = z * scale
    want_noisy, want_target = sch.add_noise_and_target(original_samples=z, noise=nz, timesteps=t)
    sa, sb = _coefs(sch, t)
    rc, noisy, cond, target, _ = _call(c["cache"], idx, sa, sb, scale, pred, draws=(e_l, e_i, nz))
    assert rc == 0
    assert torch.equal(noisy, want_noisy), float((noisy - want_noisy).abs().max())
    assert torch.equal(cond, want_cond), float((cond - want_cond).abs().max())
    assert torch.equal(target, want_target), float((target - want_target).abs().max())


@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_fp64_formula(cuda, caches, shape, pred):
    """Max abs error <= 1e-6 * max|reference| per output: the bound the project holds add_noise to."""
    from ldm3d.schedulers import DDPMScheduler
    c = caches[shape]
    idx, t = [2, 0, 2], torch.tensor([0, 999, 417], device=cuda)
    sch = DDPMScheduler(**cfgs.SCHED, prediction_type=pred)
    sa, sb = _coefs(sch, t)
    scale = 0.7311
    rc, noisy, cond, target, _ = _call(c["cache"], idx, sa, sb, scale, pred, draws=c["draws"])
    assert rc == 0
    # the kernel receives the scale as a float: the reference multiplies by that fp32 value
    want = R.latent_batch_ref(*c["cache"], idx, *c["draws"], sa, sb, float(torch.tensor(scale, dtype=torch.float32)), pred)[:3]
    for name, got, ref in zip(("noisy", "cond", "target"), (noisy, cond, target), want):
        err, bound = float((got.double().cpu() - ref).abs().max()), 1e-6 * float(ref.abs().max())
        print(f"{shape} {pred} {name}: max abs err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("shape", SHAPES)
def test_device_draws_replay_and_do_not_depend_on_the_batch(cuda, caches, shape, pred):
    from ldm3d.schedulers import DDPMScheduler
    c = caches[shape]["cache"]
    sch = DDPMScheduler(**cfgs.SCHED, prediction_type=pred)
    t = torch.tensor([613, 7], device=cuda)
    sa, sb = _coefs(sch, t)
    kw = dict(scale=0.7311, pred=pred, seed=0x123456789ABCDEF, step=5)
    rc, noisy, cond, target, draws = _call(c, [2, 0], sa, sb, want_draws=True, **kw)
    assert rc == 0 and all(bool(torch.isfinite(x).all()) for x in (noisy, cond, target, draws))
    # 1. the returned draws, fed back explicitly, reproduce the three outputs
    rc, n2, c2, t2, _ = _call(c, [2, 0], sa, sb, kw["scale"], pred, draws=(draws[0], draws[1], draws[2]))
    assert rc == 0 and torch.equal(n2, noisy) and torch.equal(c2, cond) and torch.equal(t2, target)
    # 2. the same samples in the other order (with their timesteps): the same rows, swapped; also without draws_out
    rc, n3, c3, t3, d3 = _call(c, [0, 2], sa.flip(0).contiguous(), sb.flip(0).contiguous(), want_draws=True, **kw)
    assert rc == 0 and torch.equal(d3, draws.flip(1))
    assert torch.equal(n3, noisy.flip(0)) and torch.equal(c3, cond.flip(0)) and torch.equal(t3, target.flip(0))
    # 3. a batch of one gives the row the batch of two gave
    for slot, n in enumerate([2, 0]):
        rc, n1, c1, t1, d1 = _call(c, [n], sa[slot:slot + 1].contiguous(), sb[slot:slot + 1].contiguous(), want_draws=True, **kw)
        assert rc == 0 and torch.equal(d1[:, 0], draws[:, slot])
        assert torch.equal(n1[0], noisy[slot]) and torch.equal(c1[0], cond[slot]) and torch.equal(t1[0], target[slot])
    # 4. the same (seed, step) repeats; another step or another seed (low or high word) does not
    rc, _, _, _, again = _call(c, [2, 0], sa, sb, want_draws=True, **kw)
    assert torch.equal(again, draws)
    for other in (dict(kw, step=6), dict(kw, seed=kw["seed"] + 1), dict(kw, seed=kw["seed"] ^ (1 << 40))):
        rc, _, _, _, d = _call(c, [2, 0], sa, sb, want_draws=True, **other)
        assert rc == 0 and float((d != draws).float().mean()) > 0.99
    # 5. the three streams of one element, and two samples of one stream, are different draws
    assert float((draws[0] != draws[1]).float().mean()) > 0.99 and float((draws[0] != draws[2]).float().mean()) > 0.99
    assert float((draws[1] != draws[2]).float().mean()) > 0.99 and float((draws[:, 0] != draws[:, 1]).float().mean()) > 0.99


def test_device_draws_are_standard_normal(cuda):
    """2^16 draws per stream (4 samples x 16384 elements): |mean| < 5 / sqrt(n) and |var - 1| < 5 * sqrt(2 / n), the five-sigma bounds
    of the sample mean and the sample variance of n standard normals."""
    n_el = 1 << 14
    cache = tuple(torch.zeros((4, n_el), device=cuda) for _ in range(4))
    ones = torch.ones(4, device=cuda)
    rc, _, _, _, draws = _call(cache, [0, 1, 2, 3], ones, ones, 1.0, "epsilon", seed=2024, step=1, want_draws=True)
    assert rc == 0
    n = 4 * n_el
    for s in range(3):
        d = draws[s].double().reshape(-1)
        mean, var = float(d.mean()), float(d.var(unbiased=False))
        print(f"stream {s}: mean {mean:+.5f} (bound {5 / math.sqrt(n):.5f}), var - 1 {var - 1:+.5f} (bound {5 * math.sqrt(2 / n):.5f})")
        assert abs(mean) < 5 / math.sqrt(n) and abs(var - 1) < 5 * math.sqrt(2 / n)
    # the whole pooled sample too (3 * 2^16)
    d = draws.double().reshape(-1)
    assert abs(float(d.mean())) < 5 / math.sqrt(3 * n) and abs(float(d.var(unbiased=False)) - 1) < 5 * math.sqrt(2 / (3 * n))


def test_bad_arguments_launch_nothing(cuda, caches):
    c = caches[SHAPES[0]]
    cache, draws = c["cache"], c["draws"]
    ones = torch.ones(64, device=cuda)

    def refused(idx, draws=None, **kw):
        outs = [torch.full((3,) + SHAPES[0], 7.0, device=cuda) for _ in range(3)]
        rc = _call(cache, idx, ones, ones, 1.0, kw.pop("pred", "epsilon"), draws=draws, outs=outs, **kw)[0]
        torch.cuda.synchronize()
        return rc == BAD_ARG and all(bool((o == 7.0).all()) for o in outs)
    assert refused([0, 3, 1]) and refused([-1]) and refused([0, 1, 3])           # an index outside the cache, anywhere in the batch
    assert refused([], B=0) and refused([0] * 65)                               # B = 0 and B = 65
    for mixed in ((draws[0], None, None), (draws[0], draws[1], None), (None, draws[1], draws[2]), (None, None, draws[2])):
        assert refused([2, 0, 2], draws=mixed)
    assert refused([2, 0, 2], draws=draws, want_draws=True)                     # draws_out belongs to the device draws
    assert refused([0], pred=3) and refused([0], n=0) and refused([0], per_sample=0)
    rc, noisy, _, _, _ = _call(cache, [0] * 64, ones, ones, 1.0, "epsilon")     # the largest batch is accepted
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isfinite(noisy).all())
