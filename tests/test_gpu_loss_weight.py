"""Stage-2 objective options on the GPU (-m gpu): ldm_op_weighted_mse_loss and ldm_timestep_resample against the fp64 restatement of
loss_weight_ref.py, operator by operator, then DiffusionTrainer end to end on the tiny UNet and train_diffusion.py as a child process.
Every output buffer is NaN-filled before each launch."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cfgs
import loss_weight_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
ERR_BAD_ARG, ERR_UNSUPPORTED = -1, -2
T, K = 50, 7                                             # the small table: linear_beta 0.01 .. 0.3, 6 timesteps above gamma = 5
SMALL = dict(num_train_timesteps=T, schedule="linear_beta", beta_start=0.01, beta_end=0.3)
BETA = float(np.float32(0.9))                            # the kernel receives the fp32 value
# Launch geometry (csrc/loss_weight.h): a sample is covered by G = min(ceil(per_sample / 1024), cap(B)) virtual blocks of 256 virtual
# threads, and one pass over the sample is 256 G elements.  Below the cap a sample takes at most 4 passes.  cap(64) = 16, so at B = 64
# a sample of 16389 elements has G = 16, a pass of 4096 elements, and takes 5 passes (the fifth holds 5 elements).  At B = 1 and 3 the
# same size has G = 17, a pass of 4352, and takes 4 passes; its 17th virtual block is alone in its real block.
PAST_FOUR_PASSES_AT_CAP_16 = 16 * 1024 + 5
SIZES = [1, 3, 4, 5, 1023, 2052, PAST_FOUR_PASSES_AT_CAP_16]   # 2052: the 16-byte body over 3 virtual blocks (one real block, partly idle)


def _L():
    from ldm3d import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(shape, cuda):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=cuda)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def _table():
    from ldm3d.loss_weighting import min_snr_weights
    from ldm3d.schedulers import DDPMScheduler
    return min_snr_weights(DDPMScheduler(**SMALL), 5.0)


def _loss(cuda, pd, td, B, n, ts=None, tab=None, sw=None, tracker=None, Tt=T, Kk=K, grad=True, per=True, pad=0):
    """One call; -> (status, loss_out [2], per_sample_out [B] | None, grad_out [B n + pad] | None), all on the CPU."""
    lo = _nan((2,), cuda)
    po = _nan((B,), cuda) if per else None
    go = _nan((B * n + pad,), cuda) if grad else None
    st = _L().ldm_op_weighted_mse_loss(_p(pd), _p(td), B, n, _p(ts), _p(tab), Tt, _p(sw), _p(tracker), Kk, BETA, _p(lo), _p(po), _p(go), _stream())
    torch.cuda.synchronize()
    return st, lo.cpu(), None if po is None else po.cpu(), None if go is None else go.cpu()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("B", [1, 3, 64])
def test_weighted_loss_against_fp64(cuda, B, n):
    """lw_part_kernel / lw_fold_kernel with table, per-sample factors and tracker.  Gates: both losses and the per-sample losses rel 1e-6
    (the project's gate for ldm_op_mse_loss), every gradient element rel 4e-7 of the fp64 value (five fp32 roundings of 2^-24: the
    difference, the scale, the two weights being fp32, their product, the final product); a repeat is bit-identical; with grad_out,
    per_sample_out and tracker NULL the losses keep their bits; 1e18 behind B n is not read and nothing is written there.
    Measured over the 21 cases: losses <= 8.8e-8, per-sample <= 1.5e-7, gradient <= 2.2e-7."""
    g = torch.Generator().manual_seed(1000 * B + n)
    pr, tg = torch.randn((B * n + 4,), generator=g), torch.randn((B * n + 4,), generator=g)
    pr[B * n:] = 1e18
    tg[B * n:] = -1e18
    ts = torch.randint(0, T, (B,), generator=g)
    if B > 1:
        ts[0], ts[1] = 2, 40                              # one clamped (snr > gamma) and one unclamped timestep for certain
    sw = torch.rand((B,), generator=g) + 0.5
    tab = _table()
    want_w, want_u, want_per, want_grad = ref.weighted_loss(pr[:B * n].reshape(B, n).numpy(), tg[:B * n].reshape(B, n).numpy(), ts.numpy(),
                                                            tab.numpy(), sw.numpy())
    pd, td, tsd, tabd, swd = pr.to(cuda), tg.to(cuda), ts.to(cuda), tab.to(cuda), sw.to(cuda)
    runs = []
    for _ in range(2):
        trk = torch.zeros((2, K), device=cuda)
        st, lo, po, go = _loss(cuda, pd, td, B, n, tsd, tabd, swd, trk, pad=4)
        assert st == 0
        runs.append((lo, po, go, trk.cpu()))
    for a, b in zip(runs[0], runs[1]):
        assert _bits_equal(a, b), "a repeat launch is not bit-identical"
    lo, po, go, trk = runs[0]
    st, lo2, _, _ = _loss(cuda, pd, td, B, n, tsd, tabd, swd, None, grad=False, per=False)
    assert st == 0 and _bits_equal(lo, lo2), "the losses depend on the optional outputs"
    e_w, e_u = abs(float(lo[0]) - want_w) / want_w, abs(float(lo[1]) - want_u) / want_u
    e_p = float(np.max(np.abs(po.double().numpy() - want_per) / want_per))
    gerr = np.abs(go[:B * n].double().numpy().reshape(B, n) - want_grad)
    scale = np.abs(want_grad)
    e_g = float(np.max(np.where(scale > 0, gerr / np.where(scale > 0, scale, 1.0), gerr)))
    print(f"weighted_mse_loss B={B} n={n}: loss rel {e_w:.1e}, unweighted rel {e_u:.1e}, per-sample rel {e_p:.1e} (gate 1e-6), gradient rel {e_g:.1e} (gate 4e-7)")
    assert torch.isnan(go[B * n:]).all(), "wrote past B n"
    assert e_w <= 1e-6 and e_u <= 1e-6 and e_p <= 1e-6
    assert e_g <= 4e-7
    want_trk = ref.tracker_update(np.zeros((2, K)), want_per, ts.numpy(), K, T, BETA)
    assert (trk[1].double().numpy() == want_trk[1]).all()
    seen = want_trk[1] > 0
    assert np.max(np.abs(trk[0].double().numpy()[seen] - want_trk[0][seen]) / want_trk[0][seen]) <= 1e-6


@pytest.mark.parametrize("n", [4, 1023, 2052])
def test_unit_weights_at_batch_one_are_mse_loss_bit_for_bit(cuda, n):
    """With B = 1 and no weights the per-sample geometry is mse_part_kernel's own: loss_out[0], loss_out[1] and the gradient equal
    ldm_op_mse_loss's bits; a table of 0.25 scales loss and gradient exactly (a power of two commutes with every rounding)."""
    g = torch.Generator().manual_seed(n)
    pd, td = torch.randn((n,), generator=g).to(cuda), torch.randn((n,), generator=g).to(cuda)
    l0, g0 = _nan((1,), cuda), _nan((n,), cuda)
    assert _L().ldm_op_mse_loss(_p(pd), _p(td), n, _p(l0), _p(g0), _stream()) == 0
    st, lo, po, go = _loss(cuda, pd, td, 1, n)
    assert st == 0 and _bits_equal(lo[0:1], l0) and _bits_equal(lo[1:2], l0) and _bits_equal(po, l0) and _bits_equal(go, g0)
    quarter = torch.full((T,), 0.25, device=cuda)
    st, lo, po, go = _loss(cuda, pd, td, 1, n, torch.tensor([7], device=cuda), quarter)
    assert st == 0 and _bits_equal(lo[0:1], 0.25 * l0.cpu()) and _bits_equal(lo[1:2], l0) and _bits_equal(go, 0.25 * g0.cpu())


def test_misaligned_input_takes_the_scalar_path(cuda):
    """per_sample % 4 == 0 but pointers 4 bytes off a 16-byte boundary: not refused, same values as the aligned call bit for bit."""
    B, n = 3, 64
    g = torch.Generator().manual_seed(5)
    pr, tg = torch.randn((B * n + 1,), generator=g), torch.randn((B * n + 1,), generator=g)
    pa, ta = pr[1:].clone().to(cuda), tg[1:].clone().to(cuda)
    pm, tm = pr.to(cuda)[1:], tg.to(cuda)[1:]
    assert pa.data_ptr() % 16 == 0 and pm.data_ptr() % 16 == 4
    a, b = _loss(cuda, pa, ta, B, n), _loss(cuda, pm, tm, B, n)
    assert a[0] == b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert _bits_equal(x, y)


def test_out_of_range_timesteps_are_loud_and_read_nothing(cuda):
    """t = -1 and t = 50 beside valid timesteps: those samples' gradients and loss_out[0] are NaN, the others' gradients are correct, the
    tracker skips them, and a finite huge guard behind (and in front of) the table is never read: no finite output depends on it."""
    B, n = 4, 37
    g = torch.Generator().manual_seed(9)
    pr, tg = torch.randn((B, n), generator=g), torch.randn((B, n), generator=g)
    ts = torch.tensor([-1, 3, 50, 49])
    tab = _table()
    outs = []
    for guard in (1e30, -3e33):
        buf = torch.full((T + 16,), guard)
        buf[8:8 + T] = tab
        trk = torch.zeros((2, K), device=cuda)
        st, lo, po, go = _loss(cuda, pr.to(cuda), tg.to(cuda), B, n, ts.to(cuda), buf.to(cuda)[8:8 + T], None, trk)
        assert st == 0
        outs.append((lo, po, go, trk.cpu()))
    for a, b in zip(outs[0], outs[1]):
        assert _bits_equal(a, b), "an output depends on the guard around the table"
    lo, po, go, trk = outs[0]
    go = go.reshape(B, n)
    _, want_u, want_per, want_grad = ref.weighted_loss(pr.numpy(), tg.numpy(), ts.numpy(), tab.numpy())
    assert torch.isnan(lo[0]) and torch.isnan(go[0]).all() and torch.isnan(go[2]).all()
    assert abs(float(lo[1]) - want_u) <= 1e-6 * want_u and np.max(np.abs(po.double().numpy() - want_per) / want_per) <= 1e-6
    for b in (1, 3):
        assert torch.isfinite(go[b]).all()
        assert np.max(np.abs(go[b].double().numpy() - want_grad[b]) / np.abs(want_grad[b])) <= 4e-7
    assert trk[1].tolist() == [1, 0, 0, 0, 0, 0, 1]


def test_tracker_update_in_batch_order(cuda):
    """Three consecutive launches, B = 8, T = 50, K = 7: two samples per launch share bin 0 (and more collide over the launches), one
    prediction is NaN (skipped).  m2 rel 1e-6 against fp64 in batch order, counts exact.  Negative control: the reference walked in
    reverse batch order is further than the gate from the kernel.  Measured: m2 rel 7.0e-8; the reversed order is off by 0.75 rel."""
    B, n = 8, 33
    state = torch.zeros((2, K), device=cuda)
    fwd, rev = np.zeros((2, K)), np.zeros((2, K))
    g = torch.Generator().manual_seed(17)
    for launch in range(3):
        scale = torch.tensor([1.0, 3.0, 0.5, 2.0, 1.0, 0.25, 1.5, 4.0])[:, None]
        pr, tg = torch.randn((B, n), generator=g) * scale, torch.zeros((B, n))
        pr[5, 7] = float("nan")
        ts = torch.tensor([0, 6, 10, 20, 30, 33, 44, 49 - launch])          # t = 0 and 6 share bin 0; 44 and 49 - launch share bin 6
        st, lo, po, _ = _loss(cuda, pr.to(cuda), tg.to(cuda), B, n, ts.to(cuda), None, None, state)
        assert st == 0 and torch.isnan(lo[0]) and torch.isnan(po[5])
        per = ref.weighted_loss(pr.numpy(), tg.numpy())[2]
        ref.tracker_update(fwd, per, ts.numpy(), K, T, BETA)
        ref.tracker_update(rev, per, ts.numpy(), K, T, BETA, order=list(range(B - 1, -1, -1)))
    got = state.cpu().double().numpy()
    assert (got[1] == fwd[1]).all() and fwd[1].sum() == 3 * 7 and fwd[1, 0] == 6
    seen = fwd[1] > 0
    err = float(np.max(np.abs(got[0][seen] - fwd[0][seen]) / fwd[0][seen]))
    err_rev = float(np.max(np.abs(got[0][seen] - rev[0][seen]) / rev[0][seen]))
    print(f"tracker: m2 rel {err:.1e} (gate 1e-6), against the reversed order {err_rev:.1e}")
    assert err <= 1e-6
    assert err_rev > 1e-6, "the test cannot see the batch order"


def _resample(cuda, state, B, warmup, up, draw=None, idx=None, seed=0, step=0, Tt=T, Kk=K):
    t, iw = torch.full((B,), -7, dtype=torch.int64, device=cuda), _nan((B,), cuda)
    ids = None if idx is None else (C.c_int * B)(*[int(i) for i in idx])
    st = _L().ldm_timestep_resample(_p(state), Kk, Tt, warmup, up, ids, B, seed, step, _p(draw), _p(t), _p(iw), _stream())
    torch.cuda.synchronize()
    return st, t.cpu(), iw.cpu()


POST = np.stack([np.array([0.04, 1.0, 0.25, 9.0, 0.01, 2.25, 0.5]), np.array([12.0, 11, 30, 10, 10, 17, 10])])   # every count >= 10
WARM = np.stack([POST[0], np.array([12.0, 11, 30, 9, 10, 17, 10])])                                                  # one count below 10


@pytest.mark.parametrize("name,state", [("post_warmup", POST), ("warmup", WARM), ("zero_sum_q", np.stack([np.zeros(K), POST[1]])),
                                        ("inf_m2", np.stack([np.array([1.0, np.inf, 1, 1, 1, 1, 1]), POST[1]]))])
def test_resample_with_explicit_draws(cuda, name, state):
    """u0 at the midpoint of every interval of the reference's CDF and 1e-4 inside each of its edges (all of them at least 1e-5 from any
    edge: asserted, none left out), u1 in {0, 0.5, 1 - 2^-24}: 63 draws in one launch.  t exact, iw rel 1e-6; iw == 1.0 exactly in
    warm-up and in the two fall-backs to uniform (zero sum q, an infinite m2).  Measured: iw rel 4.4e-8 after warm-up, 0 in the three uniform states."""
    up, warmup = float(np.float32(1e-3)), 10
    st32 = torch.tensor(state, dtype=torch.float32)
    P, uniform = ref.bin_probabilities(st32.double().numpy(), K, T, warmup, up)
    assert uniform == (name != "post_warmup")
    edges = np.concatenate([[0.0], ref.cdf(P)])
    u0s = []
    for k in range(K):
        u0s += [edges[k] + 1e-4, 0.5 * (edges[k] + edges[k + 1]), edges[k + 1] - 1e-4]
    u0s = np.array(u0s, dtype=np.float32)
    assert len(u0s) == 3 * K and all(np.min(np.abs(float(u) - edges)) >= 1e-5 for u in u0s) and (u0s >= 0).all() and (u0s < 1).all()
    u1s = np.array([0.0, 0.5, 1.0 - 2.0 ** -24], dtype=np.float32)
    draws = np.array([(a, b) for a in u0s for b in u1s], dtype=np.float32)
    B = len(draws)
    assert B == 63
    st, t, iw = _resample(cuda, st32.to(cuda), B, warmup, up, draw=torch.from_numpy(draws).to(cuda))
    assert st == 0
    worst = 0.0
    for b in range(B):
        wt, wiw, _ = ref.draw(st32.double().numpy(), K, T, warmup, up, draws[b, 0], draws[b, 1])
        assert int(t[b]) == wt, (b, draws[b], int(t[b]), wt)
        worst = max(worst, abs(float(iw[b]) - wiw) / wiw)
    print(f"resample {name}: iw rel {worst:.1e} (gate 1e-6)")
    assert worst <= 1e-6
    if uniform:
        assert (iw == 1.0).all()
    else:
        assert len(set(iw.tolist())) == K and (iw != 1.0).all()     # one importance weight per bin, none of them the warm-up's


def test_resample_philox_path(cuda):
    """The kernel's own draws: a function of (seed, step, dataset index) alone.  Permuting idx permutes (t, iw); idx = NULL is
    idx = 0 .. B-1; another step or seed changes them.  64 launches of B = 64 (4096 draws, fixed seeds) from a post-warm-up state: every
    bin's count within 5 binomial standard deviations of 4096 P_k (fp64 reference).  Measured: the largest deviation is 2.14 sigma."""
    up, warmup, B = float(np.float32(1e-3)), 10, 64
    st32 = torch.tensor(POST, dtype=torch.float32)
    sd = st32.to(cuda)
    idx = list(range(100, 100 + B))
    st, t0, w0 = _resample(cuda, sd, B, warmup, up, idx=idx, seed=42, step=3)
    assert st == 0 and (t0 >= 0).all() and (t0 < T).all() and torch.isfinite(w0).all()
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).tolist()
    _, t1, w1 = _resample(cuda, sd, B, warmup, up, idx=[idx[p] for p in perm], seed=42, step=3)
    assert torch.equal(t1, t0[perm]) and _bits_equal(w1, w0[perm])
    _, t2, w2 = _resample(cuda, sd, B, warmup, up, idx=None, seed=42, step=3)
    _, t3, w3 = _resample(cuda, sd, B, warmup, up, idx=list(range(B)), seed=42, step=3)
    assert torch.equal(t2, t3) and _bits_equal(w2, w3) and not torch.equal(t2, t0)
    _, t4, _ = _resample(cuda, sd, B, warmup, up, idx=idx, seed=42, step=4)
    _, t5, _ = _resample(cuda, sd, B, warmup, up, idx=idx, seed=43, step=3)
    _, t6, _ = _resample(cuda, sd, B, warmup, up, idx=idx, seed=42 + (1 << 32), step=3)
    assert not torch.equal(t4, t0) and not torch.equal(t5, t0) and not torch.equal(t6, t0)
    P, uniform = ref.bin_probabilities(st32.double().numpy(), K, T, warmup, up)
    assert not uniform
    counts, within = np.zeros(K), np.zeros(T, dtype=int)
    for step in range(64):
        st, t, iw = _resample(cuda, sd, B, warmup, up, idx=None, seed=7, step=step)
        assert st == 0
        for v in t.tolist():
            counts[ref.bin_of(v, K, T)] += 1
            within[v] += 1
    N = 64 * B
    sigma = np.sqrt(N * P * (1.0 - P))
    dev = np.abs(counts - N * P) / sigma
    print(f"resample philox: bin counts {counts.astype(int).tolist()} vs {np.round(N * P, 1).tolist()}, largest deviation {dev.max():.2f} sigma (gate 5)")
    assert counts.sum() == N and (dev <= 5.0).all()
    lo3, hi3 = ref.bin_edges(K, T)[3:5]                   # the likeliest bin (about 250 expected draws per timestep): u1 reaches all of it
    assert (within[lo3:hi3] > 0).all(), "a timestep of the likeliest bin is never drawn"


def test_refusals_leave_the_outputs_untouched(cuda):
    """B = 65 -> LDM_ERR_UNSUPPORTED; K = 0, K > T, K > 64, NULL pred, B = 0, per_sample = 0, T = 0 -> LDM_ERR_BAD_ARG; nothing launched."""
    n = 8
    pd, td = torch.zeros((65 * n,), device=cuda), torch.ones((65 * n,), device=cuda)
    ts = torch.zeros((65,), dtype=torch.int64, device=cuda)
    trk = torch.zeros((2, 64), device=cuda)

    def untouched(r):
        return all(x is None or torch.isnan(x).all() for x in r[1:])
    r = _loss(cuda, pd, td, 65, n, ts, None, None, trk)
    assert r[0] == ERR_UNSUPPORTED and untouched(r)
    for kw in (dict(Kk=0), dict(Kk=T + 1), dict(Kk=65, Tt=1000)):
        r = _loss(cuda, pd, td, 2, n, ts, None, None, trk, **kw)
        assert r[0] == ERR_BAD_ARG and untouched(r), kw
    assert _loss(cuda, None, td, 2, n, ts)[0] == ERR_BAD_ARG and _loss(cuda, pd, None, 2, n, ts)[0] == ERR_BAD_ARG
    assert _loss(cuda, pd, td, 0, n, ts)[0] == ERR_BAD_ARG and _loss(cuda, pd, td, 2, n, ts, Tt=0)[0] == ERR_BAD_ARG
    lo = _nan((2,), cuda)
    assert _L().ldm_op_weighted_mse_loss(_p(pd), _p(td), 2, 0, None, None, T, None, None, K, BETA, _p(lo), None, None, _stream()) == ERR_BAD_ARG
    assert _L().ldm_op_weighted_mse_loss(_p(pd), _p(td), 2, n, None, _p(td), T, None, None, K, BETA, _p(lo), None, None, _stream()) == ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.isnan(lo).all() and float(trk.abs().sum()) == 0.0
    sd = torch.tensor(POST, dtype=torch.float32, device=cuda)
    for B, Kk, Tt, want in ((65, K, T, ERR_UNSUPPORTED), (4, 0, T, ERR_BAD_ARG), (4, T + 1, T, ERR_BAD_ARG), (4, K, 0, ERR_BAD_ARG)):
        st, t, iw = _resample(cuda, sd, B, 10, 1e-3, Tt=Tt, Kk=Kk)
        assert st == want, (B, Kk, Tt, st)
        assert (t == -7).all() and torch.isnan(iw).all()
    assert _resample(cuda, sd, 4, 10, 1.5)[0] == ERR_BAD_ARG
    t1, w1 = torch.zeros(1, dtype=torch.int64, device=cuda), _nan((1,), cuda)
    assert _L().ldm_timestep_resample(_p(sd), K, T, 10, 1e-3, None, 0, 0, 0, None, _p(t1), _p(w1), _stream()) == ERR_BAD_ARG
    assert _L().ldm_timestep_resample(None, K, T, 10, 1e-3, None, 1, 0, 0, None, _p(t1), _p(w1), _stream()) == ERR_BAD_ARG


# ------------------------------------------------------------------------------------------------ DiffusionTrainer end to end
VCFG = dict(cfgs.VAE_TINY, in_channels=1, out_channels=1, latent_channels=4)
PATCH, LATENT = (16, 16, 16), (4, 4, 4, 4)


class _Pairs:
    randcrop, scale_on_host = False, True

    def __init__(self):
        g = torch.Generator().manual_seed(21)
        self.items = [{"image": torch.rand((1,) + PATCH, generator=g), "label": torch.rand((1,) + PATCH, generator=g)} for _ in range(3)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


@pytest.fixture(scope="module")
def world(cuda):
    """The frozen autoencoder, three fixed pairs and their latent cache: built once, never written."""
    from ldm3d.latents import LatentCache
    from ldm3d.networks import AutoencoderKL
    from oracle import autoencoder as oa, unet as ou
    vae = AutoencoderKL(**VCFG)
    vae.load_state_dict(ou.init_state_dict(oa.ae_param_shapes(VCFG), 2))
    vae = vae.to(cuda).eval()
    pairs = _Pairs()
    return vae, pairs, LatentCache.build(vae, pairs, cuda)


def _trainer(cuda, vae, precision="bf16", pred="epsilon", state=None, **kw):
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.networks import DiffusionModelUNet
    from ldm3d.schedulers import DDPMScheduler
    from ldm3d.trainer import DiffusionTrainer
    from oracle import unet as ou
    unet = DiffusionModelUNet(**cfgs.UNET_TINY_COND)
    unet.load_state_dict(state if state is not None else ou.init_state_dict(ou.unet_param_shapes(cfgs.UNET_TINY_COND), 3, gain=0.5))
    if precision != "bf16":
        unet.set_precision(precision)
    sch = DDPMScheduler(**cfgs.SCHED, prediction_type=pred)
    return DiffusionTrainer(unet.to(cuda), vae, LatentDiffusionInferer(sch, scale_factor=0.7311), lr=1e-4, **kw)


def _explicit(cuda, B, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((B,) + LATENT, generator=g).to(cuda) for _ in range(3)]


def _cached_step(tr, cache, idx, draws, ts):
    e_image, e_label, noise = draws
    loss, skipped = tr.train_step_cached(cache, idx, noise=noise, timesteps=ts, eps_label=e_label, eps_image=e_image)
    torch.cuda.synchronize()
    assert not bool(skipped)
    return loss, tr.unet.flat_grads.clone()


def test_default_trainer_builds_no_tracker(cuda, world):
    tr = _trainer(cuda, world[0])
    assert tr.tracker is None and tr.loss_table is None and tr.last_unweighted_loss is None
    assert tr.objective_state_dict() == {"timestep_draws": 0}


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("path", ["cached", "uncached"])
def test_power_of_two_table_scales_loss_and_gradients_exactly(cuda, world, precision, path):
    """B = 1, loss_weights[t] = 0.25 for every t: flat_grads and the loss are 0.25 x the default trainer's, bit for bit (a power-of-two
    scale commutes with every rounding of the backward plan), in both precisions and through both step entries; the unweighted figure is
    the default loss itself.  Fails without the feature (the constructor takes no loss_weights)."""
    vae, pairs, cache = world
    ts = torch.tensor([417], device=cuda)
    res = []
    for kw in ({}, dict(loss_weights=torch.full((1000,), 0.25))):
        tr = _trainer(cuda, vae, precision, **kw)
        if path == "cached":
            loss, grads = _cached_step(tr, cache, [2], _explicit(cuda, 1, 11), ts)
        else:
            item = pairs[2]
            torch.manual_seed(11)
            loss, skipped = tr.train_step(item["image"][None].to(cuda), item["label"][None].to(cuda), noise=_explicit(cuda, 1, 11)[2], timesteps=ts)
            torch.cuda.synchronize()
            assert not bool(skipped)
            grads = tr.unet.flat_grads.clone()
        res.append((loss.clone(), grads, tr))
    (l0, g0, _), (l1, g1, tr) = res
    assert bool(torch.isfinite(l0)) and float(g0.abs().max()) > 0.0
    assert _bits_equal(l1.reshape(1), (0.25 * l0).reshape(1)), (float(l1), float(l0))
    assert _bits_equal(tr.last_unweighted_loss.reshape(1), l0.reshape(1))
    assert torch.equal(g1, 0.25 * g0), float((g1 - 0.25 * g0).abs().max())
    assert int(tr.tracker.state[1].sum()) == 1


def test_two_samples_with_different_weights(cuda, world):
    """B = 2 under loss_weighting="min_snr", fp32 precision mode, t = (10, 500): w0 = 5 / snr_10 < 1 (clamped), w1 = 1 (unclamped).
    flat_grads against (w0 g0 + w1 g1) / 2 with g_b the default trainer's B = 1 gradients of sample b.  The gate is 2 x the noise floor
    of "a batch is the mean of its samples", measured here as the rel-L2 of the same identity with w0 = w1 = 1 on the default path (the
    weights add one rounding per element on top of an identical sum).
    Measured: floor 1.29e-07, weighted 9.54e-08 (rel-L2); the loss against (w0 l0 + w1 l1) / 2: 4.8e-08."""
    from ldm3d.loss_weighting import min_snr_weights
    vae, _, cache = world
    idx, tvals = [2, 0], [10, 500]
    draws = _explicit(cuda, 2, 5)
    ts = torch.tensor(tvals, device=cuda)
    singles = []
    for b in range(2):
        tr = _trainer(cuda, vae, "fp32")
        singles.append(_cached_step(tr, cache, [idx[b]], [d[b:b + 1] for d in draws], ts[b:b + 1]))
    table = min_snr_weights(_trainer(cuda, vae, "fp32").inferer.scheduler, 5.0).double()
    w = [float(table[t]) for t in tvals]
    assert w[0] < 1.0 and w[1] == 1.0

    def rel_l2(a, b):
        return float((a.double() - b).norm() / b.norm())
    l_def, g_def = _cached_step(_trainer(cuda, vae, "fp32"), cache, idx, draws, ts)
    floor = rel_l2(g_def, 0.5 * (singles[0][1].double() + singles[1][1].double()))
    trw = _trainer(cuda, vae, "fp32", loss_weighting="min_snr", snr_gamma=5.0)
    l_w, g_w = _cached_step(trw, cache, idx, draws, ts)
    err = rel_l2(g_w, 0.5 * (w[0] * singles[0][1].double() + w[1] * singles[1][1].double()))
    want_loss = 0.5 * (w[0] * float(singles[0][0]) + w[1] * float(singles[1][0]))
    e_loss = abs(float(l_w) - want_loss) / want_loss
    print(f"two samples, min_snr weights {w[0]:.4f}, {w[1]:.1f}: rel-L2 {err:.2e}, floor of the unweighted identity {floor:.2e} (gate 2 x floor); loss rel {e_loss:.1e}")
    assert floor > 0.0 or err == 0.0
    assert err <= 2.0 * floor
    assert e_loss <= 1e-6
    assert abs(float(trw.last_unweighted_loss) - float(l_def)) <= 1e-6 * float(l_def)


def test_loss_aware_sampling_is_reproducible_and_resumes(cuda, world):
    """timestep_sampling="loss_aware" on the cached path, draws by the kernel: two trainers from one seed walk the same timesteps and
    losses over 4 steps; a trainer resumed from the state saved after step 2 reproduces steps 3 and 4 bit for bit; report() has K rows
    whose counts sum to the finite samples seen.  warmup = 0 here, so that steps 2 .. 4 draw from the tracker and carry iw != 1."""
    vae, _, cache = world
    batches = ([0, 1], [2, 1], [1, 0], [2, 0])

    def build(state=None):
        tr = _trainer(cuda, vae, state=state, timestep_sampling="loss_aware", timestep_bins=10)
        tr.cache_seed = 3
        tr.tracker.warmup = 0
        seen, inner = [], tr._timesteps

        def spy(*a, **k):
            t = inner(*a, **k)
            seen.append((t.clone(), None if tr._iw is None else tr._iw.clone()))
            return t
        tr._timesteps = spy
        return tr, seen

    def run(tr, steps):
        out = []
        for idx in steps:
            loss, skipped = tr.train_step_cached(cache, idx)
            assert not bool(skipped)
            out.append(loss.clone())
        return out
    a, seen_a = build()
    la = run(a, batches[:2])
    saved = {"unet": {k: v.detach().clone() for k, v in a.unet.state_dict().items()}, "optimizer": a.optimizer.state_dict(),
             "objective": a.objective_state_dict(), "cached_steps": a.cached_steps}
    la += run(a, batches[2:])
    b, seen_b = build()
    lb = run(b, batches)
    torch.cuda.synchronize()
    assert len(seen_a) == len(seen_b) == 4
    for (ta, wa), (tb, wb), x, y in zip(seen_a, seen_b, la, lb):
        assert torch.equal(ta, tb) and _bits_equal(wa, wb) and _bits_equal(x.reshape(1), y.reshape(1))
        assert ta.dtype == torch.int64 and (ta >= 0).all() and (ta < 1000).all() and torch.isfinite(wa).all()
    assert (seen_a[0][1] == 1.0).all(), "an empty tracker draws uniformly: iw = 1"
    assert any(bool((w != 1.0).any()) for _, w in seen_a[1:]), "no step drew from the tracker"
    c, seen_c = build(state=saved["unet"])
    c.optimizer.load_state_dict(saved["optimizer"])
    c.load_objective_state_dict(saved["objective"])
    c.cached_steps = saved["cached_steps"]
    lc = run(c, batches[2:])
    torch.cuda.synchronize()
    for k in range(2):
        assert torch.equal(seen_c[k][0], seen_a[2 + k][0]) and _bits_equal(seen_c[k][1], seen_a[2 + k][1])
        assert _bits_equal(lc[k].reshape(1), la[2 + k].reshape(1)), (k, float(lc[k]), float(la[2 + k]))
    assert torch.equal(c.unet.flat_params, a.unet.flat_params) and _bits_equal(c.tracker.state, a.tracker.state)
    rows = a.tracker.report()
    assert len(rows) == 10 and sum(r["count"] for r in rows) == 8 and abs(sum(r["prob"] for r in rows) - 1.0) <= 1e-12
    assert rows[0]["lo"] == 0 and rows[-1]["hi"] == 999 and all(r["rms_loss"] > 0 for r in rows if r["count"])
    # explicit timesteps under "loss_aware": no importance weights
    d, _ = build()
    _cached_step(d, cache, [0, 1], _explicit(cuda, 2, 1), torch.tensor([5, 900], device=cuda))
    assert d._iw is None
    # validation stays uniform and unweighted: it does not touch the tracker
    before = a.tracker.state.clone()
    val = a.validate_cached(cache, [[0, 1], [2]])
    assert val == val and val > 0 and torch.equal(a.tracker.state, before)


def test_explicit_timesteps_with_drawn_noise_carry_no_importance_weights(cuda, world):
    """train_step(images, labels, timesteps=ts) under "loss_aware", the noise left to the step: the tracker is not asked for a draw
    (its timesteps would be thrown away and its importance weights would scale the loss), ``_iw`` is None, and loss and gradients
    equal those of a trainer whose only option is a table of ones, bit for bit.  The tracker state is far from uniform here, so a
    stale draw would carry weights other than 1."""
    vae, pairs, _ = world
    item = pairs[1]
    images, labels = item["image"][None].to(cuda), item["label"][None].to(cuda)
    ts = torch.tensor([613], device=cuda)
    aware = _trainer(cuda, vae, timestep_sampling="loss_aware", timestep_bins=10)
    aware.tracker.warmup = 0
    aware.tracker.state[0] = torch.tensor([4.0, 0.01, 1.0, 0.25, 9.0, 0.04, 2.0, 0.5, 0.09, 1.5], device=cuda)
    aware.tracker.state[1] = 20.0
    calls, inner = [], aware.tracker.sample

    def spy(*a, **k):
        calls.append(1)
        return inner(*a, **k)
    aware.tracker.sample = spy
    ones = _trainer(cuda, vae, loss_weights=torch.ones(1000))
    res = []
    torch.manual_seed(11)
    noise = torch.randn((1,) + LATENT, dtype=torch.float32).to(cuda)   # the noise the step draws on the host right after this seed
    for tr in (aware, ones):
        torch.manual_seed(11)
        # the reference trainer gets that noise explicitly: with a uniform draw a missing noise would also consume a device randint
        # in front of the autoencoder's draws, and the two steps would no longer see the same latents
        loss, skipped = tr.train_step(images, labels, timesteps=ts) if tr is aware else tr.train_step(images, labels, noise=noise, timesteps=ts)
        torch.cuda.synchronize()
        assert not bool(skipped)
        res.append((loss.clone(), tr.unet.flat_grads.clone()))
    assert calls == [] and aware._iw is None and aware.timestep_draws == 1
    assert bool(torch.isfinite(res[0][0])) and _bits_equal(res[0][0].reshape(1), res[1][0].reshape(1))
    assert torch.equal(res[0][1], res[1][1])
    torch.manual_seed(12)                                  # and a step that does draw still gets its weights
    aware.train_step(images, labels)
    assert calls == [1] and aware._iw is not None and bool((aware._iw != 1.0).all())


def test_cli_trains_with_min_snr_and_the_loss_aware_draw(tmp_path):
    """train_diffusion.py --random-init --synthetic 4 --max-steps 4 --cache-latents --loss-weighting min_snr --timestep-sampling
    loss_aware in a fresh child process under its own timeout: loss_by_timestep.jsonl has one parseable record per validation (the
    script validates after epoch 0, 3 steps, and again when --max-steps is reached: as many lines as val_diffusion_loss scalars), the last
    one taken at step 4; the unweighted loss is logged beside the weighted one, and the state file carries the tracker and
    timestep_draws."""
    env = {"npz_dir": str(tmp_path / "pairs"), "val_fraction": 0.25, "model_dir": str(tmp_path / "ckpt"),
           "tfevent_path": str(tmp_path / "tfevent"), "output_dir": str(tmp_path / "out"), "resume_ckpt": False, "seed": 0}
    env_file = str(tmp_path / "environment.json")
    json.dump(env, open(env_file, "w"))
    cmd = [sys.executable, os.path.join(ROOT, "train_diffusion.py"), "-e", env_file, "-c", os.path.join(ROOT, "config", "config_synthetic_train.json"),
           "--random-init", "--synthetic", "4", "--max-steps", "4", "--cache-latents", "--sample-steps", "2",
           "--loss-weighting", "min_snr", "--timestep-sampling", "loss_aware"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    lines = open(tmp_path / "tfevent" / "diffusion" / "loss_by_timestep.jsonl").read().splitlines()
    recs = [json.loads(line) for line in lines]                      # every line parses
    rows = [json.loads(line) for line in open(tmp_path / "tfevent" / "diffusion" / "scalars.jsonl")]
    assert len(recs) >= 1 and len(recs) == len([x for x in rows if x["tag"] == "val_diffusion_loss"])
    for rec in recs:
        assert len(rec["bins"]) == 20 and rec["bins"][0]["lo"] == 0 and rec["bins"][-1]["hi"] == 999
        assert abs(sum(b["prob"] for b in rec["bins"]) - 1.0) <= 1e-9
    batch = json.load(open(os.path.join(ROOT, "config", "config_synthetic_train.json")))["diffusion_train"]["batch_size"]
    assert recs[-1]["step"] == 4 and 4 <= sum(b["count"] for b in recs[-1]["bins"]) <= 4 * batch
    weighted = [x["value"] for x in rows if x["tag"] == "train_diffusion_loss_iter"]
    plain = [x["value"] for x in rows if x["tag"] == "train_diffusion_loss_iter_unweighted"]
    assert len(weighted) == len(plain) == 4 and all(v == v and 0 < v < float("inf") for v in weighted + plain)
    assert all(a <= b * (1 + 1e-6) for a, b in zip(weighted, plain)), "epsilon Min-SNR weights are <= 1 and warm-up importance weights are 1"
    state = torch.load(tmp_path / "ckpt" / "diffusion_train_state.pt", map_location="cpu", weights_only=True)
    assert "timestep_draws" in state and tuple(state["loss_tracker"]["state"].shape) == (2, 20)
