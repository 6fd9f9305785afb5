"""CPU checks of the stage-2 objective options: the Min-SNR-gamma table on the project's own schedules (known answers), the bin
arithmetic and the unbiasedness identity of the loss-aware draw in the fp64 restatement (loss_weight_ref.py), and the refusals."""
import os

import numpy as np
import pytest
import torch

import cfgs
import loss_weight_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(num_train_timesteps=50, schedule="linear_beta", beta_start=0.01, beta_end=0.3)   # the small table of the GPU tests


def _sched(kw, pred="epsilon"):
    from ldm3d.schedulers import DDPMScheduler
    return DDPMScheduler(**kw, prediction_type=pred)


def test_known_answers_on_the_project_schedule():
    from ldm3d.loss_weighting import min_snr_weights
    sch = _sched(cfgs.SCHED)
    snr = ref.snr(sch.alphas_cumprod.numpy())
    assert 600 < snr[0] < 700 and 1e-4 < snr[-1] < 2e-4            # 666 down to 1.4e-4
    high = snr > 5.0
    assert int(high.sum()) == 95 and high[:95].all()                # the first 95 timesteps
    w = min_snr_weights(sch, 5.0).double().numpy()
    assert (w[~high] == 1.0).all()
    np.testing.assert_allclose(w[high], 5.0 / snr[high], rtol=1e-6)
    w_x0 = min_snr_weights(_sched(cfgs.SCHED, "sample"), 5.0).double().numpy()
    assert (w_x0[high] == 5.0).all()
    np.testing.assert_allclose(w_x0[~high], snr[~high], rtol=1e-6)
    w_v = min_snr_weights(_sched(cfgs.SCHED, "v_prediction"), 5.0).double().numpy()
    assert (w_v < 1.0).all() and (w_v > 0.0).all()


def test_the_schedule_restated_matches_the_scheduler():
    for kw in (cfgs.SCHED, SMALL):
        sch = _sched(kw)
        b = ref.betas(kw["num_train_timesteps"], kw["schedule"], kw["beta_start"], kw["beta_end"])
        np.testing.assert_allclose(np.cumprod(1.0 - b.astype(np.float64)), sch.alphas_cumprod.double().numpy(), rtol=1e-5)


def test_small_table_has_six_clamped_timesteps():
    snr = ref.snr(_sched(SMALL).alphas_cumprod.numpy())
    assert int((snr > 5.0).sum()) == 6


@pytest.mark.parametrize("kw", [cfgs.SCHED, SMALL], ids=["T1000", "T50"])
@pytest.mark.parametrize("pred", ["epsilon", "sample", "v_prediction"])
@pytest.mark.parametrize("gamma", [5.0, 1.0, 0.01])
def test_min_snr_weights_against_the_reference(kw, pred, gamma):
    """The only difference is the fp32 store (2^-24)."""
    from ldm3d.loss_weighting import min_snr_weights
    sch = _sched(kw, pred)
    got = min_snr_weights(sch, gamma)
    assert got.dtype == torch.float32 and got.device.type == "cpu" and got.shape == (kw["num_train_timesteps"],)
    want = ref.min_snr(sch.alphas_cumprod.numpy(), gamma, pred)
    rel = np.abs(got.double().numpy() - want) / np.abs(want)
    assert rel.max() <= 1e-6, rel.max()


@pytest.mark.parametrize("K,T", [(20, 1000), (7, 50), (50, 50), (1, 50), (64, 1000)])
def test_bin_arithmetic(K, T):
    from ldm3d.loss_weighting import LossTracker
    edges = ref.bin_edges(K, T)
    assert LossTracker(T, n_bins=K).bin_edges() == edges             # ceil(k T / K) against exhaustive membership
    n = [edges[k + 1] - edges[k] for k in range(K)]
    assert sum(n) == T and min(n) >= 1
    seen = np.zeros(T, dtype=int)
    for k in range(K):
        for t in range(edges[k], edges[k + 1]):
            assert ref.bin_of(t, K, T) == k
            seen[t] += 1
    assert (seen == 1).all()                                         # every t lies in exactly one bin


@pytest.mark.parametrize("K,T", [(20, 1000), (7, 50), (50, 50)])
def test_unbiasedness_identity(K, T):
    """sum_t p(t) iw(t) f(t) is the uniform mean of f; with f = 1: sum_t p(t) iw(t) = 1, to 1e-12 in fp64, in warm-up and after it."""
    rng = np.random.default_rng(K * 1000 + T)
    state = np.stack([rng.uniform(1e-4, 2.0, K) ** 2, np.full(K, 3.0)])
    f = rng.normal(size=T)
    for warmup in (10, 2):                                           # counts are 3: the first is warm-up, the second is not
        P, uniform = ref.bin_probabilities(state, K, T, warmup, 1e-3)
        assert uniform == (warmup == 10)
        assert abs(P.sum() - 1.0) <= 1e-12
        p, iw = ref.timestep_probability(P, K, T)
        assert abs(p.sum() - 1.0) <= 1e-12
        assert abs((p * iw).sum() - 1.0) <= 1e-12
        assert abs((p * iw * f).sum() - f.mean()) <= 1e-12
        if uniform:
            assert np.abs(iw - 1.0).max() <= 1e-15
    # the tracker's host-side probabilities are the reference's
    from ldm3d.loss_weighting import LossTracker
    tr = LossTracker(T, n_bins=K, warmup=2, uniform_prob=1e-3)
    tr.state.copy_(torch.from_numpy(state))
    np.testing.assert_allclose(tr.probabilities(), ref.bin_probabilities(tr.state.double().numpy(), K, T, 2, 1e-3)[0], rtol=1e-12)
    rows = tr.report()
    assert len(rows) == K and rows[0]["lo"] == 0 and rows[-1]["hi"] == T - 1 and sum(r["count"] for r in rows) == 3 * K


def test_degenerate_states_fall_back_to_uniform():
    K, T = 7, 50
    for m2 in (np.zeros(K), np.array([1.0, 2.0, np.inf, 1.0, 1.0, 1.0, 1.0]), np.array([1.0, -1.0, 1.0, 1.0, 1.0, 1.0, 1.0])):
        P, uniform = ref.bin_probabilities(np.stack([m2, np.full(K, 50.0)]), K, T, 10, 1e-3)
        assert uniform and abs(P.sum() - 1.0) <= 1e-12


def test_tracker_update_reference_is_order_dependent():
    K, T = 7, 50
    per, ts = np.array([1.0, 4.0, np.nan, 2.0]), np.array([3, 5, 10, 49])     # t = 3 and 5 share bin 0
    a = ref.tracker_update(np.zeros((2, K)), per, ts, K, T, 0.9)
    b = ref.tracker_update(np.zeros((2, K)), per, ts, K, T, 0.9, order=[3, 2, 1, 0])
    assert a[1].sum() == b[1].sum() == 3 and a[1, 0] == 2 and a[1, 6] == 1
    assert abs(a[0, 0] - 2.5) <= 1e-12 and abs(b[0, 0] - 14.5) <= 1e-12


def test_refusals():
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.loss_weighting import LossTracker, min_snr_weights, weighted_mse_loss
    from ldm3d.schedulers import RFlowScheduler
    from ldm3d.trainer import DiffusionTrainer
    from ldm3d import _lib
    with pytest.raises(NotImplementedError):
        min_snr_weights(RFlowScheduler(), 5.0)
    for g in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="gamma"):
            min_snr_weights(_sched(SMALL), g)
    inf = LatentDiffusionInferer(_sched(SMALL))
    lin = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="exclude"):
        DiffusionTrainer(lin, None, inf, lr=1e-4, loss_weighting="min_snr", loss_weights=torch.ones(50))
    with pytest.raises(ValueError, match="loss_weighting"):
        DiffusionTrainer(lin, None, inf, lr=1e-4, loss_weighting="p2")
    with pytest.raises(ValueError, match="timestep_sampling"):
        DiffusionTrainer(lin, None, inf, lr=1e-4, timestep_sampling="importance")
    with pytest.raises(ValueError, match="gamma"):
        DiffusionTrainer(lin, None, inf, lr=1e-4, loss_weighting="min_snr", snr_gamma=0.0)
    with pytest.raises(ValueError, match="entries"):
        DiffusionTrainer(lin, None, inf, lr=1e-4, loss_weights=torch.ones(49))
    rf = LatentDiffusionInferer(RFlowScheduler())
    for kw in (dict(loss_weighting="min_snr"), dict(timestep_sampling="loss_aware"), dict(loss_weights=torch.ones(1000))):
        with pytest.raises(NotImplementedError):
            DiffusionTrainer(lin, None, rf, lr=1e-4, **kw)
    for kw in (dict(n_bins=0), dict(n_bins=65), dict(beta=1.0), dict(uniform_prob=1.5), dict(warmup=-1)):
        with pytest.raises(ValueError):
            LossTracker(1000, **kw)
    with pytest.raises(ValueError):
        LossTracker(50, n_bins=51)
    with pytest.raises(_lib.LdmError, match="CUDA"):                 # no CPU fallback
        weighted_mse_loss(torch.zeros(1, 4), torch.zeros(1, 4), None)
    with pytest.raises(_lib.LdmError, match="CUDA"):
        LossTracker(50, n_bins=7).sample(2, torch.zeros(1))


def test_tracker_state_dict_round_trip():
    from ldm3d.loss_weighting import LossTracker
    a = LossTracker(50, n_bins=7, beta=0.8, warmup=3, uniform_prob=0.01)
    a.state.copy_(torch.arange(14, dtype=torch.float32).reshape(2, 7))
    b = LossTracker(50, n_bins=7)
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.state, b.state) and (b.beta, b.warmup, b.uniform_prob) == (0.8, 3, 0.01)
    with pytest.raises(ValueError):
        LossTracker(50, n_bins=5).load_state_dict(a.state_dict())


def test_new_entries_are_declared_and_exported():
    from ldm3d import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "ldm3d.h")).read()
    for name in ("ldm_op_weighted_mse_loss", "ldm_timestep_resample"):
        assert name + "(" in hdr and hasattr(L, name) and getattr(L, name).argtypes is not None, name
