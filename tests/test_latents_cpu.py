"""Known answers of the fp64 restatement of ldm_latent_batch (tests/latent_batch_ref.py), which the GPU tests gate the kernel against, and
the host-side logic of ldm3d.latents.LatentCache and of train_diffusion.py --cache-latents that needs no GPU."""
import os
import subprocess
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfgs                    # noqa: E402
import latent_batch_ref as R   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed=0, n=3, shape=(2, 3), idx=(2, 0, 2)):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    B = len(idx)
    return dict(mu_label=r(n, *shape), sigma_label=r(n, *shape).abs(), mu_image=r(n, *shape), sigma_image=r(n, *shape).abs(), idx=list(idx),
                e_label=r(B, *shape), e_image=r(B, *shape), noise=r(B, *shape),
                sqrt_a=torch.tensor([0.8, 0.6, 0.28][:B], dtype=torch.float64), sqrt_b=torch.tensor([0.6, 0.8, 0.96][:B], dtype=torch.float64))


def test_hand_computed_element():
    """One element by hand: mu 2, sigma 0.5, e 4 -> 4, times scale 0.25 -> z = 1; noisy = 0.8 * 1 + 0.6 * 3 = 2.6; v = 0.8 * 3 - 0.6 * 1 = 1.8;
    cond = -1 + 2 * 0.5 = 0 (never scaled)."""
    one = lambda v: torch.tensor([[v]], dtype=torch.float64)
    for pred, want in (("epsilon", 3.0), ("sample", 1.0), ("v_prediction", 1.8)):
        noisy, cond, target, z = R.latent_batch_ref(one(2.0), one(0.5), one(-1.0), one(2.0), [0], one(4.0), one(0.5), one(3.0),
                                                    torch.tensor([0.8], dtype=torch.float64), torch.tensor([0.6], dtype=torch.float64), 0.25, pred)
        assert float(z) == 1.0 and float(cond) == 0.0
        assert abs(float(noisy) - 2.6) < 1e-14 and abs(float(target) - want) < 1e-14, (pred, float(target))


def test_rows_follow_idx_and_a_zero_sigma_gives_the_scaled_mean():
    c = _case()
    c["sigma_label"] = torch.zeros_like(c["sigma_label"])
    noisy, cond, target, z = R.latent_batch_ref(**c, scale=0.7311, pred="sample")
    assert torch.equal(z, c["mu_label"][[2, 0, 2]] * 0.7311) and torch.equal(target, z)
    assert torch.equal(z[0], z[2])                                              # the repeated index: the same row twice
    assert torch.equal(cond, c["mu_image"][[2, 0, 2]] + c["sigma_image"][[2, 0, 2]] * c["e_image"])


def test_a_timestep_without_noise_leaves_the_latent():
    """sqrt_b = 0 (abar = 1): noisy = z, and the velocity is the noise."""
    c = _case(1)
    c["sqrt_a"], c["sqrt_b"] = torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    noisy, _, target, z = R.latent_batch_ref(**c, scale=1.0, pred="v_prediction")
    assert torch.equal(noisy, z) and torch.equal(target, c["noise"])


def test_v_target_is_get_velocity():
    """MONAI's Scheduler.get_velocity: sqrt(abar_t) noise - sqrt(1 - abar_t) sample with the scheduler's own table, on the scaled z."""
    from ldm3d.schedulers import DDPMScheduler
    sch = DDPMScheduler(**cfgs.SCHED, prediction_type="v_prediction")
    t = torch.tensor([0, 999, 417])
    abar = sch.alphas_cumprod.double()[t]
    c = _case(2)
    c["sqrt_a"], c["sqrt_b"] = abar ** 0.5, (1 - abar) ** 0.5
    noisy, _, target, z = R.latent_batch_ref(**c, scale=0.5, pred=2)
    a, s = (abar ** 0.5).reshape(3, 1, 1), ((1 - abar) ** 0.5).reshape(3, 1, 1)
    assert torch.allclose(target, a * c["noise"] - s * z, rtol=0, atol=1e-15)
    assert torch.allclose(noisy, a * z + s * c["noise"], rtol=0, atol=1e-15)
    # noisy and v are a rotation of (z, noise): z and the noise come back from them
    assert torch.allclose(a * noisy - s * target, z, rtol=0, atol=1e-12) and torch.allclose(s * noisy + a * target, c["noise"], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ LatentCache, host side
def _cpu_cache(n=5, shape=(2, 3, 4, 5)):
    from ldm3d.latents import LatentCache
    return LatentCache(*(torch.zeros((n,) + shape) for _ in range(4)))


def test_byte_accounting():
    from ldm3d import latents
    assert latents.cache_bytes(3, (8, 36, 44, 28)) == 4 * 4 * 3 * 8 * 36 * 44 * 28
    c = _cpu_cache()
    assert len(c) == 5 and c.latent_shape == (2, 3, 4, 5) and c.per_sample == 120 and c.nbytes == 16 * 5 * 120
    latents.check_fits(100, 200)                                                # exactly half is allowed
    with pytest.raises(MemoryError, match="101 bytes"):
        latents.check_fits(101, 200)
    with pytest.raises(ValueError):
        latents.LatentCache(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 4), torch.zeros(2, 3))


def test_random_crops_are_refused_before_anything_is_encoded():
    from ldm3d.data import PairVolumes
    from ldm3d.latents import LatentCache
    ds = PairVolumes(["a.npz", "b.npz"], (16, 16, 16), randcrop=True)
    with pytest.raises(ValueError, match="randcrop"):
        LatentCache.build(None, ds, "cpu")                                      # neither the autoencoder nor a file is touched


def test_index_validation():
    c = _cpu_cache(n=5)
    assert c.check_idx([4, 0, 4]) == [4, 0, 4] and c.check_idx(torch.tensor([1, 2])) == [1, 2]
    for bad in ([5], [-1], [0, 7, 1]):
        with pytest.raises(IndexError):
            c.check_idx(bad)
    for bad in ([], [0] * 65):
        with pytest.raises(ValueError):
            c.check_idx(bad)
    # batch() checks the indices and the draws before it needs a device
    sch = types.SimpleNamespace(prediction_type="epsilon")
    with pytest.raises(IndexError):
        c.batch([5], sch, torch.tensor([3]), 1.0)
    with pytest.raises(ValueError, match="together"):
        c.batch([1], sch, torch.tensor([3]), 1.0, noise=torch.zeros(1, 2, 3, 4, 5))


def test_batch_samplers_of_two_replicas_cover_the_set_disjointly(tmp_path):
    """--cache-latents iterates ``loader.batch_sampler`` instead of the loader: the same DistributedSampler shards, set_epoch reshuffles
    and drop_last holds, and no file is read for it."""
    from ldm3d.data import prepare_dataloader
    d = tmp_path / "pairs"
    d.mkdir()
    for i in range(9):
        (d / f"pair_{i:04d}.npz").write_bytes(b"")                            # never opened
    args = types.SimpleNamespace(npz_dir=str(d), val_fraction=0.0, seed=0)     # val = 1 file, train = 9
    per_rank = []
    for rank in (0, 1):
        train, _ = prepare_dataloader(args, 2, (16, 16, 16), rank=rank, world_size=2)
        assert train.batch_sampler.sampler is train.sampler
        epochs = []
        for epoch in (0, 1):
            train.sampler.set_epoch(epoch)
            batches = list(train.batch_sampler)
            assert all(len(b) == 2 and all(isinstance(i, int) for i in b) for b in batches)   # drop_last: no short batch
            epochs.append([i for b in batches for i in b])
        assert epochs[0] != epochs[1]                                           # set_epoch reaches the sampler behind batch_sampler
        per_rank.append(epochs)
    for epoch in (0, 1):
        a, b = per_rank[0][epoch], per_rank[1][epoch]
        # 9 samples on 2 replicas: the sampler pads to 10 (5 each), drop_last keeps 2 batches of 2 per rank
        assert len(a) == len(b) == 4 and not set(a) & set(b) and len(set(a) | set(b)) == 8
    n = 8                                                                       # an even set is covered completely
    for f in sorted(d.glob("*.npz"))[n:]:
        f.unlink()
    seen = []
    for rank in (0, 1):
        train, _ = prepare_dataloader(types.SimpleNamespace(npz_dir=str(d), val_fraction=0.0, seed=0), 2, (16, 16, 16), rank=rank, world_size=2)
        seen.append([i for b in train.batch_sampler for i in b])
    assert not set(seen[0]) & set(seen[1]) and sorted(seen[0] + seen[1]) == list(range(n))


def test_cache_latents_flag_and_its_exclusion():
    """train_diffusion.py --cache-latents exists and refuses --reference-rng-order with a message, before anything is loaded."""
    script = os.path.join(ROOT, "train_diffusion.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--cache-latents" in r.stdout
    r = subprocess.run([sys.executable, script, "--cache-latents", "--reference-rng-order"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--cache-latents and --reference-rng-order exclude each other" in r.stderr
