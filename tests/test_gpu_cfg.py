"""Classifier-free guidance for concat conditioning on the GPU (-m gpu): the combine kernel against fp64 (tests/cfg_ref.py), the guided
device step against the unfused chain (UNet forward at batch 2 B on torch.cat-built inputs -> ldm_guidance_combine -> sampler step) bit for
bit, the fp64 oracle composition under the model-level gates, the graph-replay key, refusals, the inferer's two loops, sliding windows,
the condition-dropout kernel against its Python mirror, and the trainer against a by-hand replay.

UNET_TINY_COND (4 + 4 input channels) at 8^3 with seeded non-zero weights; one module per precision, shared by the tests."""
import ctypes as C
import functools

import pytest
import torch

import cfg_ref
import cfgs
from util import rel_l2

pytestmark = pytest.mark.gpu
BAD_ARG = -1                                                            # LDM_ERR_BAD_ARG, include/ldm3d.h
SHAPE = (4, 8, 8, 8)


@functools.lru_cache(maxsize=None)
def _unet(precision="bf16"):
    from ldm3d.networks import DiffusionModelUNet
    from oracle import unet as ou
    m = DiffusionModelUNet(**cfgs.UNET_TINY_COND)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfgs.UNET_TINY_COND), 3))
    m = m.to(torch.device("cuda:0")).eval()
    m.set_precision(precision)
    return m


def _sched(kind):
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler, PNDMScheduler, RFlowScheduler
    if kind == "ddpm":
        return DDPMScheduler(**dict(cfgs.SCHED, num_train_timesteps=5))
    if kind == "ddim":
        sch = DDIMScheduler(**cfgs.SCHED)
        sch.set_timesteps(4)
        return sch
    if kind == "pndm":
        sch = PNDMScheduler(**cfgs.SCHED, skip_prk_steps=True, set_alpha_to_one=True)
        sch.set_timesteps(5)
        return sch
    sch = RFlowScheduler()
    sch.set_timesteps(4, input_img_size_numel=8 ** 3)
    return sch


def _inputs(B, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn((B,) + SHAPE, device=dev, generator=g), torch.randn((B,) + SHAPE, device=dev, generator=g)


def _combine(u, c, w, out=None):
    from ldm3d import _lib
    out = torch.empty_like(u) if out is None else out
    with torch.cuda.device(u.device):
        _lib.check(_lib.lib().ldm_guidance_combine(u.data_ptr(), c.data_ptr(), float(w), out.data_ptr(), u.numel(), _lib.current_stream()))
    return out


# ---- 1. the combine kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4098])
def test_combine_matches_fp64(cuda, n):
    """|err| <= 4 * 2^-24 * (|u| + |w| |c - u|) per element: one rounding of c - u scaled by w, plus one of the fused multiply-add.  Aligned
    (quads + tail) and unaligned (all scalar) pointers; out aliasing u; w = 0 returns u bit for bit."""
    g = torch.Generator(device=cuda).manual_seed(100 + n)
    for off in (0, 1):                                                  # off 1: pointers 4 bytes past a 16-byte boundary
        ub, cb = torch.randn((n + 1,), device=cuda, generator=g), torch.randn((n + 1,), device=cuda, generator=g)
        u, c = ub[off:off + n], cb[off:off + n]
        for w in (0.0, 1.0, 3.5, -0.5):
            got = _combine(u, c, w)
            ref = cfg_ref.combine(u.cpu(), c.cpu(), w)
            bound = 4 * 2.0 ** -24 * (u.cpu().double().abs() + abs(w) * (c.cpu().double() - u.cpu().double()).abs())
            err = (got.cpu().double() - ref).abs()
            print(f"combine n={n} off={off} w={w}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
            assert bool((err <= bound).all()), (n, off, w, float(err.max()))
            alias = u.clone()
            _combine(alias, c, w, out=alias)
            assert torch.equal(alias, got)
            if w == 0.0:
                assert torch.equal(got, u)
    from ldm3d import _lib
    L = _lib.lib()
    assert L.ldm_guidance_combine(None, c.data_ptr(), 1.0, u.data_ptr(), n, None) == BAD_ARG
    assert L.ldm_guidance_combine(u.data_ptr(), c.data_ptr(), 1.0, c.data_ptr(), n, None) == BAD_ARG      # out may alias u, not c


# ---- 2. the guided step == the unfused chain ------------------------------------------------------------------------------------
def _unfused_chain(m, sch, smp, x0, cond, w, fill, host_noise=False):
    """forward at 2 B on torch.cat-built inputs with an explicit fill tensor -> ldm_guidance_combine -> sampler step."""
    B = x0.shape[0]
    x, tbuf = x0.clone(), torch.empty((2 * B,), device=x0.device)
    smp.reset(tbuf)
    ts = sch.timesteps.tolist()
    xh = x0.clone()                                                     # DDPM: the host-driven scheduler on the sampler's own draws
    for k in range(smp.n_steps):
        out = m(x=torch.cat([x, x]), timesteps=tbuf, context=None, cond=torch.cat([torch.full_like(cond, fill), cond]))
        guided = _combine(out[:B], out[B:], w)
        if host_noise:
            assert torch.equal(xh, x)
            t = int(ts[k])
            xh, _ = sch.step(guided, t, xh, noise=smp.noise(k, x.shape, x.device) if t > 0 else None)
        smp.step(guided, x, tbuf)
    if host_noise:
        assert torch.equal(xh, x)
    return x


def _fused_chain(m, smp, x0, cond, w, fill, x=None, tbuf=None):
    B = x0.shape[0]
    x = torch.empty_like(x0) if x is None else x
    tbuf = torch.empty((2 * B,), device=x0.device) if tbuf is None else tbuf
    x.copy_(x0)
    smp.reset(tbuf)
    for k in range(smp.n_steps):
        assert tbuf.tolist() == [float(smp.timesteps[k])] * (2 * B), k   # the next t in all 2 B entries
        m.denoise_step(x, tbuf, smp, cond=cond, guidance=w, guidance_fill=fill)
    assert tbuf.tolist() == [float(smp.timesteps[-1])] * (2 * B)
    return x.clone()


@pytest.mark.parametrize("kind,B,precision", [("ddpm", 1, "bf16"), ("ddim", 2, "bf16"), ("pndm", 2, "fp32"), ("rflow", 1, "fp32"),
                                              ("ddim", 1, "fp32"), ("pndm", 1, "bf16")])
def test_guided_step_equals_the_unfused_chain(cuda, kind, B, precision):
    m = _unet(precision)
    sch = _sched(kind)
    x0, cond = _inputs(B, 7, cuda)
    w, fill = 3.5, -1.0
    with torch.no_grad():
        m.enable_graph_replay(False)
        want = _unfused_chain(m, sch, sch.device_sampler(5), x0, cond, w, fill, host_noise=kind == "ddpm")
        assert torch.isfinite(want).all() and not torch.equal(want, x0)
        eager = _fused_chain(m, sch.device_sampler(5), x0, cond, w, fill)
        assert torch.equal(eager, want), rel_l2(eager, want)
        m.enable_graph_replay(True)
        try:
            smp = sch.device_sampler(5)
            x, tbuf = torch.empty_like(x0), torch.empty((2 * B,), device=cuda)
            for _ in range(3):                                          # eager first sight, capture, then replays on a rewound counter
                got = _fused_chain(m, smp, x0, cond, w, fill, x=x, tbuf=tbuf)
                assert torch.equal(got, want), rel_l2(got, want)
            unfused_graph = _unfused_chain(m, sch, sch.device_sampler(5), x0, cond, w, fill)
            assert torch.equal(unfused_graph, want)
        finally:
            m.enable_graph_replay(False)
    if kind == "pndm":
        assert smp.state_numel(x0.numel()) == 6 * x0.numel() and smp._state_n == x0.numel()   # the state of B samples, not 2 B


# ---- 3. the fp64 oracle composition under the model-level gates ------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_guided_output_matches_the_oracle_composition(cuda, precision):
    """MONAI's doubled-batch call through oracle/unet.py, combined in fp64, against forward(2 B) -> ldm_guidance_combine (which test 2 shows
    to be the guided step's model output bit for bit).  Gates: tests/test_gpu_models.py's floor gate for bf16, tests/test_gpu_fp32.py's
    1e-3 for fp32."""
    from oracle import unet as ou
    from test_gpu_fp32 import TOL
    from test_gpu_models import floor_gate
    cfg = cfgs.UNET_TINY_COND
    sd = ou.init_state_dict(ou.unet_param_shapes(cfg), 3)
    m = _unet(precision)
    x, cond = (t.cpu() for t in _inputs(2, 11, cuda))
    t = torch.tensor([37.0, 911.0])
    w, fill = 2.0, -1.0
    with torch.no_grad():
        xx, tt, cc = cfg_ref.doubled_inputs(x, t, cond, fill)
        out = m(x=xx.to(cuda), timesteps=tt.to(cuda), context=None, cond=cc.to(cuda))
        got = _combine(out[:2], out[2:], w).cpu()
    oracle = lambda bf: cfg_ref.guided_output(lambda a, b, c: ou.unet_forward(sd, cfg, torch.cat([a, c], 1), b, emulate_bf16=bf),
                                              x, t, cond, w, fill).float()
    ref32 = oracle(False)
    if precision == "fp32":
        e = rel_l2(got, ref32)
        print(f"guided output, fp32 mode vs fp32 oracle: {e:.2e}")
        assert e <= TOL, e
    else:
        floor_gate(got, oracle(True), ref32, "guided concat-conditioned UNet, w = 2")


# ---- 4. / 5. exact zero difference; the graph key --------------------------------------------------------------------------------
def test_cond_equal_to_the_fill_tensor_ignores_the_scale(cuda):
    """cond == the fill tensor: both halves see the same input, c - u is exactly 0, so w = 3.5 gives the w = 0 chain bit for bit."""
    m = _unet("bf16")
    sch = _sched("ddim")
    x0, _ = _inputs(2, 13, cuda)
    cond = torch.full_like(x0, -1.0)
    with torch.no_grad():
        a = _fused_chain(m, sch.device_sampler(), x0, cond, 3.5, -1.0)
        b = _fused_chain(m, sch.device_sampler(), x0, cond, 0.0, -1.0)
        assert torch.equal(a, b) and torch.isfinite(a).all()
        c = _fused_chain(m, sch.device_sampler(), x0, cond, 3.5, 0.5)   # another fill: the halves differ again
        assert not torch.equal(a, c)


def test_scale_and_fill_are_part_of_the_graph_key(cuda):
    m = _unet("bf16")
    sch = _sched("ddim")
    x0, cond = _inputs(1, 17, cuda)
    with torch.no_grad():
        m.enable_graph_replay(False)
        eager = {(w, f): _fused_chain(m, sch.device_sampler(), x0, cond, w, f) for w, f in ((1.5, -1.0), (4.0, -1.0), (4.0, 0.25))}
        assert len({tuple(v.flatten()[:64].tolist()) for v in eager.values()}) == 3
        m.enable_graph_replay(True)
        try:
            smp = sch.device_sampler()
            x, tbuf = torch.empty_like(x0), torch.empty((2,), device=cuda)
            for key in ((1.5, -1.0), (4.0, -1.0), (4.0, 0.25), (1.5, -1.0)):   # same pointers, same sampler: only (w, fill) tell the recordings apart
                got = _fused_chain(m, smp, x0, cond, *key, x=x, tbuf=tbuf)
                assert torch.equal(got, eager[key]), key
        finally:
            m.enable_graph_replay(False)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(cuda):
    from ldm3d import _lib
    L = _lib.lib()
    m = _unet("bf16")
    x, cond = _inputs(1, 19, cuda)
    keep = x.clone()
    tbuf = torch.empty((2,), device=cuda)
    nbytes = L.ldm_unet_guided_workspace_bytes(m._h, 1, 8, 8, 8)
    assert nbytes > 0 and L.ldm_unet_guided_workspace_bytes(m._h, 0, 8, 8, 8) == 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=cuda)
    scratch = torch.full((2,) + SHAPE, 7.0, device=cuda)

    def raw(smp, cond_ptr, cc):
        return L.ldm_unet_denoise_step_guided(m._h, smp._h, x.data_ptr(), 4, cond_ptr, cc, 2.0, -1.0, tbuf.data_ptr(), scratch.data_ptr(),
                                              1, 8, 8, 8, ws.data_ptr(), ws.numel(), _lib.current_stream())
    ddim = _sched("ddim").device_sampler()
    ddim.reset(tbuf)
    first_t = tbuf.tolist()
    assert raw(ddim, None, 4) == BAD_ARG and b"condition" in L.ldm_last_error()
    assert raw(ddim, cond.data_ptr(), 0) == BAD_ARG
    pndm = _sched("pndm").device_sampler()
    pndm.bind_state(torch.empty((6 * 2 * x.numel(),), device=cuda), 2 * x.numel())    # bound for the doubled batch: the step has B samples
    assert raw(pndm, cond.data_ptr(), 4) == BAD_ARG and b"bound for" in L.ldm_last_error()
    with pytest.raises(ValueError, match="2 B"):
        m.denoise_step(x, tbuf[:1], ddim, cond=cond, guidance=2.0)
    with pytest.raises(_lib.LdmError):
        m.denoise_step(x, tbuf, ddim, cond=None, guidance=2.0)
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and bool((scratch == 7.0).all()) and tbuf.tolist() == first_t


# ---- 7. / 8. the inferer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddim", "pndm", "rflow"])
def test_inferer_fused_equals_host_driven(cuda, kind):
    from ldm3d.inferer import LatentDiffusionInferer
    m = _unet("bf16")
    inf = LatentDiffusionInferer(_sched(kind))
    noise, cond = _inputs(2, 23, cuda)
    with torch.no_grad():
        fused = inf.sample(noise, None, m, conditioning=cond, mode="concat", fused_seed=0, cfg=2.0)
        host = inf.sample(noise, None, m, conditioning=cond, mode="concat", cfg=2.0)
        plain = inf.sample(noise, None, m, conditioning=cond, mode="concat", fused_seed=0)
        other = inf.sample(noise, None, m, conditioning=cond, mode="concat", fused_seed=0, cfg=2.0, cfg_fill_value=0.0)
    assert torch.equal(fused, host), rel_l2(fused, host)
    assert torch.isfinite(fused).all() and not torch.equal(fused, plain) and not torch.equal(fused, other)
    if kind == "ddim":                                                  # step_noise keeps working (all-zero draws at eta = 0)
        with torch.no_grad():
            sn = inf.sample(noise, None, m, conditioning=cond, mode="concat", cfg=2.0, step_noise=lambda t: torch.zeros_like(noise))
        assert torch.equal(sn, host)


@pytest.mark.parametrize("kind,sw", [("ddim", 1), ("ddim", 2), ("pndm", 1), ("rflow", 2)])
def test_sliding_window_fused_equals_host_driven(cuda, kind, sw):
    """Latent 1 x 4 x 12 x 8 x 8, windows of 8^3 (two), one or both per UNet call."""
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.sliding import WindowGrid
    m = _unet("bf16")
    inf = LatentDiffusionInferer(_sched(kind))
    g = torch.Generator(device=cuda).manual_seed(29)
    noise = torch.randn((1, 4, 12, 8, 8), device=cuda, generator=g)
    cond = torch.randn((1, 4, 12, 8, 8), device=cuda, generator=g)
    assert WindowGrid((12, 8, 8), 8).n_windows == 2
    with torch.no_grad():
        fused = inf.sample_sliding_window(noise, None, m, (8, 8, 8), sw_batch_size=sw, conditioning=cond, fused_seed=0, cfg=2.0)
        host = inf.sample_sliding_window(noise, None, m, (8, 8, 8), sw_batch_size=sw, conditioning=cond, cfg=2.0)
        plain = inf.sample_sliding_window(noise, None, m, (8, 8, 8), sw_batch_size=sw, conditioning=cond, fused_seed=0)
    assert torch.equal(fused, host), rel_l2(fused, host)
    assert torch.isfinite(fused).all() and not torch.equal(fused, plain)


def test_one_window_covering_the_latent_equals_sample(cuda):
    from ldm3d.inferer import LatentDiffusionInferer
    m = _unet("bf16")
    inf = LatentDiffusionInferer(_sched("ddim"))
    noise, cond = _inputs(1, 31, cuda)
    with torch.no_grad():
        m.enable_graph_replay(True)
        try:
            a = inf.sample_sliding_window(noise, None, m, (8, 8, 8), conditioning=cond, fused_seed=0, cfg=2.0)
        finally:
            m.enable_graph_replay(False)
        b = inf.sample(noise, None, m, conditioning=cond, mode="concat", fused_seed=0, cfg=2.0)
    assert torch.equal(a, b), rel_l2(a, b)


# ---- 9. condition dropout --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_sample", [1, 5, 512])
def test_cond_dropout_matches_the_mirror(cuda, per_sample):
    from ldm3d.latents import cond_dropout
    seed, step, p, fill = 0x1234567890ABCDEF, 9, 0.3, -1.0
    idx = torch.randperm(1000, generator=torch.Generator().manual_seed(1))[:64].tolist()
    want = cfg_ref.drop_mask(seed, step, idx, p)
    assert 5 <= sum(want) <= 40                                         # 19.2 +- 3.7: a real mixture
    g = torch.Generator(device=cuda).manual_seed(per_sample)
    src = torch.randn((64, per_sample), device=cuda, generator=g)
    cond = src.clone()
    got = cond_dropout(cond, p, fill, idx=idx, seed=seed, step=step)
    assert got == want
    wm = torch.tensor(want, device=cuda)
    assert bool((cond[wm] == fill).all()) and torch.equal(cond[~wm], src[~wm])      # dropped: all fill; kept: bit-unchanged
    # the same dataset indices in other slots and at B = 3: the same decisions
    pick = [10, 3, 40]
    c3 = src[:3].clone()
    assert cond_dropout(c3, p, fill, idx=[idx[i] for i in pick], seed=seed, step=step) == [want[i] for i in pick]
    # idx None means 0 .. B-1
    c4 = src[:7].clone()
    assert cond_dropout(c4, p, fill, seed=seed, step=step) == cfg_ref.drop_mask(seed, step, range(7), p)
    # p = 0 and p = 1
    c0 = src.clone()
    assert cond_dropout(c0, 0.0, fill, idx=idx, seed=seed, step=step) == [False] * 64 and torch.equal(c0, src)
    c1 = src.clone()
    assert cond_dropout(c1, 1.0, 0.25, idx=idx, seed=seed, step=step) == [True] * 64 and bool((c1 == 0.25).all())
    # mask_in overrides the draw
    mask = [b % 3 == 0 for b in range(64)]
    cm = src.clone()
    assert cond_dropout(cm, 0.0, fill, idx=idx, seed=seed, step=step, mask=mask) == mask
    mm = torch.tensor(mask, device=cuda)
    assert bool((cm[mm] == fill).all()) and torch.equal(cm[~mm], src[~mm])
    # an unaligned base pointer takes the scalar stores
    if per_sample == 5:
        buf = torch.zeros((64 * 5 + 1,), device=cuda)
        view = buf[1:].view(64, 5)
        view.copy_(src)
        assert cond_dropout(view, p, fill, idx=idx, seed=seed, step=step) == want and torch.equal(view, cond) and float(buf[0]) == 0.0


def test_cond_dropout_refusals(cuda):
    from ldm3d import _lib
    L = _lib.lib()
    cond = torch.randn((64, 8), device=cuda)
    keep = cond.clone()
    out = (C.c_ubyte * 64)()
    call = lambda ptr, B, per, idx, p: L.ldm_cond_dropout(ptr, B, per, idx, p, -1.0, None, 1, 0, out, None)
    assert call(cond.data_ptr(), 0, 8, None, 1.0) == BAD_ARG
    assert call(cond.data_ptr(), 65, 8, None, 1.0) == BAD_ARG
    assert call(cond.data_ptr(), 64, 8, None, -0.1) == BAD_ARG
    assert call(cond.data_ptr(), 64, 8, None, 1.5) == BAD_ARG
    assert call(cond.data_ptr(), 64, 8, None, float("nan")) == BAD_ARG
    assert call(None, 64, 8, None, 1.0) == BAD_ARG
    assert call(cond.data_ptr(), 64, 0, None, 1.0) == BAD_ARG
    assert call(cond.data_ptr(), 2, 8, (C.c_int * 2)(3, -1), 1.0) == BAD_ARG and b"negative" in L.ldm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(cond, keep)


# ---- 10. the trainer -------------------------------------------------------------------------------------------------------------
VCFG = dict(cfgs.VAE_TINY, in_channels=1, out_channels=1, latent_channels=4)     # 4 latent channels: UNET_TINY_COND takes 4 + 4
PATCH, LATENT = (16, 16, 16), (4, 4, 4, 4)
SEED = 3                                                                # gives mixed decisions on both paths (asserted below)


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
    from ldm3d.latents import LatentCache
    from ldm3d.networks import AutoencoderKL
    from oracle import autoencoder as oa, unet as ou
    vae = AutoencoderKL(**VCFG)
    vae.load_state_dict(ou.init_state_dict(oa.ae_param_shapes(VCFG), 2))
    vae = vae.to(cuda).eval()
    pairs = _Pairs()
    return vae, pairs, LatentCache.build(vae, pairs, cuda)


def _trainer(cuda, vae, p, fill=-1.0):
    from ldm3d.inferer import LatentDiffusionInferer
    from ldm3d.networks import DiffusionModelUNet
    from ldm3d.schedulers import DDPMScheduler
    from ldm3d.trainer import DiffusionTrainer
    from oracle import unet as ou
    unet = DiffusionModelUNet(**cfgs.UNET_TINY_COND)
    unet.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfgs.UNET_TINY_COND), 3, gain=0.5))
    tr = DiffusionTrainer(unet.to(cuda), vae, LatentDiffusionInferer(DDPMScheduler(**cfgs.SCHED), scale_factor=0.7311), lr=1e-4,
                          cond_drop_prob=p, cfg_fill_value=fill)
    tr.cache_seed = SEED
    return tr


def _manual_step(tr, noisy, cond, target, ts):
    from ldm3d.optim import mse_loss
    tr.unet.train()
    tr.optimizer.zero_grad(set_to_none=True)
    loss = mse_loss(tr.unet(x=noisy, timesteps=ts, context=None, cond=cond), target)
    loss.backward()
    tr.optimizer.step()
    return loss.detach()


def _overwrite(cond, mask, fill):
    cond = cond.clone()
    cond[torch.tensor(mask, device=cond.device)] = fill
    return cond


@pytest.mark.parametrize("p", [0.5, 0.0])
def test_trainer_uncached_equals_the_replay(cuda, world, p):
    """Two steps against a second trainer (cond_drop_prob = 0) that walks them by hand with the condition overwritten by torch where the
    mirror's mask says so; p = 0 is today's trainer.  Key: (cache_seed, timestep_draws) and rank * B + slot, rank 0 here."""
    vae, pairs, _ = world
    tr, by_hand = _trainer(cuda, vae, p, fill=-0.75), _trainer(cuda, vae, 0.0)
    sch = by_hand.inferer.scheduler
    images = torch.stack([pairs[0]["image"], pairs[2]["image"]]).to(cuda)
    labels = torch.stack([pairs[0]["label"], pairs[2]["label"]]).to(cuda)
    g = torch.Generator().manual_seed(3)
    masks = [cfg_ref.drop_mask(SEED, k, [0, 1], p) for k in range(2)]
    assert (any(any(m) for m in masks) and not all(all(m) for m in masks)) if p else not any(any(m) for m in masks)
    for k, ts in enumerate(([5, 613], [999, 250])):
        noise = torch.randn((2,) + LATENT, generator=g).to(cuda)
        ts = torch.tensor(ts, device=cuda)
        torch.manual_seed(11 + k)
        loss, skipped = tr.train_step(images, labels, noise=noise, timesteps=ts)
        torch.manual_seed(11 + k)
        with torch.no_grad():
            cond = _overwrite(vae.encode_stage_2_inputs(images), masks[k], -0.75)
            z = vae.encode_stage_2_inputs(labels) * by_hand.inferer.scale_factor
        noisy, target = sch.add_noise_and_target(original_samples=z, noise=noise, timesteps=ts)
        want = _manual_step(by_hand, noisy, cond, target, ts)
        assert not bool(skipped) and float(loss) == float(want) and float(loss) > 0
        assert torch.equal(tr.unet.flat_params, by_hand.unet.flat_params), k
    assert tr.timestep_draws == (2 if p else 0)


@pytest.mark.parametrize("p", [0.5, 0.0])
def test_trainer_cached_equals_the_replay(cuda, world, p):
    """train_step_cached on the same terms; key: (cache_seed, cached_steps) and the dataset indices.  Validation never drops."""
    vae, _, cache = world
    tr, by_hand = _trainer(cuda, vae, p), _trainer(cuda, vae, 0.0)
    sch = by_hand.inferer.scheduler
    g = torch.Generator(device=cuda).manual_seed(8)
    steps = (([2, 0], [5, 613]), ([1, 0], [999, 250]))
    masks = [cfg_ref.drop_mask(SEED, k, idx, p) for k, (idx, _) in enumerate(steps)]
    assert (any(any(m) for m in masks) and not all(all(m) for m in masks)) if p else not any(any(m) for m in masks)
    for k, (idx, ts) in enumerate(steps):
        e_l, e_i, noise = (torch.randn((2,) + LATENT, device=cuda, generator=g) for _ in range(3))
        ts = torch.tensor(ts, device=cuda)
        loss, skipped = tr.train_step_cached(cache, idx, noise=noise, timesteps=ts, eps_label=e_l, eps_image=e_i)
        noisy, cond, target = cache.batch(idx, sch, ts, by_hand.inferer.scale_factor, eps_label=e_l, eps_image=e_i, noise=noise)
        want = _manual_step(by_hand, noisy, _overwrite(cond, masks[k], -1.0), target, ts)
        assert not bool(skipped) and float(loss) == float(want) and float(loss) > 0
        assert torch.equal(tr.unet.flat_params, by_hand.unet.flat_params), k
    assert tr.cached_steps == 2
    if p:
        torch.manual_seed(5)                                            # the validation timesteps are the device torch.randint's
        a = _trainer(cuda, vae, 1.0).validate_cached(cache, [[0, 1], [2]])      # fresh trainers: the same weights and validation key
        torch.manual_seed(5)
        b = _trainer(cuda, vae, 0.0).validate_cached(cache, [[0, 1], [2]])
        assert a == b and 0 < a < float("inf")                         # cond_drop_prob = 1 would have changed every batch


# ---- the two command lines -------------------------------------------------------------------------------------------------------
def _env(tmp_path, **extra):
    import json
    env = {"data_base_dir": str(tmp_path / "data"), "npz_dir": str(tmp_path / "pairs"), "val_fraction": 0.25, "model_dir": str(tmp_path / "ckpt"),
           "tfevent_path": str(tmp_path / "tfevent"), "output_dir": str(tmp_path / "out"), "resume_ckpt": False, "seed": 0, **extra}
    env_file = str(tmp_path / "environment.json")
    with open(env_file, "w") as fh:
        json.dump(env, fh)
    return env_file


def test_inference_cli_samples_with_cfg(tmp_path):
    """inference.py --cfg 2 --condition pair.npz, the central patch and (--sliding-window) the whole scan: one finite volume each."""
    import os
    import subprocess
    import sys
    import numpy as np
    from ldm3d.data import write_synthetic_pairs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pair = write_synthetic_pairs(str(tmp_path / "pairs"), 1, (100, 96, 120))[0]
    base = [sys.executable, os.path.join(root, "inference.py"), "-e", _env(tmp_path), "-c", os.path.join(root, "config", "config_synthetic_train.json"),
            "-n", "1", "--random-init", "--steps", "3", "--condition", pair]
    vols = {}
    for name, extra in (("cfg", ["--cfg", "2.0"]), ("sw-cfg", ["--cfg", "2.0", "--cfg-fill-value", "0", "--sliding-window"])):
        r = subprocess.run(base + extra, cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (name, r.stdout[-2000:] + r.stderr[-2000:])
        out = sorted((tmp_path / "out").glob("*.nii"))
        assert len(out) == 1, name
        vols[name] = np.fromfile(out[0], dtype=np.float32, offset=352)
        out[0].unlink()
        assert np.isfinite(vols[name]).all() and float(vols[name].std()) > 0.0, name
    assert vols["cfg"].size == 96 ** 3
    assert vols["sw-cfg"].size == 100 * 96 * 120


def test_train_cli_drops_conditions_and_samples_with_cfg(tmp_path):
    """train_diffusion.py --cond-drop-prob 0.5 --sample-cfg 2 --sample-steps 4 from the latent cache: finite losses, the checkpoints, a
    guided periodic sample (the uncached step is test_trainer_uncached_equals_the_replay's)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for extra in (["--cache-latents"],):
        cmd = [sys.executable, os.path.join(root, "train_diffusion.py"), "-e", _env(tmp_path), "-c",
               os.path.join(root, "config", "config_synthetic_train.json"), "--random-init", "--synthetic", "4", "--max-steps", "3",
               "--cond-drop-prob", "0.5", "--sample-cfg", "2.0", "--sample-steps", "4"] + extra
        r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
        log = r.stdout + r.stderr
        assert r.returncode == 0, log[-3000:]
        assert os.path.exists(tmp_path / "ckpt" / "diffusion_unet_last.pt")
        assert "NaN loss" not in log and "conditional sample (4 steps" in log, log[-3000:]
        rows = [json.loads(line) for line in open(tmp_path / "tfevent" / "diffusion" / "scalars.jsonl")]
        losses = [x["value"] for x in rows if x["tag"] == "train_diffusion_loss_iter"]
        assert len(losses) >= 3 and all(v == v and 0 < v < float("inf") for v in losses)
    bad = subprocess.run(cmd[:-1] + ["--cond-drop-prob", "1.5"], cwd=root, capture_output=True, text=True, timeout=600)
    assert bad.returncode == 2 and "--cond-drop-prob" in bad.stderr
