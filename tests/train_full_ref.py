"""Full-width training-step fixtures (tests/golden/train_step_full_24.pt, train_step_cfg3_latent.pt, vae_train_step_full_{64,48}.pt):
the seeded cases, the fixture format and the comparer that gates a {name: gradient} dict against a loaded fixture.

The CPU oracle needs 10 s to minutes for one of these steps, so tests/golden/make_golden.py runs it once (torch autograd, fp32 and
bf16-emulating) and stores per parameter tensor: the norm of both gradients, ``floor`` = rel-L2 of the bf16-emulated gradient
against the fp32 one over the WHOLE tensor, and the fp32 gradient at K = 256 seeded flat indices (the whole tensor where it has no
more elements).  tests/test_gpu_train_full.py compares the HIP backward plans against that tensor by tensor;
tests/test_train_full_cpu.py proves on a synthetic fixture that the comparer bites.

A sampled rel-L2 over 128 indices was measured at 0.53 - 1.33 x the full-tensor value, over 512 at 0.81 - 1.24 x; that spread is
what the factor 2.5 of the per-tensor gate absorbs.
"""
import torch

import cfgs

K_SAMPLES = 256
EXEMPT_FLOOR = 0.1          # tensors whose own bf16-vs-fp32 floor is above this carry no relative information (true gradient zero)
MAX_EXEMPT = 11             # ... and only the attention to_k.bias tensors may be among them: 11 attention blocks in the benchmark UNet

# name -> (kind, model kwargs, spatial dims, weight seed, input seed, index seed, timestep)
CASES = {
    "train_step_full_24": ("unet", cfgs.UNET_FULL, (24, 24, 24), 41, 42, 43, 417.0),
    # diffusion_def of config_train_16g.json the way the configs[3] benchmark leg runs it: in 8 (4 latent + 4 concatenated condition), out 4
    "train_step_cfg3_latent": ("unet", dict(cfgs.REF_CONFIGS["config_train_16g"]["unet"], out_channels=4), (36, 44, 28), 44, 45, 46, 417.0),
    "vae_train_step_full_64": ("vae", cfgs.VAE_FULL, (64, 64, 64), 47, 48, 49, None),
    "vae_train_step_full_48": ("vae", cfgs.VAE_FULL, (48, 48, 48), 50, 51, 52, None),
}
KL_WEIGHT = 1e-3


def case_inputs(case):
    """Seeded weights and inputs of one case: unet -> (cfg, sd, x [1, in, D, H, W] (latent then condition channels), t, target),
    vae -> (cfg, sd, x, eps)."""
    from oracle import autoencoder as oa
    from oracle import unet as ou
    kind, cfg, dims, wseed, iseed, _, t = CASES[case]
    g = torch.Generator().manual_seed(iseed)
    if kind == "unet":
        sd = ou.init_state_dict(ou.unet_param_shapes(cfg), wseed, gain=0.5)
        x = torch.randn((1, cfg["in_channels"], *dims), generator=g)
        target = torch.randn((1, cfg["out_channels"], *dims), generator=g)
        return cfg, sd, x, torch.tensor([t]), target
    sd = ou.init_state_dict(oa.ae_param_shapes(cfg), wseed, gain=0.7)
    x = torch.rand((1, cfg["in_channels"], *dims), generator=g)
    f = 2 ** (len(cfg["channels"]) - 1)
    eps = torch.randn((1, cfg["latent_channels"], *[d // f for d in dims]), generator=g)
    return cfg, sd, x, eps


def sample_indices(numels, seed, k=K_SAMPLES):
    """One flat index tensor per parameter tensor, in order: the whole tensor where numel <= k, else k seeded draws."""
    g = torch.Generator().manual_seed(seed)
    return [torch.arange(n) if n <= k else torch.randint(0, n, (k,), generator=g) for n in numels]


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def build_fixture(g32, gbf, index_seed, k=K_SAMPLES, **extra):
    """{name: fp32 gradient}, {name: bf16-emulated gradient} (same key order) -> the fixture dict (plain tensors / lists / floats)."""
    names = list(g32.keys())
    numels = [g32[n].numel() for n in names]
    idx = sample_indices(numels, index_seed, k)
    a32 = [g32[n].detach().reshape(-1).double() for n in names]
    abf = [gbf[n].detach().reshape(-1).double() for n in names]
    tot32 = torch.cat(a32)
    out = dict(names=names, numel=torch.tensor(numels), index_seed=index_seed, k=k,
               norm_fp32=torch.stack([v.norm() for v in a32]), norm_bf16=torch.stack([v.norm() for v in abf]),
               floor=torch.tensor([_rel(b, a) for a, b in zip(a32, abf)], dtype=torch.float64),
               samples=torch.cat([v[i] for v, i in zip(a32, idx)]).float(),
               total_grad_norm_fp32=float(tot32.norm()), global_floor=_rel(torch.cat(abf), tot32))
    # the same global figure as the comparer can form it from samples alone (numel / k weights): what the GPU tests gate against
    w = _weights(out)
    s32, sbf = out["samples"].double(), torch.cat([v[i] for v, i in zip(abf, idx)])
    out["global_floor_sampled"] = float(((sbf - s32) ** 2 * w).sum().sqrt() / (s32 ** 2 * w).sum().sqrt())
    out.update(extra)
    return out


def _counts(fx):
    return [min(int(n), int(fx["k"])) for n in fx["numel"].tolist()]


def _weights(fx):
    """Per-sample weight numel / samples of its tensor: a weighted sum over the samples estimates the sum over the whole gradient."""
    return torch.cat([torch.full((c,), n / c, dtype=torch.float64) for n, c in zip(fx["numel"].tolist(), _counts(fx))])


def compare(got, fx):
    """got: {name: gradient tensor (any device)}.  Per tensor (lists in fx["names"] order): ``err`` sampled rel-L2 against the stored
    fp32 samples, ``norm`` of the whole tensor and ``norm_ratio`` = norm / norm_fp32 (inf where the reference norm is zero); global:
    ``e32`` and ``cos`` over all samples with numel / k weights (estimates of the whole-gradient figures), ``finite``."""
    names = fx["names"]
    idx = sample_indices(fx["numel"].tolist(), fx["index_seed"], fx["k"])
    ref = torch.split(fx["samples"].double(), _counts(fx))
    err, norm, ratio, mine, finite = [], [], [], [], True
    for n, numel, i, r in zip(names, fx["numel"].tolist(), idx, ref):
        g = got[n].detach().reshape(-1)
        assert g.numel() == numel, (n, g.numel(), numel)
        finite = finite and bool(torch.isfinite(g).all())
        s = g[i.to(g.device)].double().cpu()
        mine.append(s)
        err.append(_rel(s, r))
        norm.append(float(g.double().norm()))
    for v, r in zip(norm, fx["norm_fp32"].tolist()):
        ratio.append(v / r if r > 0 else float("inf"))
    a, r, w = torch.cat(mine), fx["samples"].double(), _weights(fx)
    e32 = float(((a - r) ** 2 * w).sum().sqrt() / (r ** 2 * w).sum().sqrt())
    cos = float((a * r * w).sum() / ((a ** 2 * w).sum().sqrt() * (r ** 2 * w).sum().sqrt()))
    return dict(names=names, err=err, norm=norm, norm_ratio=ratio, e32=e32, cos=cos, finite=finite,
                total_norm=float(torch.tensor(norm, dtype=torch.float64).norm()))


def exempt(fx):
    """Tensors left out of the relative checks: own floor above EXEMPT_FLOOR.  Only attention key biases may be (their true gradient
    is zero: a key bias shifts every logit of a softmax row equally), and at most MAX_EXEMPT of them; anything else is a failure."""
    ex = [n for n, f in zip(fx["names"], fx["floor"].tolist()) if not f <= EXEMPT_FLOOR]
    bad = [n for n in ex if not n.endswith("to_k.bias")]
    assert not bad and len(ex) <= MAX_EXEMPT, (len(ex), bad)
    return ex


def tensor_bound(fx, mode):
    """Per-tensor bound on the sampled rel-L2 and on |norm ratio - 1|, in fx["names"] order."""
    if mode == "fp32":
        return [2e-3] * len(fx["names"])
    return [2.5 * f + 5e-3 for f in fx["floor"].tolist()]


def failing_tensors(res, fx, mode, zero_margin):
    """Names that miss their gate.  Relative gates (tensor_bound) on every tensor but the exempt ones; those are bounded in norm by
    ``zero_margin`` x the bf16-emulating oracle's own rounding noise in the same tensor (norm_bf16)."""
    ex = set(exempt(fx))
    bad = []
    for n, e, nr, g, nb, b in zip(fx["names"], res["err"], res["norm_ratio"], res["norm"], fx["norm_bf16"].tolist(), tensor_bound(fx, mode)):
        if n in ex:
            ok = g <= zero_margin * nb
        else:
            ok = e <= b and abs(nr - 1.0) <= b
        if not ok:
            bad.append(n)
    return bad


def global_ok(res, fx, mode, kind):
    """bf16: e32 <= 1.5 floor + 2e-3 (UNet) / 5e-3 (AutoencoderKL) and the cosine condition of the tiny-network tests, the floor being the
    oracle's own bf16-vs-fp32 figure formed from the same samples; fp32 mode: 1e-3."""
    if mode == "fp32":
        return res["finite"] and res["e32"] <= 1e-3
    fl = fx["global_floor_sampled"]
    add = 2e-3 if kind == "unet" else 5e-3
    return res["finite"] and res["e32"] <= 1.5 * fl + add and res["cos"] >= 1.0 - 2.0 * (2.0 * fl + 2e-3) ** 2


def floor_ratio_stats(res, fx):
    """Distribution of err / floor over the non-exempt tensors: (median, p90, max, name of the max)."""
    ex = set(exempt(fx))
    rows = sorted((e / max(f, 1e-30), n) for n, e, f in zip(fx["names"], res["err"], fx["floor"].tolist()) if n not in ex)
    vals = [v for v, _ in rows]
    return vals[len(vals) // 2], vals[min(len(vals) - 1, int(0.9 * len(vals)))], rows[-1][0], rows[-1][1]


def synthetic(seed=0, floor=1e-2):
    """A small seeded stand-in for an oracle run: {name: g32}, {name: gbf} with per-tensor rounding noise at ``floor`` and one
    attention key bias whose true gradient is zero; build_fixture() of it is what tests/test_train_full_cpu.py gates against."""
    g = torch.Generator().manual_seed(seed)
    shapes = {"down.0.conv1.conv.weight": (32, 16, 3, 3, 3), "down.0.conv1.conv.bias": (32,), "down.1.conv1.conv.weight": (32, 16, 3, 3, 3),
              "down.1.conv1.conv.bias": (32,), "down.0.norm1.weight": (16,), "down.0.norm1.bias": (16,), "attn.to_q.weight": (64, 64),
              "attn.to_k.weight": (64, 64), "attn.to_k.bias": (64,), "time_embed.0.weight": (256, 64), "out.2.conv.weight": (4, 32, 3, 3, 3)}
    g32, gbf = {}, {}
    for i, (n, s) in enumerate(shapes.items()):
        scale = 10.0 ** (-(i % 4))                         # tensors of very different size in the global norm
        g32[n] = torch.zeros(s) if n.endswith("to_k.bias") else scale * torch.randn(s, generator=g)
        noise = torch.randn(s, generator=g)
        gbf[n] = g32[n] + (1e-6 * noise if n.endswith("to_k.bias") else floor * scale * noise)
    return g32, gbf
