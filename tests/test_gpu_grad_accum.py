"""Gradient accumulation through the model (-m gpu): ldm_model_set_grad_accum on the UNet and AutoencoderKL training plans, in bf16 and fp32
precision, alone, with a world-size-1 communicator and against a fake second rank.  Shapes of
test_gpu_comm.py::test_bucketed_exchange_with_a_fake_second_rank_gives_the_mean: UNET_TINY, 1x4x8^3, gain 0.5, 1 MB buckets (several
buckets at odd offsets) and once more the default bucket size (one bucket).

The reference for every armed backward is the gradient of the same sample from an un-armed backward (the backward plans are bit
reproducible; test_gpu_comm.py relies on that too) and torch's own fp32 arithmetic on those: acc = g_0 * s, then acc = acc + g_j * s,
product and sum rounded separately.  An accumulator that starts as NaN shows a range that no bucket covers (NaN survives), a range
accumulated twice (the value doubles) and assign and add swapped (NaN survives / the first term is lost)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import cfgs

pytestmark = pytest.mark.gpu
BAD_ARG = -1


@pytest.fixture(scope="module")
def samples(cuda):
    g = torch.Generator().manual_seed(7)
    xs = torch.randn((4, 4, 8, 8, 8), generator=g).to(cuda)
    tg = torch.randn((4, 4, 8, 8, 8), generator=g).to(cuda)
    ts = torch.tensor([17.0, 803.0, 401.0, 990.0], device=cuda)
    return xs, tg, ts


@pytest.fixture(params=["1", None], ids=["1MB-buckets", "default-buckets"])
def bucket_mb(request, monkeypatch):
    """Set before a model's first backward: the plan reads it when it is built."""
    if request.param is None:
        monkeypatch.delenv("LDM_GRAD_BUCKET_MB", raising=False)
    else:
        monkeypatch.setenv("LDM_GRAD_BUCKET_MB", request.param)
    return request.param


def _unet(cuda, precision="bf16"):
    from ldm3d.networks import DiffusionModelUNet
    from oracle import unet as ou
    cfg = cfgs.UNET_TINY
    m = DiffusionModelUNet(**cfg)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfg), 3, gain=0.5))
    m = m.to(cuda).train()
    if precision != "bf16":
        m.set_precision(precision)
    m.flatten_parameters()
    return m


def _backward(m, samples, j):
    """One backward of sample j (a slice: B = 1) or of the samples j (a list: B = len)."""
    xs, tg, ts = samples
    sel = slice(j, j + 1) if isinstance(j, int) else j
    F.mse_loss(m(x=xs[sel], timesteps=ts[sel]).float(), tg[sel]).backward()
    torch.cuda.synchronize()
    return m.flat_grads.clone()


def _bits(t):
    return t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _torch_sequence(grads, K):
    """acc after each micro-batch in torch's fp32 arithmetic, two roundings per step."""
    s = torch.tensor(float(1.0 / K), dtype=torch.float32, device=grads[0].device)
    out, acc = [], None
    for j in range(K):
        p = grads[j] * s
        acc = p if j == 0 else acc + p
        out.append(acc)
    return out


def _armed_window(m, samples, K, acc, after=None):
    """K armed backwards into ``acc``; returns flat_grads and the accumulator after each."""
    fgs, accs = [], []
    for j in range(K):
        m.set_grad_accum(acc, j, K)
        fgs.append(_backward(m, samples, j))
        accs.append(acc.clone())
        if after is not None:
            after(j)
    return fgs, accs


def test_armed_backwards_accumulate_bucket_by_bucket(cuda, built_lib, samples, bucket_mb):
    L = built_lib
    m = _unet(cuda)
    g = [_backward(m, samples, j) for j in range(4)]
    assert not _same_bits(g[0], g[1]) and all(bool(torch.isfinite(x).all()) for x in g)
    total = int(L.ldm_model_param_numel_total(m._h))
    sched = (C.c_int * 512)(), (C.c_int64 * 512)(), (C.c_int64 * 512)(), (C.c_int * 512)()
    n_ev = L.ldm_model_grad_schedule(m._h, 1, 8, 8, 8, *sched, 512)
    n_buckets = sum(1 for k in range(min(n_ev, 512)) if sched[0][k] == 1)
    assert n_buckets >= 4 if bucket_mb == "1" else n_buckets == 1, n_buckets
    acc = torch.full((total,), float("nan"), device=cuda)

    # K = 3: s = float(1/3) is no power of two.  Bound against the fp64 running sum S_j = sum_{i <= j} g_i s, elementwise:
    #   E_0 = 2^-23 |g_0 s|                    (assign: one rounding of the product, <= 2^-24 |g_0 s|; the kernel bound of the op test)
    #   E_j = E_{j-1} + 2^-23 (|S_{j-1}| + E_{j-1} + |g_j s|)
    # each add step makes at most two roundings of at most 2^-24 of a quantity no larger than |acc_{j-1}| + |g_j s|, and the accumulator it
    # starts from is no further than E_{j-1} from S_{j-1}.
    K = 3
    fgs, accs = _armed_window(m, samples, K, acc)
    s64 = float(torch.tensor(1.0 / K, dtype=torch.float32))
    S, E = None, None
    for j in range(K):
        assert _same_bits(fgs[j], g[j]), f"flat_grads of armed micro-batch {j} differs from the un-armed backward"
        p = g[j].double() * s64
        if j == 0:
            S, E = p, 2.0 ** -23 * p.abs()
        else:
            E = E + 2.0 ** -23 * (S.abs() + E + p.abs())
            S = S + p
        assert bool(torch.isfinite(accs[j]).all()), f"micro-batch {j}: a NaN of the pre-filled accumulator survived"
        err = (accs[j].double() - S).abs()
        assert bool((err <= E).all()), (j, float((err - E).max()))
    # contraction is off in the kernel, so the K = 3 window is torch's two-rounding sequence as well
    for j, ref in enumerate(_torch_sequence(g, K)):
        assert _same_bits(accs[j], ref), (K, j)

    # K = 2 and K = 4: s is a power of two, bit for bit the torch sequence after every micro-batch
    for K in (2, 4):
        acc.fill_(float("nan"))
        fgs, accs = _armed_window(m, samples, K, acc)
        for j, ref in enumerate(_torch_sequence(g, K)):
            assert _same_bits(fgs[j], g[j]) and _same_bits(accs[j], ref), (K, j, int((_bits(accs[j]) != _bits(ref)).sum()))
        assert not _same_bits(accs[1], g[1] * (1.0 / K))                 # negative control: add taken for assign
    last = acc.clone()

    # bad arguments return LDM_ERR_BAD_ARG and leave the previous setting (micro-batch 1 of 2: add mode, s = 0.5) in force
    m.set_grad_accum(acc, 1, 2)
    assert L.ldm_model_set_grad_accum(m._h, acc.data_ptr(), 2, 2) == BAD_ARG
    assert L.ldm_model_set_grad_accum(m._h, acc.data_ptr(), 0, 0) == BAD_ARG
    assert L.ldm_model_set_grad_accum(m._h, acc.data_ptr(), -1, 2) == BAD_ARG
    assert _same_bits(_backward(m, samples, 2), g[2])
    assert _same_bits(acc, last + g[2] * 0.5)

    # disarmed: today's behaviour, flat_grads bit for bit, the accumulator untouched
    m.set_grad_accum(None)
    kept = acc.clone()
    m.flat_grads.fill_(float("nan"))
    assert _same_bits(_backward(m, samples, 0), g[0]) and _same_bits(acc, kept)


def test_fp32_precision_mode_and_the_batch_two_gradient(cuda, samples, bucket_mb):
    m = _unet(cuda, "fp32")
    g = [_backward(m, samples, j) for j in range(2)]
    acc = torch.full_like(g[0], float("nan"))
    fgs, accs = _armed_window(m, samples, 2, acc)
    for j, ref in enumerate(_torch_sequence(g, 2)):
        assert _same_bits(fgs[j], g[j]) and _same_bits(accs[j], ref), j
    m.set_grad_accum(None)
    gAB = _backward(_unet(cuda, "fp32"), samples, [0, 1])          # mse mean over the batch = the mean of the two samples' losses
    r = float((gAB - acc).norm() / gAB.norm())
    print(f"fp32 mode: accumulated K = 2 gradient vs the B = 2 gradient: rel-L2 {r:.2e}")
    assert r <= 2e-2                                                # the bound test_gpu_comm.py allows between a mean of gradients and B = 2


def test_autoencoder_plan_accumulates(cuda, bucket_mb):
    """VAE_TINY at 8^3 (every one of its three levels keeps at least 2^3 voxels), one eps draw, K = 2, bit for bit."""
    from ldm3d.networks import AutoencoderKL
    from oracle import autoencoder as oa
    from oracle.unet import init_state_dict
    cfg = cfgs.VAE_TINY
    v = AutoencoderKL(**cfg)
    v.load_state_dict(init_state_dict(oa.ae_param_shapes(cfg), 3))
    v = v.to(cuda).train()
    v.flatten_parameters()
    gen = torch.Generator().manual_seed(12)
    imgs = torch.rand((2, 2, 8, 8, 8), generator=gen).to(cuda)
    eps = torch.randn((1, 8, 2, 2, 2), generator=gen).to(cuda)

    def once(k):
        rec, mu, sigma = v(imgs[k:k + 1], eps=eps)
        (F.l1_loss(rec, imgs[k:k + 1]) + 1e-6 * oa.kl_loss(mu, sigma).mean()).backward()
        torch.cuda.synchronize()
        return v.flat_grads.clone()
    g = [once(0), once(1)]
    assert not _same_bits(g[0], g[1]) and float(g[0].abs().max()) > 0
    acc = torch.full_like(g[0], float("nan"))
    ref = _torch_sequence(g, 2)
    for j in range(2):
        v.set_grad_accum(acc, j, 2)
        assert _same_bits(once(j), g[j]) and _same_bits(acc, ref[j]), j
    v.set_grad_accum(None)
    kept = acc.clone()
    assert _same_bits(once(0), g[0]) and _same_bits(acc, kept)


def _trace(L, m):
    issue, done, elems = (C.c_double * 256)(), (C.c_double * 256)(), (C.c_int64 * 256)()
    n = L.ldm_model_grad_sync_trace(m._h, issue, done, elems, 256)
    return n, [elems[k] for k in range(max(n, 0))]


def test_only_the_last_micro_batch_exchanges(cuda, built_lib, samples, bucket_mb):
    """World size 1 (mean = identity): micro-batches 0 .. K-2 issue nothing, the last one hands over buckets that tile the buffer, and the
    accumulator equals the un-synchronised accumulation bit for bit."""
    from ldm3d.trainer import GradSync
    L = built_lib
    K = 3
    m = _unet(cuda)
    g = [_backward(m, samples, j) for j in range(K)]
    total = g[0].numel()
    plain = torch.full((total,), float("nan"), device=cuda)
    _armed_window(m, samples, K, plain)
    m.set_grad_accum(None)
    assert GradSync().attach(m, force_single=True)
    _backward(m, samples, 0)                                        # an un-armed backward first: its buckets must not show up below
    assert _trace(L, m)[0] >= 1
    acc = torch.full((total,), float("nan"), device=cuda)
    seen = []

    def after(j):
        seen.append((L.ldm_model_grad_sync_pending(m._h),) + _trace(L, m))
    fgs, _ = _armed_window(m, samples, K, acc, after=after)
    for j in range(K - 1):
        assert seen[j][0] == 0 and seen[j][1] == 0, (j, seen[j])
    pending, n, elems = seen[K - 1]
    assert pending == 0 and n >= (4 if bucket_mb == "1" else 1) and sum(elems) == total, (n, sum(elems), total)
    assert all(_same_bits(fgs[j], g[j]) for j in range(K))
    assert _same_bits(acc, plain)


class AccPeer:
    """Rank 1 of a 2-rank job on one GPU, over the ACCUMULATOR: the shape of test_gpu_comm.py's FakePeer.  Leaves op(own, peer) in the range
    it is handed, on the stream it is handed, and records which micro-batch was running when it was called."""

    def __init__(self, acc: torch.Tensor, peer: torch.Tensor):
        self.acc, self.peer, self.calls, self.micro = acc, peer, [], None

    def __call__(self, buf, count, dtype, op, stream):
        off = (buf - self.acc.data_ptr()) // 4
        inside = (buf - self.acc.data_ptr()) % 4 == 0 and 0 <= off and off + count <= self.acc.numel()
        self.calls.append((off, count, dtype, op, self.micro, inside))
        if not inside:
            return 1
        with torch.cuda.stream(torch.cuda.ExternalStream(stream)):
            view = self.acc[off:off + count]
            view.add_(self.peer[off:off + count])
            if op == 1:
                view.mul_(0.5)
        return 0


def test_fake_second_rank_reduces_the_accumulator(cuda, samples, bucket_mb):
    """World size 2: this rank accumulates samples 0 and 1, the peer contributes the accumulation of samples 2 and 3.  The transport is
    called only during the last micro-batch, every call lies inside the accumulator, the ranges tile it back to front exactly once, and the
    result is (acc_own + acc_peer) * 0.5 bit for bit -- a bucket exchanged before its accumulate launch, or on flat_grads, shows here."""
    from ldm3d.trainer import GradSync
    K = 2
    m = _unet(cuda)
    g = [_backward(m, samples, j) for j in range(4)]
    own, peer_acc = _torch_sequence(g[:2], K)[-1], _torch_sequence(g[2:], K)[-1]
    total = own.numel()
    acc = torch.full((total,), float("nan"), device=cuda)
    peer = AccPeer(acc, peer_acc)
    assert GradSync().attach(m, transport=peer, world=2, rank=0)
    for j in range(K):
        peer.micro = j
        m.set_grad_accum(acc, j, K)
        assert _same_bits(_backward(m, samples, j), g[j])           # flat_grads is this rank's own micro gradient, never reduced
        if j < K - 1:
            assert peer.calls == [] and _same_bits(acc, g[0] * 0.5)
    calls = peer.calls
    assert len(calls) >= (4 if bucket_mb == "1" else 1)
    assert all(inside and micro == K - 1 and dtype == 0 and op == 1 for _, _, dtype, op, micro, inside in calls), calls
    assert calls[0][0] + calls[0][1] == total and calls[-1][0] == 0
    assert all(a[0] == b[0] + b[1] for a, b in zip(calls, calls[1:]))
    assert _same_bits(acc, (own + peer_acc) * 0.5)
    assert not _same_bits(acc, own)                                  # negative control: an exchange that did nothing
