"""The plan trace (ldm_set_plan_trace) is the one externally visible rendering of the plan records (ConvRec, GnRec, WgradRec,
LayoutRec, AttnRec, LinRec, ElemRec, RangeRec in csrc/ldm3d.hip): tools/plan_trace.py and ldm3d/profiling.py read its rows.  One
UNet forward per precision pins the text of the OP_CONV / OP_FINALIZE rows and ties them to what ldm_model_plan_conv_cfgs reports
for the same plan; one inference forward and one training step per precision tie the GroupNorm, weight-gradient and light-GEMM rows
to the model's own parameter shapes; the same UNet plans, a denoise step and the AutoencoderKL plans tie the rows of the small kinds
(packing, attention, time embedding, element-wise, batch and bucket ops) to the model and the shape."""
import collections
import ctypes as C
import re

import pytest
import torch

import cfgs

pytestmark = pytest.mark.gpu
OP_CONV, OP_FINALIZE = 1, 2                  # enum OpKind, as tools/plan_trace.py's KINDS
ROW = re.compile(r"M=(\d+) k=(\d+) s=(\d+) ups=(\d+) cin=(\d+)\+(\d+)\(x(\d+)\) cin1=(\d+) couts=(\d+) cfg=(\d+)x(\d+)x(\d+) "
                 r"splitk=(\d+) halo=(\d+) mtps=(\d+) qps=(\d+) cube=(\d+)")
FIELDS = "M k s ups cin_a cin_b nchunk cin1 couts wgm wgn bk splitk halo mtps qps cube".split()


def test_trace_rows_of_the_conv_family(cuda, tmp_path):
    from ldm3d import _lib
    from ldm3d.networks import DiffusionModelUNet
    from oracle import unet as ou
    L = _lib.lib()
    m = DiffusionModelUNet(**cfgs.UNET_FULL)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfgs.UNET_FULL), 0))
    m = m.to(cuda).eval()
    x = torch.randn((1, 4, 8, 8, 8), generator=torch.Generator().manual_seed(0)).to(cuda)
    t = torch.tensor([500.0], device=cuda)
    path = tmp_path / "trace.csv"
    buf = (C.c_int * (4 * 512))()
    n = L.ldm_model_plan_conv_cfgs(m._h, b"unet", 1, 8, 8, 8, buf, 512)
    assert 0 < n <= 512, n
    # (halo code, splitk) of the OP_CONV entries; the OP_CONV_BLOCK entries it interleaves report halo codes 3 / 4
    planned = [(buf[4 * i + 2] >> 8, buf[4 * i + 3]) for i in range(n) if buf[4 * i + 2] >> 8 not in (3, 4)]
    _lib.check(L.ldm_set_plan_trace(str(path).encode()))
    try:
        with torch.no_grad():
            m(x=x, timesteps=t)
            torch.cuda.synchronize()
            n_bf16 = len(path.read_text().splitlines())
            m.set_precision("fp32")
            m(x=x, timesteps=t)
            torch.cuda.synchronize()
    finally:
        _lib.check(L.ldm_set_plan_trace(None))
    lines = path.read_text().splitlines()
    assert 0 < n_bf16 < len(lines)

    def conv_rows(part):
        out = []
        for ln in part:
            nops, oi, kind, us, desc = ln.split(",", 4)
            assert int(oi) < int(nops) and float(us) >= 0.0, ln
            if int(kind) in (OP_CONV, OP_FINALIZE):
                mt = ROW.fullmatch(desc)
                assert mt, ln
                out.append((int(kind), dict(zip(FIELDS, map(int, mt.groups())))))
            else:
                assert re.fullmatch(r"i=-?\d+( -?\d+){5}", desc), ln
        return out

    bf16, fp32 = conv_rows(lines[:n_bf16]), conv_rows(lines[n_bf16:])
    traced = [(5 if r["cube"] else r["halo"], r["splitk"]) for k, r in bf16 if k == OP_CONV]
    assert traced == planned, (traced, planned)
    assert any(c == 5 for c, _ in traced), traced                  # the 4^3 / 2^3 levels' plain 3^3 convs run on conv3_cube_kernel
    # an OP_FINALIZE is a copy of the split-K conv in front of it: the same row
    for (k0, r0), (k1, r1) in zip(bf16, bf16[1:]):
        if k1 == OP_FINALIZE:
            assert k0 == OP_CONV and r0 == r1 and r0["splitk"] > 1, (r0, r1)
    # ups= is the bit set 1 ups | 2 exact | 4 phase | 8 3 x bf16 product | 16 / 32 fused fp32 NDHWC / NCDHW epilogue: inference plans
    # have no exact (transposed) convs and run the Upsample convs in the phase form; the bf16-kernel convs of an fp32 plan are all
    # 3 x bf16 products, and only an unsplit one can own its epilogue
    assert {r["ups"] for _, r in bf16} <= {0, 4} and sum(1 for k, r in bf16 if k == OP_CONV and r["ups"] == 4) == 2, bf16
    assert fp32 and all(k == OP_CONV and r["ups"] & 8 and not r["ups"] & 3 for k, r in fp32), fp32
    assert all(r["splitk"] == 1 for _, r in fp32 if r["ups"] & 48) and not any(r["ups"] & 16 and r["ups"] & 32 for _, r in fp32)
    for _, r in bf16 + fp32:
        assert r["k"] == (2 if r["ups"] & 4 else 3) or r["k"] == 1, r
        assert r["M"] in (512, 64, 8) and r["couts"] % 32 == 0 and r["cin_a"] % 32 == 0, r


# enum OpKind, as tools/plan_trace.py's KINDS
GN_STATS, GN_PREP, GN_APPLY, GN_FUSED, WGRAD, GNB, GEMM_LIGHT, GN_STATS32, GN_APPLY32, FIN_GN, GEMM_LIGHT32 = 3, 5, 6, 11, 14, 18, 25, 31, 32, 40, 41


def test_trace_rows_of_the_groupnorm_wgrad_and_light_gemm_ops(cuda, tmp_path):
    """UNET_TINY at 1 x 4 x 8^3: an inference forward and a training step (forward + backward) in bf16, then in fp32 precision.  The
    six integers of every converted kind's row are checked against the model: the weight-gradient rows (cdy cx Cout Cin ld ci_off)
    against the conv weights, the GroupNorm rows against the GroupNorm weights, the light-GEMM rows (M K CoutS CoutPad big ca)
    against the three resolutions."""
    import torch.nn.functional as F
    from ldm3d import _lib
    from ldm3d.networks import DiffusionModelUNet
    from oracle import unet as ou
    L = _lib.lib()
    cfg = cfgs.UNET_TINY
    m = DiffusionModelUNet(**cfg)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfg), 3, gain=0.5))
    m = m.to(cuda)
    g = torch.Generator().manual_seed(1)
    x = torch.randn((1, 4, 8, 8, 8), generator=g).to(cuda)
    target = torch.randn((1, 4, 8, 8, 8), generator=g).to(cuda)
    t = torch.tensor([500.0], device=cuda)
    # what the rows must describe.  Conv weights: 5-D tensors and the attention projections; to_q / to_k / to_v of one block are rows
    # of ONE packed (3 C, C) matrix, differentiated by one weight-gradient launch.  GroupNorm weights: the 1-D `.weight`s.
    convs, gn_sizes = collections.Counter(), collections.Counter()
    for name, p in m.named_parameters():
        if p.dim() == 5 or name.endswith(".attn.out_proj.weight"):
            convs[(p.shape[0], p.shape[1])] += 1
        elif name.endswith(".attn.to_q.weight"):
            convs[(3 * p.shape[0], p.shape[1])] += 1
        elif p.dim() == 1 and name.endswith(".weight"):
            gn_sizes[p.shape[0]] += 1
    n_gn = sum(gn_sizes.values())
    assert n_gn > 0 and len(convs) > 1

    path = tmp_path / "trace.csv"
    marks = []

    def mark():
        torch.cuda.synchronize()
        marks.append(len(path.read_text().splitlines()))

    _lib.check(L.ldm_set_plan_trace(str(path).encode()))
    try:
        for prec in ("bf16", "fp32"):
            m.set_precision(prec)
            m.eval()
            with torch.no_grad():
                m(x=x, timesteps=t)
            mark()
            m.train()
            loss = F.mse_loss(m(x=x, timesteps=t).float(), target)
            mark()
            loss.backward()
            mark()
            m.zero_grad(set_to_none=True)
    finally:
        _lib.check(L.ldm_set_plan_trace(None))
    lines = path.read_text().splitlines()
    assert len(marks) == 6 and all(a < b for a, b in zip([0] + marks, marks)) and marks[-1] == len(lines), marks

    def rows(lo, hi):
        out = []
        for ln in lines[lo:hi]:
            _, _, kind, _, desc = ln.split(",", 4)
            if desc.startswith("i="):
                out.append((int(kind), tuple(int(v) for v in desc[2:].split())))
        return out

    def check_forward(part, inference):
        applied = 0
        for kind, v in part:
            if kind in (GN_STATS, GN_STATS32, GN_PREP, GN_FUSED, GN_APPLY, GN_APPLY32):     # ca cb ...
                assert v[0] % 8 == 0 and v[0] + v[1] in gn_sizes, (kind, v)
            if kind in (GN_FUSED, GN_APPLY, GN_APPLY32) or (inference and kind == FIN_GN):  # (a split-K finalize may apply the GroupNorm behind it)
                applied += 1
            if kind in (GEMM_LIGHT, GEMM_LIGHT32):                                        # M K CoutS CoutPad big ca
                M, K, couts, cout_pad, big, ca = v
                assert M in (512, 64, 8) and K % 32 == 0 and couts % 32 == 0 and couts <= cout_pad and big in (0, 1), v
        assert applied == n_gn, (applied, n_gn)
        return sum(1 for kind, _ in part if kind in (GEMM_LIGHT, GEMM_LIGHT32))

    def check_backward(part):
        groups, cur = [], None                       # one weight matrix: rows of equal (Cout, ld) whose columns ci_off run 0 .. ld
        for kind, v in part:
            if kind != WGRAD:
                continue
            cdy, cx, cout, cin, ld, ci_off = v
            assert ci_off + cin <= ld and cout <= cdy and cdy % 32 == 0, v
            if cur is None or ci_off == 0:
                assert cur is None or cur[2] == cur[1], (cur, v)      # the Cin of a group sum to ld
                cur = [cout, ld, 0]
                groups.append(cur)
            assert (cout, ld) == (cur[0], cur[1]) and ci_off == cur[2], (cur, v)
            cur[2] += cin
        assert cur is not None and cur[2] == cur[1], cur
        assert collections.Counter((c, ld) for c, ld, _ in groups) == convs, (groups, convs)
        gnb = [v for kind, v in part if kind == GNB]  # ca cb groups DHW N silu
        for ca, cb, ng, dhw, n, silu in gnb:
            assert ng == 32 and n == 1 and dhw in (512, 64, 8) and silu in (0, 1), (ca, cb, ng, dhw, n, silu)
        assert collections.Counter(ca + cb for ca, cb, *_ in gnb) == gn_sizes, (gnb, gn_sizes)

    b = [0] + marks
    for k in (0, 3):                                 # bf16, fp32
        n_light = check_forward(rows(b[k], b[k + 1]), True)
        n_light += check_forward(rows(b[k + 1], b[k + 2]), False)
        assert n_light > 0
        check_backward(rows(b[k + 2], b[k + 3]))


# enum OpKind, as tools/plan_trace.py's KINDS
PACK, ATTN, SINUSOID, GEMV, VAE_HEADS, WT_BATCH, EXPORT_BATCH, ATTN_BWD, ADD, SUMPOOL, LIN_DX, LIN_DW, VAE_HEADS_BWD = 0, 7, 8, 9, 10, 13, 16, 19, 20, 21, 22, 23, 24
COLSUM_BATCH, IM2COL, PACK32, ATTN32, GEMV32, BUCKET, BUCKET_JOIN, UPS_SPLIT32, TEMB_ROW = 26, 27, 28, 33, 34, 36, 37, 38, 43


def _traced(path, steps):
    """Runs the callables of ``steps`` in order with the plan trace on: the rows [(kind, six integers)] each of them appended."""
    from ldm3d import _lib
    L = _lib.lib()
    parts, seen = [], 0
    _lib.check(L.ldm_set_plan_trace(str(path).encode()))
    try:
        for step in steps:
            step()
            torch.cuda.synchronize()
            lines = path.read_text().splitlines()
            assert len(lines) > seen, step
            descs = [ln.split(",", 4) for ln in lines[seen:]]
            parts.append([(int(d[2]), tuple(int(v) for v in d[4][2:].split())) for d in descs if d[4].startswith("i=")])
            seen = len(lines)
    finally:
        _lib.check(L.ldm_set_plan_trace(None))
    return parts


def _of(part, *kinds):
    return [v for kind, v in part if kind in kinds]


def _check_common(fwd_parts, bwd, fp32, n_attn_bwd):
    """What holds for the backward of the UNet and of the AutoencoderKL alike, and for the kinds that only a backward has."""
    for part in fwd_parts:
        assert not _of(part, ADD, SUMPOOL, WT_BATCH, BUCKET, BUCKET_JOIN, COLSUM_BATCH, EXPORT_BATCH, ATTN_BWD, LIN_DX, LIN_DW, VAE_HEADS_BWD), part
    # one weight flip / transpose launch, first; then the packed gradient of the network output
    assert bwd[0] == (WT_BATCH, (int(fp32), 0, 0, 0, 0, 0)) and len(_of(bwd, WT_BATCH)) == 1, bwd[:2]
    assert bwd[1][0] == (PACK32 if fp32 else PACK) and len(_of(bwd, PACK, PACK32, IM2COL)) == 1, bwd[:2]
    for v in _of(bwd, ADD):                          # vector count, fp32
        assert v[0] > 0 and v[1:] == (int(fp32), 0, 0, 0, 0), v
    for n, d, h, w, c, f in _of(bwd, SUMPOOL):       # N D H W C fp32
        assert n == 1 and d == h == w and d in (2, 4, 8) and c % 32 == 0 and f == int(fp32), (n, d, h, w, c, f)
    assert len(_of(bwd, ATTN_BWD)) == n_attn_bwd
    for kind in (COLSUM_BATCH, EXPORT_BATCH):        # first block, end block: each launch continues where the previous one ended
        end = 0
        for v in _of(bwd, kind):
            assert v[0] == end and v[0] <= v[1] and v[2:] == (0, 0, 0, 0), (kind, v)
            end = v[1]
    assert _of(bwd, EXPORT_BATCH)


def _check_buckets(bwd, total):
    hi = total                                       # first element, element count: the flat gradient buffer from its end to its front
    for first, count, *rest in _of(bwd, BUCKET):
        assert count > 0 and first + count == hi and rest == [0, 0, 0, 0], (first, count, hi)
        hi = first
    assert hi == 0 and _of(bwd, BUCKET)
    assert bwd[-1] == (BUCKET_JOIN, (0,) * 6) and len(_of(bwd, BUCKET_JOIN)) == 1, bwd[-1]


def test_trace_rows_of_the_small_kinds(cuda, tmp_path):
    """The rows of the kinds LayoutRec, AttnRec, LinRec, ElemRec and RangeRec describe, tied to the model and the shape.  UNET_TINY
    at 1 x 4 x 8^3: an inference forward and a training step per precision, then one denoise step through the device sampler (the
    time-embedding table: one TEMB_ROW row instead of SINUSOID + three GEMVs).  VAE_TINY_ATTN at 1 x 1 x 16^3: encode, decode and
    a training step per precision.  The packed gradient at the head of a backward is marked internal in the AutoencoderKL plan
    alone: the UNet's arrives with its channel count, like the network input (Builder::pack).  The AutoencoderKL backward has no
    ADD row (no tensor of it collects two aliased gradients), the UNet's has; TAP rows occur in none of these plans (only the
    debug-tap entry points emit them)."""
    import torch.nn.functional as F
    from ldm3d import _lib
    from ldm3d.networks import AutoencoderKL, DiffusionModelUNet
    from ldm3d.schedulers import DDPMScheduler
    from oracle import autoencoder as oa
    from oracle import unet as ou
    L = _lib.lib()
    g = torch.Generator().manual_seed(1)

    # ---- UNet
    cfg = cfgs.UNET_TINY
    m = DiffusionModelUNet(**cfg)
    m.load_state_dict(ou.init_state_dict(ou.unet_param_shapes(cfg), 3, gain=0.5))
    m = m.to(cuda)
    x = torch.randn((1, 4, 8, 8, 8), generator=g).to(cuda)
    target = torch.randn((1, 4, 8, 8, 8), generator=g).to(cuda)
    t = torch.tensor([500.0], device=cuda)
    shapes = {name: tuple(p.shape) for name, p in m.named_parameters()}
    ch = cfg["channels"]
    # attention blocks: num_res_blocks per down level, one more per up level, and the middle block at the last level's width
    nrb = cfg["num_res_blocks"]
    attn = collections.Counter()
    for lvl, on in enumerate(cfg["attention_levels"]):
        if on:
            attn[(1, (8 >> lvl) ** 3, ch[lvl], 64)] += 2 * nrb + 1          # B N C d
    attn[(1, (8 >> (len(ch) - 1)) ** 3, ch[-1], 64)] += 1
    n_attn = sum(attn.values())
    assert n_attn == sum(1 for name in shapes if name.endswith(".attn.to_q.weight")) and set(attn) == {(1, 64, 64, 64), (1, 8, 128, 64)}
    rows = sum(s[0] for name, s in shapes.items() if name.endswith(".time_emb_proj.weight"))
    lins = [shapes["time_embed.0.weight"][::-1], shapes["time_embed.2.weight"][::-1], (shapes["time_embed.2.weight"][0], rows)]   # (I, O)
    assert lins[0] == (ch[0], 4 * ch[0]) and rows > 0
    total = int(L.ldm_model_param_numel_total(m._h))
    state = {}

    def infer():
        m.eval()
        with torch.no_grad():
            m(x=x, timesteps=t)

    def train_forward():
        m.train()
        state["loss"] = F.mse_loss(m(x=x, timesteps=t).float(), target)

    def backward():
        state.pop("loss").backward()
        m.zero_grad(set_to_none=True)

    def denoise():
        m.eval()
        m.enable_graph_replay(False)
        sampler = DDPMScheduler(**cfgs.SCHED).device_sampler(seed=3)
        xb, tbuf = x.clone(), torch.empty((1,), device=cuda)
        with torch.no_grad():
            sampler.reset(tbuf)
            m.denoise_step(xb, tbuf, sampler)

    for prec in ("bf16", "fp32"):
        fp32 = prec == "fp32"
        m.set_precision(prec)
        inf, trf, bwd = _traced(tmp_path / f"unet_{prec}.csv", [infer, train_forward, backward])
        att_kind, gemv_kind, pack_kind = (ATTN32, GEMV32, PACK32) if fp32 else (ATTN, GEMV, PACK)
        for part, inference in ((inf, True), (trf, False)):
            assert not _of(part, *({ATTN, ATTN32, GEMV, GEMV32, PACK, PACK32} - {att_kind, gemv_kind, pack_kind}), TEMB_ROW), part
            att = _of(part, att_kind)                # B N C heads d x3: 3 x bf16 products in the fp32 inference plans only
            assert collections.Counter((b, n, c, d) for b, n, c, _, d, _ in att) == attn, (att, attn)
            assert all(h * d == c and x3 == int(fp32 and inference) for _, _, c, h, d, x3 in att), att
            assert _of(part, SINUSOID) == [(1, ch[0], 0, 0, 0, 0)], part
            gv = _of(part, gemv_kind)                # I O x-stride y-stride silu B
            assert gv == [(i, o, i, o, silu, 1) for (i, o), silu in zip(lins, (0, 1, 1))], (gv, lins)
            pk = [(k, v) for k, v in part if k in (pack_kind, IM2COL)]
            assert len(pk) == 1 and pk[0][1][:2] == (1, 4) and pk[0][1][2] % 32 == 0, pk
            if pk[0][0] == IM2COL:                   # N cin Kp D H W
                assert pk[0][1][3:] == (8, 8, 8), pk
            else:                                    # N real stored DHW internal 0: the caller's (x | cond)
                assert pk[0][1][3:] == (512, 0, 0), pk
            ups = _of(part, UPS_SPLIT32)             # N C D H W ups: the source of each Upsample conv of an fp32 inference plan
            assert [u[:5] for u in ups] == ([(1, ch[2], 2, 2, 2), (1, ch[1], 4, 4, 4)] if fp32 and inference else []), ups
            assert all(u[5] in (0, 1) for u in ups), ups
        _check_common((inf, trf), bwd, fp32, n_attn)
        assert bwd[1][1][:2] == (1, 4) and bwd[1][1][2] % 32 == 0 and bwd[1][1][3:] == (512, 0, 0), bwd[1]
        ab = _of(bwd, ATTN_BWD)                      # B N C d fp32 0
        assert collections.Counter(v[:4] for v in ab) == attn and all(v[4:] == (int(fp32), 0) for v in ab), ab
        # B I O dy-stride x-stride silu: the three linears again, last first; the first one's input needs no gradient
        dw = [(1, i, o, o, i, silu) for (i, o), silu in zip(lins[::-1], (1, 1, 0))]
        assert _of(bwd, LIN_DW) == dw and _of(bwd, LIN_DX) == dw[:2], (_of(bwd, LIN_DW), _of(bwd, LIN_DX), dw)
        assert _of(bwd, ADD) and _of(bwd, SUMPOOL), bwd
        _check_buckets(bwd, total)

    m.set_precision("bf16")
    step, = _traced(tmp_path / "step.csv", [denoise])
    assert _of(step, TEMB_ROW) == [(rows, 1, 0, 0, 0, 0)] and not _of(step, SINUSOID, GEMV, GEMV32), step
    assert collections.Counter(v[:3] + v[4:5] for v in _of(step, ATTN)) == attn
    del m

    # ---- AutoencoderKL
    vcfg = cfgs.VAE_TINY_ATTN
    v = AutoencoderKL(**vcfg)
    v.load_state_dict(ou.init_state_dict(oa.ae_param_shapes(vcfg), 2))
    v = v.to(cuda)
    img = torch.rand((1, 1, 16, 16, 16), generator=g).to(cuda)
    noise = torch.randn((1, 8, 4, 4, 4), generator=g).to(cuda)
    vshapes = {name: tuple(p.shape) for name, p in v.named_parameters()}
    n_enc = sum(1 for name in vshapes if name.startswith("encoder.") and name.endswith(".attn.to_q.weight"))
    n_dec = sum(1 for name in vshapes if name.startswith("decoder.") and name.endswith(".attn.to_q.weight"))
    assert n_enc > 0 and n_dec > 0
    vtotal = int(L.ldm_model_param_numel_total(v._h))
    dhw = 4 ** 3                                     # the latent grid: 16^3 halved twice

    def encode():
        v.eval()
        with torch.no_grad():
            state["mu"], _ = v.encode(img)

    def decode():
        with torch.no_grad():
            v.decode(state.pop("mu"))

    def vae_train_forward():
        v.train()
        recon, z_mu, z_sigma = v(img, noise)
        state["loss"] = F.mse_loss(recon, img) + 1e-3 * (z_mu.pow(2).sum() + z_sigma.pow(2).sum())

    def vae_backward():
        state.pop("loss").backward()
        v.zero_grad(set_to_none=True)

    for prec in ("bf16", "fp32"):
        fp32 = prec == "fp32"
        v.set_precision(prec)
        enc, dec, trf, bwd = _traced(tmp_path / f"vae_{prec}.csv", [encode, decode, vae_train_forward, vae_backward])
        att_kind, pack_kind = (ATTN32, PACK32) if fp32 else (ATTN, PACK)
        for part, n_att in ((enc, n_enc), (dec, n_dec), (trf, n_enc + n_dec)):
            att = _of(part, ATTN, ATTN32)            # single head: d = C
            assert att == _of(part, att_kind) and len(att) == n_att, (att, n_att)
            assert all((b, n, c, h, d) == (1, dhw, 64, 1, 64) for b, n, c, h, d, _ in att), att
            assert not _of(part, SINUSOID, GEMV, GEMV32, TEMB_ROW), part
        heads = (1, 8, dhw, 0, 0, 0)                 # B L dhw
        assert _of(enc, VAE_HEADS) == [heads] and _of(trf, VAE_HEADS) == [heads] and not _of(dec, VAE_HEADS)
        # packing: the image (a pack or the first conv's im2col), the caller's latent; the training plan's own image and latent
        pk = [(k, p[:3]) for k, p in enc if k in (pack_kind, IM2COL)]
        assert len(pk) == 1 and pk[0][1][:2] == (1, 1) and pk[0][1][2] % 32 == 0, pk
        assert [(k, p) for k, p in dec if k in (PACK, PACK32, IM2COL)] == [(pack_kind, (1, 8, 32, dhw, 0, 0))], dec[:2]
        assert [(k, p) for k, p in trf if k in (PACK, PACK32, IM2COL)] == [(pack_kind, (1, 1, 32, 4096, 1, 0)), (pack_kind, (1, 8, 32, dhw, 1, 0))]
        _check_common((enc, dec, trf), bwd, fp32, n_enc + n_dec)
        assert bwd[1][1] == (1, 1, 32, 4096, 1, 0), bwd[1]                   # marked internal
        hb, = _of(bwd, VAE_HEADS_BWD)                # N L stored-channels DHW dz-channels fp32
        assert hb[:2] == (1, 8) and hb[2] % 32 == 0 and hb[3] == dhw and hb[4] % 32 == 0 and hb[5] == int(fp32), hb
        assert all(p[:4] == (1, dhw, 64, 64) and p[4:] == (int(fp32), 0) for p in _of(bwd, ATTN_BWD))
        assert _of(bwd, SUMPOOL), bwd
        assert not _of(bwd, LIN_DX, LIN_DW)
        _check_buckets(bwd, vtotal)
