"""The plan trace (ldm_set_plan_trace) is the one externally visible rendering of the plan records (ConvRec, GnRec, WgradRec in
csrc/ldm3d.hip): tools/plan_trace.py and ldm3d/profiling.py read its rows.  One UNet forward per precision pins the text of the
OP_CONV / OP_FINALIZE rows and ties them to what ldm_model_plan_conv_cfgs reports for the same plan; one inference forward and one
training step per precision tie the GroupNorm, weight-gradient and light-GEMM rows to the model's own parameter shapes."""
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
