"""The plan trace (ldm_set_plan_trace) is the one externally visible rendering of the conv family's plan record (ConvRec in
csrc/ldm3d.hip): tools/plan_trace.py and ldm3d/profiling.py read its rows.  One UNet forward per precision pins the text of the
OP_CONV / OP_FINALIZE rows and ties them to what ldm_model_plan_conv_cfgs reports for the same plan."""
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
