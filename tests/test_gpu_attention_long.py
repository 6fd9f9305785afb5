"""The long-sequence form of the bf16 attention forward (-m gpu): head dimension 64, N >= 1024 and fewer than 128 (tile, head, batch)
triples, the case launch_attn_fwd gives to attn_fwd_kernel<4, 2, true, 64, 3> (knob LDM_ATTN_LONG, csrc/attention.h): 4 key groups of
2 waves, three K/V tiles in flight per group, the groups' (max, sum, O) partials merged through LDS.

Every case goes through ldm_op_attention and is compared with fp64 softmax attention on the CPU on the same bf16-rounded q, k, v.
Bound: the 8e-3 rel-L2 of tests/test_gpu_ops.py::test_attention (P and the output are each rounded to bf16, ~2^-9 relative each)."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from util import bf16_round, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 8e-3
KT = 64                       # keys per tile


def _split(z, b, n, h):
    return z.reshape(b, n, h, 64).permute(0, 2, 1, 3)


def _make_qkv(b, n, c, kind):
    """kind "random": the inputs of test_attention.  "late" / "early": small random q and k, except that the first channel of every head
    is 8 in every query and 2 + level / 8 in a key, where level is the key's tile index ("late") or the number of tiles after it
    ("early"; both exact in bf16).  A tile's scores then lie 0.125 above (below) those of the tile before it, far more than the random
    part (sigma about 0.01) moves a tile's maximum, so every query's tile maximum rises (falls) strictly from tile to tile, a partial
    last tile included."""
    g = torch.Generator().manual_seed(1000 * n + c + len(kind))
    qkv = torch.randn((b, n, 3 * c), generator=g)
    if kind == "random":
        qkv[..., :2 * c] *= 1.7
        return bf16_round(qkv)
    qkv[..., :2 * c] *= 0.1
    level = torch.arange(n) // KT
    if kind == "early":
        level = level.max() - level
    qkv[..., 0:c:64] = 8.0                                                # q
    qkv[..., c:2 * c:64] = (2.0 + level.float() / 8.0)[None, :, None]     # k
    return bf16_round(qkv)


@functools.lru_cache(maxsize=None)
def _case(b, n, c, kind):
    """(bf16-rounded qkv, fp64 reference output, fp64 scaled scores); computed once per case and shared, never modified."""
    qkv = _make_qkv(b, n, c, kind)
    h = c // 64
    q, k, v = (_split(z.double(), b, n, h) for z in (qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]))
    s = q @ k.transpose(-1, -2) * 0.125
    ref = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(b, n, c)
    return qkv, ref, s


def _run(cuda, lib, qkv, b, n, c):
    from ldm3d import _lib
    dq = qkv.to(torch.bfloat16).to(cuda)
    out = torch.full((b, n, c), float("nan"), dtype=torch.bfloat16, device=cuda)
    _lib.check(lib.ldm_op_attention(dq.data_ptr(), out.data_ptr(), b, n, c, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.float().cpu()


def _check(got, ref):
    bad = (~torch.isfinite(got)).any(dim=-1)
    assert not bool(bad.any()), f"{int(bad.sum())} output rows are not finite"
    err = rel_l2(got, ref.float())
    print(f"rel-L2 vs fp64 {err:.3e}")
    assert err <= TOL, err


@pytest.mark.parametrize("b,n,c", [(1, 1024, 64),       # the dispatch threshold, 16 full tiles, one head
                                   (1, 1025, 128),      # a last tile with one valid key
                                   (1, 1030, 256),      # ragged tile; unequal tile counts per group
                                   (2, 1088, 192),      # batch 2, three heads, 17 tiles, grid 102 < 128
                                   (1, 1728, 256)])     # the workload's shape
def test_long_form_against_fp64(cuda, built_lib, b, n, c):
    assert n >= 1024 and ((n + 63) // 64) * (c // 64) * b < 128          # the shape takes the long-sequence case
    qkv, ref, _ = _case(b, n, c, "random")
    _check(_run(cuda, built_lib, qkv, b, n, c), ref)


def _tile_max(s):
    n = s.shape[-1]
    pad = (-n) % KT
    s = torch.nn.functional.pad(s, (0, pad), value=float("-inf"))
    return s.reshape(*s.shape[:-1], -1, KT).amax(dim=-1)                  # [b][h][query][tile]


@pytest.mark.parametrize("n", [1030, 1728])
def test_late_maxima(cuda, built_lib, n):
    """The score maximum of every query grows from each key tile to the next: the running max moves in every tile of every group and
    the rescale of O runs each time."""
    qkv, ref, s = _case(1, n, 256, "late")
    tm = _tile_max(s)
    assert bool((tm[..., 1:] > tm[..., :-1]).all())                       # the construction does what it says
    _check(_run(cuda, built_lib, qkv, 1, n, 256), ref)


@pytest.mark.parametrize("n", [1030, 1728])
def test_early_maximum(cuda, built_lib, n):
    """The score maximum of every query sits in the first tile and the tile maxima fall from there: after a group's first tile alpha == 1
    and the rescale is skipped everywhere."""
    qkv, ref, s = _case(1, n, 256, "early")
    tm = _tile_max(s)
    assert bool((tm[..., 1:] < tm[..., :-1]).all())
    _check(_run(cuda, built_lib, qkv, 1, n, 256), ref)


def test_log_sum_exp_rows_are_still_written(cuda, built_lib):
    """The training forward's lse output (ldm_op_attention_train takes the same launch): 1e-5 rel-L2 as test_attention_backward."""
    from ldm3d import _lib
    b, n, c = 1, 1030, 256
    qkv, ref, s = _case(b, n, c, "random")
    dq = qkv.to(torch.bfloat16).to(cuda)
    out = torch.empty((b, n, c), dtype=torch.bfloat16, device=cuda)
    lse = torch.full((b, c // 64, n), float("nan"), dtype=torch.float32, device=cuda)
    _lib.check(built_lib.ldm_op_attention_train(dq.data_ptr(), out.data_ptr(), lse.data_ptr(), b, n, c, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    _check(out.float().cpu(), ref)
    assert rel_l2(lse.cpu(), torch.logsumexp(s, dim=-1).float()) <= 1e-5


def test_bit_stable_eager_and_graph(cuda, built_lib):
    """Three eager launches and three graph replays give identical bits (the groups merge in a fixed order)."""
    from ldm3d import _lib
    b, n, c = 1, 1030, 256
    qkv, ref, _ = _case(b, n, c, "random")
    dq = qkv.to(torch.bfloat16).to(cuda)
    out = torch.empty((b, n, c), dtype=torch.bfloat16, device=cuda)
    outs = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            out.fill_(float("nan"))
            _lib.check(built_lib.ldm_op_attention(dq.data_ptr(), out.data_ptr(), b, n, c, side.cuda_stream))
            side.synchronize()
            outs.append(out.cpu().clone())
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(built_lib.ldm_op_attention(dq.data_ptr(), out.data_ptr(), b, n, c, torch.cuda.current_stream().cuda_stream))
    for _ in range(3):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        outs.append(out.cpu().clone())
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16))
    _check(outs[0].float(), ref)


_KNOB_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np, torch
import test_gpu_attention_long as t
from ldm3d import _lib
b, n, c = 1, 1728, 256
qkv, _, _ = t._case(b, n, c, "random")
np.save(sys.argv[2], t._run(torch.device("cuda:0"), _lib.lib(), qkv, b, n, c).numpy())
"""


def test_knob_arms_both_meet_the_bound(cuda, built_lib, tmp_path):
    """LDM_ATTN_LONG = 0 (8 groups of 2 waves, one tile in flight) and 1 on the workload's shape, each in a child process (the knob is
    read once per process): both meet the fp64 bound.  They need not agree bit for bit: the tile-to-group assignment changes the fp32
    summation order; their mutual rel-L2 is printed."""
    import numpy as np
    _, ref, _ = _case(1, 1728, 256, "random")
    outs = {}
    for arm in (0, 1):
        f = tmp_path / f"arm{arm}.npy"
        r = subprocess.run([sys.executable, "-c", _KNOB_CHILD, ROOT, str(f)], env=dict(os.environ, LDM_ATTN_LONG=str(arm)),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[arm] = torch.from_numpy(np.load(f))
        _check(outs[arm], ref)
    print(f"LDM_ATTN_LONG 1 vs 0: mutual rel-L2 {rel_l2(outs[1], outs[0]):.3e}")
