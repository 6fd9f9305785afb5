"""grad_accum_kernel on its own through ldm_op_grad_accumulate (-m gpu): every alignment of the range's start, every path through the
scalar head / float4 body / scalar tail, both modes, against torch's fp32 arithmetic bit for bit, with guard bands on both sides."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64                                   # sentinel floats on each side of the range (64 floats keep the base 16-byte aligned)
FIRSTS = (0, 1, 2, 3, 5)                     # floats past a 16-byte-aligned base
SIZES = (1, 3, 4, 5, 7, 255, 1024, 4099, 2 ** 20 + 3)
NMAX = max(SIZES)
BAD_ARG = -1


@pytest.fixture(scope="module")
def data(cuda):
    """One (g, acc0) pair for every case (slices of it), never written, and one pair of work buffers with room for the guards."""
    gen = torch.Generator().manual_seed(31)
    g = (torch.randn(NMAX, generator=gen) * torch.exp2(torch.randint(-6, 6, (NMAX,), generator=gen).float())).to(cuda)
    acc0 = (torch.randn(NMAX, generator=gen) * torch.exp2(torch.randint(-6, 6, (NMAX,), generator=gen).float())).to(cuda)
    size = GUARD + max(FIRSTS) + NMAX + GUARD
    wa, wg = torch.empty(size, device=cuda), torch.empty(size, device=cuda)
    assert wa.data_ptr() % 16 == 0 and wg.data_ptr() % 16 == 0
    sent = torch.arange(size, dtype=torch.float32, device=cuda) * 0.5 + 7.0
    return g, acc0, wa, wg, sent


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(L, data, first, n, s, assign, acc_init=None, g_src=None):
    """Lays the case out between the sentinels, runs the entry, checks both guard bands and g, returns the range of acc."""
    g, acc0, wa, wg, sent = data
    lo = GUARD + first
    wa.copy_(sent)
    wg.copy_(sent)
    wg[lo:lo + n].copy_(g[:n] if g_src is None else g_src)
    wa[lo:lo + n].copy_(acc0[:n] if acc_init is None else acc_init)
    g_before = wg.clone()
    rc = L.ldm_op_grad_accumulate(wa.data_ptr() + 4 * lo, wg.data_ptr() + 4 * lo, n, s, int(assign), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(wa[:lo], sent[:lo]) and torch.equal(wa[lo + n:], sent[lo + n:]), (first, n, "guard band of acc written")
    assert torch.equal(_bits(wg), _bits(g_before)), (first, n, "g written")
    return wa[lo:lo + n].clone()


def _ref(data, n, s, assign):
    g, acc0 = data[0][:n], data[1][:n]
    p = g * torch.tensor(s, dtype=torch.float32, device=g.device)      # one fp32 rounding
    return p if assign else acc0 + p                                    # and a second one, in a launch of its own (no fma)


@pytest.mark.parametrize("assign", [1, 0], ids=["assign", "add"])
@pytest.mark.parametrize("s", [1.0, 0.5, 0.25], ids=["s1", "s0.5", "s0.25"])
def test_power_of_two_scales_equal_torch_bit_for_bit(built_lib, data, s, assign):
    """g * s is exact for a power of two, so one rounding remains whether or not the compiler contracts: bitwise equality with torch.  The
    negative control: the other mode's reference must NOT match (the data would let a swapped mode through otherwise)."""
    for n in SIZES:
        ref, wrong = _ref(data, n, s, assign), _ref(data, n, s, not assign)
        assert not torch.equal(_bits(ref), _bits(wrong))
        for first in FIRSTS:
            nan = torch.full((n,), float("nan"), device=ref.device) if assign else None     # assign mode must not read acc
            out = _run(built_lib, data, first, n, s, assign, acc_init=nan)
            assert bool(torch.isfinite(out).all()), (first, n)
            assert torch.equal(_bits(out), _bits(ref)), (first, n, int((_bits(out) != _bits(ref)).sum()))
            assert not torch.equal(_bits(out), _bits(wrong)), (first, n)


@pytest.mark.parametrize("assign", [1, 0], ids=["assign", "add"])
def test_one_third_scale_stays_within_two_roundings_of_fp64(built_lib, data, assign):
    """s = float(1/3): the assign result is torch's g * s bit for bit; the add result lies within 2^-23 (|acc| + |g s|) of the fp64 value
    -- at most two fp32 roundings, each at most 2^-24 of a quantity no larger than that sum, contracted into an fma or not."""
    s = float(torch.tensor(1.0 / 3.0, dtype=torch.float32))             # the value the C float holds
    g, acc0 = data[0], data[1]
    for n in SIZES:
        for first in FIRSTS:
            nan = torch.full((n,), float("nan"), device=g.device) if assign else None
            out = _run(built_lib, data, first, n, s, assign, acc_init=nan)
            if assign:
                assert torch.equal(_bits(out), _bits(_ref(data, n, s, True))), (first, n)
                assert not torch.equal(_bits(out), _bits(_ref(data, n, s, False))), (first, n)
                continue
            p64 = g[:n].double() * s
            exact = acc0[:n].double() + p64
            bound = 2.0 ** -23 * (acc0[:n].double().abs() + p64.abs())
            err = (out.double() - exact).abs()
            assert bool((err <= bound).all()), (first, n, float((err / bound.clamp_min(1e-300)).max()))
            assert not bool(((out.double() - p64).abs() <= bound).all()), (first, n)      # the assign value would not pass


@pytest.mark.parametrize("assign", [1, 0], ids=["assign", "add"])
def test_nan_and_infinities_in_g_arrive_in_acc(built_lib, data, assign):
    """Ordinary arithmetic: NaN and +-inf at the head, in the float4 body and in the tail of the range land where they were."""
    n, first = 4099, 3
    g = data[0][:n].clone()
    spots = {0: float("nan"), 1: float("inf"), 2: float("-inf"), 1000: float("nan"), 1001: float("inf"), 1002: float("-inf"),
             n - 2: float("-inf"), n - 1: float("nan")}
    for i, v in spots.items():
        g[i] = v
    out = _run(built_lib, data, first, n, 0.5, assign, g_src=g)
    p = g * 0.5
    ref = p if assign else data[1][:n] + p
    assert torch.equal(torch.isnan(out), torch.isnan(ref)) and int(torch.isnan(out).sum()) == 3
    ok = ~torch.isnan(ref)
    assert torch.equal(out[ok], ref[ok]) and int(torch.isinf(out).sum()) == 5
    for i, v in spots.items():
        assert (out[i] != out[i]) if v != v else float(out[i]) == v, i


def test_empty_and_bad_arguments_launch_nothing(built_lib, cuda):
    L = built_lib
    st = torch.cuda.current_stream().cuda_stream
    acc = torch.full((64,), float("nan"), device=cuda)
    g = torch.ones(64, device=cuda)
    assert L.ldm_op_grad_accumulate(acc.data_ptr(), g.data_ptr(), 0, 1.0, 1, st) == 0
    assert L.ldm_op_grad_accumulate(None, None, 0, 1.0, 1, st) == 0
    assert L.ldm_op_grad_accumulate(None, g.data_ptr(), 64, 1.0, 1, st) == BAD_ARG
    assert L.ldm_op_grad_accumulate(acc.data_ptr(), None, 64, 1.0, 0, st) == BAD_ARG
    assert L.ldm_op_grad_accumulate(acc.data_ptr(), g.data_ptr(), -1, 1.0, 1, st) == BAD_ARG
    assert L.ldm_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(acc).all()) and bool((g == 1.0).all())


def test_a_pair_with_different_misalignments_runs_scalar(built_lib, cuda):
    """Outside the flat buffers acc and g need not share their misalignment: the entry then takes the scalar path for the whole range."""
    gen = torch.Generator().manual_seed(5)
    src = torch.randn(1031, generator=gen).to(cuda)
    wa, wg = torch.zeros(1100, device=cuda), torch.zeros(1100, device=cuda)
    wg[2:2 + 1031].copy_(src)
    wa[1:1 + 1031].fill_(3.0)
    rc = built_lib.ldm_op_grad_accumulate(wa.data_ptr() + 4, wg.data_ptr() + 8, 1031, 0.25, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(wa[1:1 + 1031], 3.0 + src * 0.25) and float(wa[0]) == 0.0 and bool((wa[1032:] == 0).all())
