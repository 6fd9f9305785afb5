"""Inpainting (RePaint) on the host: the schedule against known answers and an independent walk, the row table's identities in float64,
the refusals, the image-to-latent mask pooling and the command line's parsing.  No GPU."""
import math
import os
import sys

import pytest
import torch

import cfgs
import repaint_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scheduler(kind, n=10):
    from ldm3d.schedulers import DDIMScheduler, DDPMScheduler, PNDMScheduler, RFlowScheduler
    if kind == "ddpm":
        return DDPMScheduler(**dict(cfgs.SCHED, num_train_timesteps=n))
    if kind == "flow":
        sch = RFlowScheduler(num_train_timesteps=1000)
    elif kind == "pndm":
        sch = PNDMScheduler(skip_prk_steps=True, **cfgs.SCHED)
    else:
        sch = DDIMScheduler(**cfgs.SCHED)
    sch.set_timesteps(n)
    return sch


# ---- the schedule ----------------------------------------------------------------------------------------------------------------
def test_schedule_known_answers():
    from ldm3d.schedulers import repaint_schedule
    assert repaint_schedule(4, 2, 2) == [(0, False), (1, True), (0, False), (1, False), (2, False), (3, False)]
    assert repaint_schedule(3, 1, 3) == [(0, True), (0, True), (0, False), (1, True), (1, True), (1, False), (2, False)]
    for n in (1, 2, 7):
        plain = [(L, False) for L in range(n)]
        assert repaint_schedule(n) == plain and repaint_schedule(n, 3, 1) == plain           # n_resample = 1: the plain chain
        assert repaint_schedule(n, n, 4) == plain and repaint_schedule(n, n + 5, 4) == plain      # jump_length >= n_steps: no jump
    for bad in ((0, 1, 1), (4, 0, 1), (4, 1, 0)):
        with pytest.raises(ValueError):
            repaint_schedule(*bad)


def test_schedule_call_count_and_order():
    """the closed form over a small sweep, equality with the reference's block walk, and every level visited in a legal order: a call
    follows the level the previous one arrived at, or that level minus jump_length after a jump; every level is visited; a jump
    is taken from a multiple of jump_length below n_steps, exactly n_resample - 1 times"""
    from ldm3d.schedulers import repaint_schedule
    for n in range(1, 12):
        for j in range(1, 7):
            for r in range(1, 5):
                s = repaint_schedule(n, j, r)
                assert len(s) == ref.n_calls(n, j, r) == n + (r - 1) * j * ((n - 1) // j), (n, j, r)
                assert s == ref.schedule(n, j, r), (n, j, r)
                level, taken = 0, {}
                for L, jump in s:
                    assert L == level and 0 <= L < n
                    a = L + 1
                    if jump:
                        assert a % j == 0 and a < n
                        taken[a] = taken.get(a, 0) + 1
                        level = a - j
                    else:
                        level = a
                assert level == n and {L for L, _ in s} == set(range(n))
                want = {a: r - 1 for a in range(j, n, j)} if r > 1 else {}
                assert taken == want, (n, j, r)


# ---- the rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("ddpm", 1000), ("ddim", 10), ("flow", 10)])
def test_row_identities(kind, n):
    """in float64, to 1e-12: the jump carries the marginal of level a to that of level b (mean and variance), the known region's
    coefficients are those of the level arrived at, the last row's are (1, 0), slot 5 is timesteps[level], slots 0 .. 7 are the
    scheduler's own sampler row, a row without a jump has (1, 0, flags 0)"""
    from ldm3d.schedulers import _repaint_marginals, _sampler_rows, repaint_rows
    sch = _scheduler(kind, n)
    j, r = (100, 2) if kind == "ddpm" else (3, 3)
    schedule, rows = repaint_rows(sch, j, r)
    assert schedule == ref.schedule(n, j, r) and len(rows) == ref.n_calls(n, j, r)
    ts = sch.timesteps.tolist()
    base = _sampler_rows(sch, 0.0)[1]
    lv = _repaint_marginals(sch)
    assert len(lv) == n + 1
    if kind == "flow":
        assert lv == [float(t) / 1000.0 for t in ts] + [0.0]
    else:
        ac = sch.alphas_cumprod.double()
        step = 1 if kind == "ddpm" else 1000 // n
        for L in range(n):                                   # level L sits at abar[timesteps[L]]; the finished sample at abar = 1
            assert lv[L] == float(ac[int(ts[L])])
            assert int(ts[L]) - step == (int(ts[L + 1]) if L + 1 < n else -step)
        assert lv[n] == 1.0
    jumps = 0
    for (L, jump), row in zip(schedule, rows):
        assert len(row) == 16 and row[13:] == [0.0, 0.0, 0.0]
        assert row[:8] == [float(v) for v in base[L]] and row[5] == float(ts[L])
        ka, ks, ja, js, flags = row[8:13]
        a = L + 1
        assert flags == (1.0 if jump else 0.0)
        if a == n:
            assert (ka, ks) == (1.0, 0.0)
        elif kind == "flow":
            assert abs(ka - (1.0 - lv[a])) <= 1e-12 and abs(ks - lv[a]) <= 1e-12
        else:
            assert abs(ka - math.sqrt(lv[a])) <= 1e-12 and abs(ka * ka + ks * ks - 1.0) <= 1e-12
        if not jump:
            assert (ja, js) == (1.0, 0.0)
            continue
        jumps += 1
        b = a - j
        assert js > 0.0 and 0.0 <= ja < 1.0                  # a flow chain's level 0 is pure noise: a jump there keeps nothing (ja = 0)
        if kind == "flow":                                   # x_a = (1 - tau_a) x0 + tau_a e  ->  (1 - tau_b) x0 + tau_b e'
            assert abs(ja * (1.0 - lv[a]) - (1.0 - lv[b])) <= 1e-12
            assert abs(ja ** 2 * lv[a] ** 2 + js ** 2 - lv[b] ** 2) <= 1e-12
            want = ref.jump_coefs(tau_a=lv[a], tau_b=lv[b])
        else:                                                # x_a = sqrt(abar_a) x0 + sqrt(1 - abar_a) e  ->  the same at abar_b
            assert abs(ja * math.sqrt(lv[a]) - math.sqrt(lv[b])) <= 1e-12
            assert abs(ja ** 2 * (1.0 - lv[a]) + js ** 2 - (1.0 - lv[b])) <= 1e-12
            want = ref.jump_coefs(a=lv[a], b=lv[b])
        assert abs(ja - want[0]) <= 1e-12 and abs(js - want[1]) <= 1e-12
    assert jumps == (r - 1) * ((n - 1) // j) > 0


def test_prev_alpha_cumprod_is_the_steps_own():
    """abar' comes from the one place the scheduler's own rows take it from: c0 of a DDIM row is sqrt(abar'), and DDPM's c0 / c1 tables
    are built on it"""
    ddim = _scheduler("ddim", 10)
    for t in (int(t) for t in ddim.timesteps.tolist()):
        assert ddim._row(t)[2] == float(ddim._prev_alpha_cumprod(t) ** 0.5)
    assert float(ddim._prev_alpha_cumprod(0)) == 1.0
    ddpm = _scheduler("ddpm", 1000)
    for t in (0, 1, 500, 999):
        ap = ddpm._prev_alpha_cumprod(t)
        assert float(ap) == (1.0 if t == 0 else float(ddpm.alphas_cumprod[t - 1]))
        assert ddpm._row(t)[2] == float(ap ** 0.5 * ddpm.betas[t] / (1 - ddpm.alphas_cumprod[t]))


def test_eta_reaches_the_base_row():
    from ldm3d.schedulers import repaint_rows
    sch = _scheduler("ddim", 10)
    r0, r5 = repaint_rows(sch, 2, 2, 0.0)[1], repaint_rows(sch, 2, 2, 0.5)[1]
    assert all(a[4] == 0.0 for a in r0) and all(b[4] > 0.0 for b in r5[:-1])
    assert [a[8:] for a in r0] == [b[8:] for b in r5]


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from ldm3d.inferer import _check_inpaint
    from ldm3d.schedulers import REPAINT_MAX_ROWS, check_keep_mask, repaint_rows
    with pytest.raises(NotImplementedError):
        repaint_rows(_scheduler("pndm", 10))
    with pytest.raises(NotImplementedError):
        _scheduler("pndm", 10).repaint_sampler(torch.zeros((1, 4, 2, 2, 2)), torch.ones((2, 2, 2)))
    with pytest.raises(TypeError):
        repaint_rows(object())
    with pytest.raises(ValueError):                          # more UNet calls than a table is built for
        repaint_rows(_scheduler("ddpm", 1000), 500, 40)
    assert 1000 + 39 * 500 > REPAINT_MAX_ROWS
    ddim = _scheduler("ddim", 10)
    z, keep = torch.zeros((1, 4, 2, 3, 4)), torch.ones((2, 3, 4))
    assert _check_inpaint(ddim, None, None, None, 0, (2, 4, 2, 3, 4)) is None
    known, k = _check_inpaint(ddim, z, keep[None, None], None, 0, (2, 4, 2, 3, 4))
    assert known.shape == z.shape and k.shape == (2, 3, 4) and k.dtype == torch.float32
    for args in ((z, None), (None, keep)):                   # both or neither
        with pytest.raises(ValueError):
            _check_inpaint(ddim, *args, None, 0, (1, 4, 2, 3, 4))
    with pytest.raises(NotImplementedError):                 # PNDM
        _check_inpaint(_scheduler("pndm", 10), z, keep, None, 0, (1, 4, 2, 3, 4))
    with pytest.raises(NotImplementedError):                 # warm-started / inverted inpainting
        _check_inpaint(ddim, z, keep, z, 0, (1, 4, 2, 3, 4))
    with pytest.raises(NotImplementedError):
        _check_inpaint(ddim, z, keep, None, 3, (1, 4, 2, 3, 4))
    with pytest.raises(ValueError):                          # a latent of another shape / a batch that is neither 1 nor B
        _check_inpaint(ddim, z, keep, None, 0, (1, 4, 2, 3, 5))
    with pytest.raises(ValueError):
        _check_inpaint(ddim, torch.zeros((2, 4, 2, 3, 4)), keep, None, 0, (3, 4, 2, 3, 4))
    with pytest.raises(ValueError):                          # a mask of another shape
        _check_inpaint(ddim, z, torch.ones((2, 3, 5)), None, 0, (1, 4, 2, 3, 4))
    soft = keep.clone()
    soft[0, 0, 0] = 0.5
    for bad in (soft, keep * 2.0, -keep, keep * float("nan")):      # soft and otherwise non-binary masks
        with pytest.raises(ValueError):
            check_keep_mask(bad)
        with pytest.raises(ValueError):
            _check_inpaint(ddim, z, bad, None, 0, (1, 4, 2, 3, 4))
    assert check_keep_mask(torch.tensor([[[True, False]]])).tolist() == [[[1.0, 0.0]]]


# ---- image mask -> latent mask ---------------------------------------------------------------------------------------------------
def test_latent_keep_mask_is_a_min_pool():
    from ldm3d.inferer import latent_keep_mask
    keep = torch.ones((8, 8, 12))
    keep[3, 4, 5] = 0.0                                      # one regenerated image voxel regenerates the latent voxel over it
    keep[4:8, 0:4, 8:12] = 0.0                               # a whole cell
    got = latent_keep_mask(keep, 4)
    want = torch.ones((2, 2, 3))
    want[0, 1, 1] = 0.0
    want[1, 0, 2] = 0.0
    assert torch.equal(got, want) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(latent_keep_mask(keep[None, None], 4), want)
    assert torch.equal(latent_keep_mask(keep, 1), keep)
    brute = torch.stack([keep[d:d + 2, h:h + 2, w:w + 2].min() for d in range(0, 8, 2) for h in range(0, 8, 2) for w in range(0, 12, 2)])
    assert torch.equal(latent_keep_mask(keep, 2).reshape(-1), brute)
    ragged = torch.ones((5, 4, 4))                           # a trailing partial cell pools the voxels it has
    ragged[4, 0, 0] = 0.0
    assert latent_keep_mask(ragged, 4).tolist() == [[[1.0]], [[0.0]]]
    with pytest.raises(ValueError):
        latent_keep_mask(keep * 0.5, 4)
    with pytest.raises(ValueError):
        latent_keep_mask(keep[0], 4)


# ---- the command line ------------------------------------------------------------------------------------------------------------
REFUSED = [
    ["--regenerate-box", "0:4,0:4,0:4"],                                                 # without --inpaint
    ["--jump-length", "2"],
    ["--resample", "2"],
    ["--inpaint-paste"],
    ["--inpaint", "x.npz"],                                                              # no region
    ["--inpaint", "x.npz", "--regenerate-box", "0:4,0:4,0:4", "--regenerate-mask", "m.npy"],
    ["--inpaint", "x.npz", "--regenerate-box", "0:4,0:4"],
    ["--inpaint", "x.npz", "--regenerate-box", "4:4,0:4,0:4"],
    ["--inpaint", "x.npz", "--regenerate-box", "0:4,0:4,0:4", "--resample", "0"],
    ["--inpaint", "x.npz", "--regenerate-box", "0:4,0:4,0:4", "--sampler", "pndm", "--steps", "10"],
    ["--condition", "x.npz", "--inpaint", "x.npz", "--regenerate-box", "0:4,0:4,0:4", "--init-from-condition"],
    ["--condition", "x.npz", "--inpaint", "x.npz", "--regenerate-box", "0:4,0:4,0:4", "--likelihood"],
    ["--inpaint", "x.npz", "--regenerate-box", "0:4,0:4,0:4", "--chains", "2"],
]


def parse(argv, tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import inference
    env = tmp_path / "environment.json"
    env.write_text("{}")
    monkeypatch.setattr(sys, "argv", ["inference.py", "-e", str(env), "-c", os.path.join(ROOT, "config", "config_synthetic_train.json")] + argv)
    monkeypatch.delenv("LDM_PRECISION", raising=False)
    return inference.parse_cli()


@pytest.mark.parametrize("argv", REFUSED, ids=[" ".join(a[-3:]) for a in REFUSED])
def test_command_line_refuses(argv, tmp_path, monkeypatch, capsys):
    with pytest.raises(SystemExit) as e:
        parse(argv, tmp_path, monkeypatch)
    assert e.value.code != 0
    assert "error" in capsys.readouterr().err


def test_command_line_accepts(tmp_path, monkeypatch):
    ns = parse(["--condition", "x.npz", "--inpaint", "x.npz", "--regenerate-box", "1:5,0:96,10:20", "--jump-length", "2", "--resample", "3",
                "--steps", "10", "--sliding-window", "--cfg", "2.0", "--metrics", "--inpaint-paste"], tmp_path, monkeypatch)
    assert ns.regenerate == ((1, 5), (0, 96), (10, 20)) and ns.jump_length == 2 and ns.resample == 3 and ns.inpaint_paste
    ns = parse(["--condition", "x.npz", "--inpaint", "x.npz", "--regenerate-mask", "m.npy", "--ensemble", "2", "--sampler", "ddpm"], tmp_path, monkeypatch)
    assert ns.regenerate is None and ns.regenerate_mask == "m.npy"
    assert parse(["--steps", "10"], tmp_path, monkeypatch).inpaint is None
