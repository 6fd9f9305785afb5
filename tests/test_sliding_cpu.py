"""Sliding-window geometry on the host (no GPU): window starts (MONAI's dense_patch_slices rule), cover, per-axis weight tables."""
import itertools

import numpy as np
import pytest

import cfgs

CASES = [(24, 24, 0.25), (25, 24, 0.25), (33, 24, 0.25), (43, 24, 0.25), (25, 24, 0.0), (48, 24, 0.0), (49, 24, 0.0),
         (33, 24, 0.5), (43, 24, 0.5), (33, 24, 0.75), (97, 24, 0.75), (13, 8, 0.25), (22, 8, 0.25), (17, 8, 0.5),
         (17, 8, 0.0), (9, 8, 0.75), (100, 16, 0.25), (31, 16, 0.5), (8, 8, 0.5), (5, 3, 0.9), (7, 1, 0.25)]


def monai_rule(dim, roi, overlap):
    """dense_patch_slices / _get_scan_interval as MONAI writes them (MONAI is not installed)."""
    interval = roi if roi == dim else (int(roi * (1 - overlap)) or 1)
    num = -(-dim // interval)
    scan = next((d for d in range(num) if d * interval + roi >= dim), None)
    n = scan + 1 if scan is not None else 1
    out = []
    for i in range(n):
        s = i * interval
        s -= max(s + roi - dim, 0)
        out.append(s)
    return out


@pytest.mark.parametrize("dim,roi,overlap", CASES)
def test_window_starts_follow_monai_and_cover_every_voxel(dim, roi, overlap):
    from ldm3d.sliding import window_starts
    st = window_starts(dim, roi, overlap)
    assert st == monai_rule(dim, roi, overlap)
    assert st[0] == 0 and st[-1] == dim - roi                      # the last window is flush with the far end
    assert len(set(st)) == len(st) and st == sorted(st)
    cov = np.zeros(dim, dtype=int)
    for s in st:
        cov[s:s + roi] += 1
    assert (cov >= 1).all()


@pytest.mark.parametrize("mode", ["gaussian", "constant"])
@pytest.mark.parametrize("dim,roi,overlap", CASES)
def test_axis_tables_sum_to_one_and_cover_table_is_exact(dim, roi, overlap, mode):
    from ldm3d.sliding import axis_profile, axis_tables, window_starts
    st = window_starts(dim, roi, overlap)
    tab, cover = axis_tables(dim, roi, st, axis_profile(roi, mode))
    assert tab.dtype == np.float64 and tab.shape == (len(st), roi)
    tot = np.zeros(dim)
    for i, s in enumerate(st):
        tot[s:s + roi] += tab[i]
    assert np.abs(tot - 1.0).max() <= 1e-12
    for p in range(dim):
        inside = [i for i, s in enumerate(st) if s <= p < s + roi]
        assert (cover[p, 0], cover[p, 1]) == (inside[0], len(inside))
    if len(st) == 1:
        assert (tab == 1.0).all()


def test_window_grid_order_and_single_window_tables():
    from ldm3d.sliding import WindowGrid
    g = WindowGrid((33, 25, 43), 24)
    assert g.n == (2, 2, 3) and g.n_windows == 12
    assert g.starts == list(itertools.product([0, 9], [0, 1], [0, 18, 19]))
    one = WindowGrid((8, 8, 8), (8, 8, 8))
    assert one.n_windows == 1 and all((t == 1.0).all() and (t.astype(np.float32) == 1.0).all() for t in one.tables64)
    small = WindowGrid((6, 30, 8), 8)                                # roi is clipped to the volume per axis
    assert small.roi == (6, 8, 8) and small.n[0] == 1
    g_c = WindowGrid((33, 25, 43), 24, mode="constant")
    assert g_c.tables64[2][1][2] == 1.0 / 3.0 and g_c.tables64[2][0][0] == 1.0   # p = 20: windows 0, 1, 2; p = 0: window 0 alone
    with pytest.raises(ValueError):
        WindowGrid((33, 25, 43), 24, mode="triangle")
    with pytest.raises(ValueError):
        WindowGrid((33, 25, 43), 24, overlap=1.0)


def test_gaussian_profile_is_centred_and_symmetric():
    from ldm3d.sliding import axis_profile
    g = axis_profile(24, "gaussian", 0.125)
    assert np.allclose(g, g[::-1], rtol=0, atol=0) and g.max() < 1.0 and g[11] == g[12]
    assert np.isclose(g[0], np.exp(-(11.5 ** 2) / (2 * 3.0 ** 2)))
    assert (axis_profile(7, "constant") == 1.0).all()


def test_window_the_unet_cannot_take_is_refused(built_lib):
    from ldm3d import _lib
    from ldm3d.networks import DiffusionModelUNet
    from ldm3d.sliding import WindowGrid
    unet = DiffusionModelUNet(**cfgs.UNET_TINY)                      # 3 levels: windows must be multiples of 4
    WindowGrid((13, 22, 17), 8).check_model(unet)
    for roi in ((6, 8, 8), (8, 8, 10), (7, 7, 7)):
        with pytest.raises(_lib.LdmError, match="odd spatial size"):
            WindowGrid((13, 22, 17), roi).check_model(unet)
    with pytest.raises(_lib.LdmError):                               # roi clipped to an odd dimension
        WindowGrid((5, 22, 17), 8).check_model(unet)
