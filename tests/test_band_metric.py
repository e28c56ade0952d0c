"""Pin gpu_util.band_rel_l1 on the CPU, and with it the blind spot it closes: on a deep encoder the whole-map relative L1
cannot see a lost border row.  The map is the ResNet oracle's own float64 heat-map of the production-width net
(bottleneck widths 256 ... 2048 as in ResNet-101) on a 160 x 96 image; nothing here needs a GPU."""
import numpy as np
import pytest

from conftest import rel_l1
from gpu_util import band_errors, band_rel_l1
from lrp_imagecaptioning_amd.synthetic import resnet_weights
from oracle import resnet_lrp_ref as RN

WIDE = ((64, 1), (128, 1), (256, 2), (512, 1))
TOL = 1e-4                                                   # the project's parity bar on a whole map


@pytest.fixture(scope="module")
def wide_map():
    rs = np.random.RandomState(0)
    w = resnet_weights(rs, WIDE, stem=64, bias_std=0.2)
    spec = RN.resnet_spec(WIDE, stem=64)
    X = rs.uniform(-120, 130, size=(1, 160, 96, 3)).astype(np.float32)
    feat = RN.forward(w, spec, X)
    assert feat.shape == (1, 5, 3, 2048)
    R = (rs.standard_normal(feat.shape) * feat).astype(np.float32)
    ref = RN.analyze(w, spec, X, R)[0]
    ref.setflags(write=False)
    return ref


def test_identical_maps_score_zero(wide_map):
    assert rel_l1(wide_map, wide_map) == 0.0
    assert band_rel_l1(wide_map, wide_map) == 0.0
    rows, cols = band_errors(wide_map, wide_map)
    assert rows.shape == (160,) and cols.shape == (96,) and not rows.any() and not cols.any()


def test_a_lost_last_row_passes_the_whole_map_bar_and_fails_the_band(wide_map):
    out = wide_map.copy()
    out[-1] = 0.0
    assert rel_l1(out, wide_map) < TOL                       # the blind spot, pinned
    assert band_rel_l1(out, wide_map) == 1.0
    assert band_rel_l1(out, wide_map, where=True) == (1.0, "row 159")
    rows, cols = band_errors(out, wide_map)
    assert (rows[:-1] == 0).all() and cols.max() < 0.2       # the columns see one pixel each: the row band is what tells


def test_a_shifted_interior_row_passes_the_whole_map_bar_and_fails_the_band(wide_map):
    """One interior row moved by one pixel along itself: |shifted - ref| is at most twice the row's mass, so on the
    interior row with the least mass the whole map stays inside 1e-4 while the row's own band is of order 1."""
    shares = np.abs(wide_map).sum(axis=(1, 2)) / np.abs(wide_map).sum()
    r = 1 + int(np.argmin(shares[1:-1]))
    assert 2.0 * shares[r] < TOL
    out = wide_map.copy()
    out[r, 1:] = wide_map[r, :-1]
    out[r, 0] = 0.0
    assert rel_l1(out, wide_map) < TOL
    band, at = band_rel_l1(out, wide_map, where=True)
    assert at == "row %d" % r and band > 0.5, (at, band)


def test_zero_mass_bands():
    """A band without reference mass must be exactly zero in `out`: 0 if it is, inf if not; other bands unaffected."""
    ref = np.ones((3, 4, 2))
    ref[1] = 0.0
    out = ref.copy()
    assert band_rel_l1(out, ref) == 0.0
    out[1, 2, 0] = 1e-30
    assert band_rel_l1(out, ref, where=True) == (np.inf, "row 1")
    out = ref.copy()
    out[0, 3, 1] = 1.5                                       # row 0 holds 8, column 3 holds 4: the column is the worst band
    v, at = band_rel_l1(out, ref, where=True)
    assert at == "col 3" and v == 0.5 / 4.0
    with pytest.raises(ValueError):
        band_rel_l1(np.zeros((2, 3, 4, 3)), np.zeros((2, 3, 4, 3)))
