"""CPU checks of the perturbation analysis (innvestigate/tools/perturbate.py): the numpy restatement
(tests/perturbation_ref.py) against the reference's own outputs (tests/golden/perturbation_*.npz), the argument validation
of `Perturbation`, the region geometry and the seeded random order (no GPU needed)."""
import ctypes

import numpy as np
import pytest

import perturbation_ref as ref
from lrp_imagecaptioning_amd import _capi
from lrp_imagecaptioning_amd import engine as E
from lrp_imagecaptioning_amd import perturbation as PB


@pytest.fixture(scope="module", params=ref.GOLDENS)
def golden(request):
    return ref.load_golden(request.param)


def test_golden_inputs_have_well_separated_region_means(golden):
    assert ref.min_relative_gap(golden["aggregated"]) >= 1e-3
    assert ref.min_relative_gap(ref.region_scores(golden["analysis"], tuple(golden["region"]))) >= 1e-3


def test_restatement_ranks_equal_the_reference(golden):
    region = tuple(golden["region"])
    s = ref.region_scores(golden["analysis"], region)
    assert s.shape == golden["aggregated"].shape
    # the reference's float32 means against the float64 ones: n terms of magnitude <= max|a| added in float32
    a = np.abs(golden["analysis"]).max()
    assert np.abs(s - golden["aggregated"]).max() <= (region[0] * region[1] + 3) * 2.0 ** -24 * a
    assert np.array_equal(ref.ranks_from_scores(s), golden["ranks"])
    assert np.array_equal(ref.region_ranks(golden["analysis"], region), golden["ranks"])


@pytest.mark.parametrize("fn", ref.FUNCTIONS)
@pytest.mark.parametrize("ri", range(len(ref.RANGES)))
def test_restatement_outputs_match_the_reference(golden, fn, ri):
    region = tuple(golden["region"])
    for ki, k in enumerate(golden["ks"]):
        got = ref.perturbate(golden["x"], golden["ranks"], k, region, fn, value_range=ref.RANGES[ri])
        ref.check_against_golden(golden, fn, ki, ri, got)


def test_reference_perturbs_channel_zero_only(golden):
    x = golden["x"]
    if x.shape[-1] == 1:
        return                                                         # the one-channel fixture has nothing to leave alone
    for fn in ref.FUNCTIONS:
        y = ref.golden_output(golden, fn, 3, 0)                        # k = 5, no value range
        assert (y[..., 0] != x[..., 0]).any()
        assert np.array_equal(y[..., 1:], x[..., 1:])


def test_restatement_ties_nan_and_orders():
    s = np.array([[1.0, 3.0, 1.0, np.nan, 3.0, -0.0, 0.0, np.nan]])
    assert ref.ranks_from_scores(s).tolist() == [[2, 0, 3, 6, 1, 4, 5, 7]]
    assert ref.ranks_from_scores(np.zeros((1, 5))).tolist() == [[0, 1, 2, 3, 4]]        # all equal: raster order
    a = np.random.RandomState(0).randn(2, 18, 18, 3)
    assert np.array_equal(ref.region_ranks(a, (9, 9), negate=True), 3 - ref.region_ranks(a, (9, 9)))


# ---------------------------------------------------------------------------------------------------- the product, host side
def test_geometry():
    assert E.perturb_geometry(224, 224, (9, 9)) == (25, 25, 0, 0)      # one row / column after: 625 regions
    assert E.perturb_geometry(18, 27, (9, 9)) == (2, 3, 0, 0)
    assert E.perturb_geometry(20, 29, (9, 9)) == (3, 4, 3, 3)
    assert E.perturb_geometry(23, 23, (4, 6)) == (6, 4, 0, 0)
    for H, W, r in [(224, 224, (9, 9)), (20, 29, (9, 9)), (5, 7, (9, 9)), (23, 23, (4, 6)), (32, 32, (9, 9))]:
        assert E.perturb_geometry(H, W, r) == ref.geometry(H, W, r)
    with pytest.raises(ValueError):
        E.perturb_geometry(18, 20, (9, 9))                             # the reference's assert (perturbate.py:107)
    with pytest.raises(ValueError):
        ref.geometry(18, 20, (9, 9))
    with pytest.raises(NotImplementedError):
        E.perturb_geometry(224, 224, (3, 3))                           # 5625 regions
    with pytest.raises(NotImplementedError):
        E.perturb_geometry(224, 224, (0, 3))
    assert E.perturb_geometry(192, 192, (3, 3)) == (64, 64, 0, 0)      # 4096: the limit itself


def test_perturbation_argument_validation():
    p = PB.Perturbation("zeros")
    assert (p.num_perturbed_regions, p.region_shape, p.reduce_function, p.aggregation_function, p.pad_mode, p.in_place,
            p.value_range, p.channels) == (0, (9, 9), "mean", "mean", "reflect", False, None, "first")
    for f in ("zeros", "mean", "invert", "gaussian"):
        assert PB.Perturbation(f).perturbation_function == f
    assert PB.Perturbation(np.zeros_like).perturbation_function == "zeros"
    assert PB.Perturbation(np.mean).perturbation_function == "mean"
    p = PB.Perturbation("mean", reduce_function=np.max, aggregation_function=np.mean, channels="all", value_range=(-1, 1))
    assert (p.reduce_function, p.aggregation_function, p.channels) == ("max", "mean", "all")
    with pytest.raises(ValueError, match="not known"):
        PB.Perturbation("ones")
    with pytest.raises(TypeError):
        PB.Perturbation(3)
    with pytest.raises(NotImplementedError):
        PB.Perturbation(lambda x: x * 0)
    with pytest.raises(NotImplementedError):
        PB.Perturbation("zeros", reduce_function=np.median)
    with pytest.raises(NotImplementedError):
        PB.Perturbation("zeros", aggregation_function=np.sum)
    with pytest.raises(ValueError):
        PB.Perturbation("zeros", reduce_function="median")
    with pytest.raises(NotImplementedError):
        PB.Perturbation("zeros", pad_mode="edge")
    with pytest.raises(ValueError):
        PB.Perturbation("zeros", channels="last")
    with pytest.raises(ValueError):
        PB.Perturbation("zeros", value_range=(1, -1))
    with pytest.raises(ValueError):
        PB.Perturbation("zeros", region_shape=(0, 9))


def test_mixed_divisibility_raises_before_any_device_work():
    x = np.zeros((1, 18, 20, 3), dtype=np.float32)
    p = PB.Perturbation("zeros", 1)
    with pytest.raises(ValueError, match="107"):
        p.perturbate_on_batch(x, x)
    with pytest.raises(ValueError, match="107"):
        p.region_ranks(x)
    with pytest.raises(ValueError):
        p.perturbate_on_batch(x, x[:, :9])


def test_random_order_is_seeded():
    a, b = PB.random_ranks(7, 625, 3), PB.random_ranks(7, 625, 3)
    assert a.dtype == np.int32 and a.shape == (7, 625) and np.array_equal(a, b)
    assert (np.sort(a, axis=1) == np.arange(625)).all()
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a, PB.random_ranks(7, 625, 4))
    with pytest.raises(ValueError):
        PB.CaptionPerturbationAnalysis(None, PB.Perturbation("zeros"), order="best")


def test_c_entries_validate_before_any_device_work():
    lib = _capi.load()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    f = ctypes.c_float
    assert lib.lrp_abi_version() == 10
    assert lib.lrp_perturb_ranks(p, 0, 1, 18, 20, 3, 9, 9, 0, 0, 0, p, None, None) == _capi.LRP_ERR_INVALID
    assert b"107" in lib.lrp_last_error()
    assert lib.lrp_perturb_ranks(p, 0, 1, 224, 224, 3, 3, 3, 0, 0, 0, p, None, None) == _capi.LRP_ERR_RANGE
    assert lib.lrp_perturb_ranks(p, 0, 1, 18, 18, 3, 0, 9, 0, 0, 0, p, None, None) == _capi.LRP_ERR_RANGE
    assert lib.lrp_perturb_ranks(p, 0, 1, 18, 18, 3, 9, 9, 2, 0, 0, p, None, None) == _capi.LRP_ERR_INVALID
    assert lib.lrp_perturb_ranks(None, 0, 1, 18, 18, 3, 9, 9, 0, 0, 0, p, None, None) == _capi.LRP_ERR_INVALID
    assert lib.lrp_perturb_apply(p, p, p, p, None, p, 1, 1, 18, 20, 3, 9, 9, 0, 0, 0, f(0), f(0), None) == _capi.LRP_ERR_INVALID
    assert lib.lrp_perturb_apply(p, p, p, p, None, p, 1, 1, 18, 18, 3, 9, 9, 3, 0, 0, f(0), f(0), None) == _capi.LRP_ERR_INVALID
    assert lib.lrp_perturb_apply(p, p, p, p, None, p, 1, 1, 18, 18, 3, 9, 9, 0, 0, 1, f(1), f(-1), None) == _capi.LRP_ERR_INVALID
    assert lib.lrp_perturb_apply(p, p, p, p, None, p, 1, 1, 224, 224, 3, 2, 2, 0, 0, 0, f(0), f(0), None) == _capi.LRP_ERR_RANGE
    assert lib.lrp_perturb_word_scores(None, p, p, p, 1, p, p, None) == _capi.LRP_ERR_INVALID
