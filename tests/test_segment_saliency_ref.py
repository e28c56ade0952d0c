"""CPU checks of the LIME / KernelSHAP restatement (tests/segment_saliency_ref.py), of the bar the device fit is held to, of the
host-side size thresholds, and of the four operators' argument checks (which run before any HIP call)."""
import ctypes

import numpy as np
import pytest

import segment_saliency_ref as ref
from lrp_imagecaptioning_amd import saliency as SAL


@pytest.mark.parametrize("d", [4, 5])
def test_enumeration_fit_equals_brute_force_shapley(d):
    rs = np.random.RandomState(d)
    v = rs.randn(2 ** d, 3)                                             # three random set functions
    bits, wtab = ref.enumeration(d)
    assert np.array_equal(wtab, SAL.shapley_weights(d))
    phi, icpt = ref.fit(bits, wtab, v[1:-1] - v[0], d, 0.0, delta=v[-1] - v[0])
    want = ref.shapley_brute(v, d)                                      # (d, 3)
    assert np.abs(phi.T - want).max() <= 1e-12 and not icpt.any()
    assert np.abs(phi.sum(axis=1) - (v[-1] - v[0])).max() <= 1e-12      # efficiency


@pytest.mark.parametrize("shapley", [False, True])
@pytest.mark.parametrize("case,ridge", ref.FIT_RUNS)
def test_cholesky_on_the_normal_equations_stays_inside_the_bar(case, ridge, shapley):
    """validates the bar itself: what the device does, done by numpy, against the lstsq form"""
    n_img, K, T, d = case
    bits, wtab, y, delta = ref.fit_case(n_img, K, T, d, shapley, SAL.shapley_size_thresholds(d))
    for i in range(n_img):
        dl = None if delta is None else delta[i]
        phi_ref, icpt_ref = ref.fit(bits[i], wtab, y[i], d, ridge, dl)
        cond, bar = ref.fit_bar(bits[i], wtab, d, ridge, shapley, phi_ref)
        assert cond < 1e8, cond                                         # the precondition of every fit case
        phi, icpt = ref.fit_cholesky(bits[i], wtab, y[i], d, ridge, dl)
        ratio = float((np.abs(phi - phi_ref) / bar).max())
        print("cholesky vs lstsq", case, ridge, shapley, "cond", cond, "err / bar", ratio)
        assert ratio <= 1.0, (cond, ratio)
        assert np.abs(icpt - icpt_ref).max() <= bar.max()


@pytest.mark.parametrize("d", [2, 3, 5, 16, 33, 49, 128])
def test_shapley_size_thresholds(d):
    thr = SAL.shapley_size_thresholds(d)
    assert thr.dtype == np.uint32 and thr.shape == (d - 2,)
    t = thr.astype(np.int64)
    assert (np.diff(t) >= 0).all()
    for i, c in enumerate(ref.size_cumulative(d)):                      # within 1 of the exact C 2^32
        assert abs(int(t[i]) - c * 2 ** 32) <= 1, (i, int(t[i]), float(c * 2 ** 32))
    if d > 2:
        assert 0 < t[0] and t[-1] < 2 ** 32 - 1                         # sizes 1 and d - 1 both have room


@pytest.mark.parametrize("d", [2, 3, 5, 33, 128])
def test_shapley_draws_are_proper_subsets_in_antithetic_pairs(d):
    thr = SAL.shapley_size_thresholds(d)
    n = 24
    bits = ref.draws([7] * n, range(n), d, ref.SHAPLEY, thr=thr, seed=(3 << 32) + 5)
    z = ref.unpack(bits, d)
    size = z.sum(axis=1)
    assert (size >= 1).all() and (size <= d - 1).all()
    assert (z[1::2] == 1 - z[0::2]).all()
    assert not (bits & ~np.array(ref.pack(range(d), d), dtype=np.uint32)).any()       # nothing at or above d
    if d >= 5:
        assert len({tuple(r) for r in bits[0::2]}) > 1


def test_bernoulli_draws_follow_p():
    bits = ref.draws([1] * 64, range(64), 128, ref.BERNOULLI, 0.25, seed=9)
    frac = ref.unpack(bits, 128).mean()
    assert abs(frac - 0.25) < 0.02, frac
    assert ref.unpack(ref.draws([1], [0], 37, ref.BERNOULLI, 1.0, seed=9), 37).all()


def test_grid_segments_and_weight_tables():
    lab = SAL.grid_segments(32, 30, (3, 4))
    assert lab.shape == (32, 30) and lab.dtype == np.int32 and set(np.unique(lab)) == set(range(12))
    for i in range(3):                                                  # boundaries at floor(i H / cells)
        assert lab[i * 32 // 3, 0] == 4 * i and (i == 0 or lab[i * 32 // 3 - 1, 0] == 4 * (i - 1))
    assert np.array_equal(SAL.grid_segments(8, 8, 2), np.repeat(np.repeat([[0, 1], [2, 3]], 4, axis=0), 4, axis=1))
    assert np.array_equal(SAL.lime_weights(49, 0.25), ref.lime_weights(49, 0.25))
    w = SAL.lime_weights(16, 0.25)
    assert w[16] == 1.0 and w[0] == np.sqrt(np.exp(-16.0)) and (np.diff(w) > 0).all()


def test_refusals_before_an_engine_exists():
    L, S = SAL.LIMESaliency.check_arguments, SAL.KernelSHAPSaliency.check_arguments
    assert L(n_samples=10) == 49 and S(n_samples=None, cells=2) == 4 and S(n_samples=98, cells=7) == 49
    with pytest.raises(NotImplementedError):
        L(n_samples=10, cells=12)                                       # d = 144 > 128
    with pytest.raises(NotImplementedError):
        S(n_samples=400, cells=(12, 11))
    with pytest.raises(NotImplementedError):
        S(n_samples=None, cells=4)                                      # enumeration at d = 16 > 12
    with pytest.raises(NotImplementedError):
        L(n_samples=10, cells=1)                                        # d = 1
    for bad in (dict(n_samples=33, cells=4), dict(n_samples=30, cells=4), dict(n_samples=32.5, cells=4),
                dict(n_samples=32, cells=4, ridge=-1.0), dict(n_samples=32, cells=4, seed=-1),
                dict(n_samples=32, cells=4, seed=2 ** 64), dict(n_samples=32, cells=4, keys=[2 ** 32]),
                dict(n_samples=32, cells=4, score="p"), dict(n_samples=32, cells=4, fill=[1.0, 2.0])):
        with pytest.raises(ValueError):
            S(**bad)
    for bad in (dict(), dict(n_samples=0), dict(n_samples=10, p=0.0), dict(n_samples=10, p=1.5), dict(n_samples=10, kernel_width=0.0),
                dict(n_samples=10, kernel_width=float("nan")), dict(n_samples=10, ridge=-0.5), dict(n_samples=10, seed=0.5),
                dict(n_samples=10, keys=[-1]), dict(n_samples=10, score="x"), dict(n_samples=10, fill=float("inf"))):
        with pytest.raises(ValueError):
            L(**bad)


def test_operator_argument_checks_without_a_gpu():
    """Every argument is checked before any HIP call: these return without touching a device."""
    from lrp_imagecaptioning_amd import _capi
    lib = _capi.load()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    R, I = _capi.LRP_ERR_RANGE, _capi.LRP_ERR_INVALID
    draws = lambda d, mode=0, key=p, thr=p, prob=0.5: lib.lrp_op_segment_draws(key, p, 1, d, mode, prob, thr, 5, p, None)
    apply = lambda d, x=p: lib.lrp_op_segment_apply(x, p, p, p, p, p, 1, 1, 2, 2, 3, d, None)
    fit = lambda d, y=p, ridge=0.0: lib.lrp_op_segment_fit(p, p, y, None, ridge, p, p, p, 1, 4, 1, d, None)
    smap = lambda d, lab=p: lib.lrp_op_segment_map(p, lab, p, 1, 1, 2, 2, d, None)
    for fn in (draws, apply, fit, smap):
        assert fn(1) == R and b"outside [2,128]" in lib.lrp_last_error()
        assert fn(129) == R
    assert draws(5, mode=2) == I and draws(5, mode=-1) == I
    assert draws(5, key=None) == I and b"null" in lib.lrp_last_error()
    assert draws(5, mode=1, thr=None) == I                              # Shapley draws at d > 2 need their thresholds
    assert draws(5, prob=0.0) == I and draws(5, prob=1.5) == I and draws(5, prob=float("nan")) == I
    assert apply(5, x=None) == I and fit(5, y=None) == I and smap(5, lab=None) == I
    assert fit(5, ridge=-1.0) == I and fit(5, ridge=float("inf")) == I
    assert lib.lrp_op_segment_fit(p, p, p, None, 0.0, p, p, p, 1, 0, 1, 5, None) == I
    assert lib.lrp_op_segment_apply(p, p, p, p, p, p, 0, 1, 2, 2, 3, 5, None) == I
