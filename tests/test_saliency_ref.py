"""CPU checks of the occlusion / RISE saliency: known answers of the numpy restatement (tests/saliency_ref.py), the mean of the
drawn masks, the C boundary (symbols and refusals, which launch nothing) and the argument errors of the driver and the classes (no GPU
needed)."""
import ctypes

import numpy as np
import pytest

import saliency_ref as ref
from lrp_imagecaptioning_amd import _capi
from lrp_imagecaptioning_amd import engine as E
from lrp_imagecaptioning_amd import saliency as SAL

NAMES = ("lrp_op_occlude", "lrp_op_occlusion_map", "lrp_op_rise_grids", "lrp_op_rise_apply", "lrp_op_rise_map")


# ---------------------------------------------------------------------------------------------------- known answers
def test_geometry_clips_the_last_window_and_covers_every_pixel():
    assert ref.geometry(20, 29, (5, 7), (3, 4)) == (6, 7) == E.occlusion_geometry(20, 29, (5, 7), (3, 4))
    assert ref.window_box(6 * 7 - 1, 20, 29, (5, 7), (3, 4)) == (15, 20, 24, 29)          # rows fit exactly, columns are clipped
    assert ref.geometry(16, 16, 4) == (4, 4) == E.occlusion_geometry(16, 16, 4)
    assert ref.geometry(16, 16, 16) == (1, 1)
    for H, W, win, st in ((20, 29, (5, 7), (3, 4)), (16, 16, (4, 4), None), (7, 9, (3, 2), (2, 1)), (32, 32, (12, 12), (8, 8))):
        assert ref.coverage(H, W, win, st).min() >= 1
    assert (ref.coverage(16, 16, 4) == 1).all()                                           # window == stride: c = 1


def test_one_window_with_difference_one_gives_its_indicator_over_c():
    H, W, win, st = 20, 29, (5, 7), (3, 4)
    Hn, Wn = ref.geometry(H, W, win, st)
    c = ref.coverage(H, W, win, st)
    for k in (0, 9, Hn * Wn - 1):
        s = np.full((1, 1 + Hn * Wn, 2), 0.75)
        s[0, 1 + k, 1] -= 1.0                                                             # s_0 - s_{1+k} = 1 for word 1 only
        S, _ = ref.occlusion_map(s, H, W, win, st)
        y0, y1, x0, x1 = ref.window_box(k, H, W, win, st)
        ind = np.zeros((H, W))
        ind[y0:y1, x0:x1] = 1.0
        assert np.array_equal(S[0, 1], ind / c) and not S[0, 0].any()


def test_a_window_covering_the_image_is_one_window():
    s = np.array([[[0.9, 0.5], [0.25, 0.75]]])                                            # (1, 2, T = 2)
    S, _ = ref.occlusion_map(s, 16, 16, 16)
    assert np.array_equal(S[0, 0], np.full((16, 16), 0.9 - 0.25)) and np.array_equal(S[0, 1], np.full((16, 16), 0.5 - 0.75))
    x = np.random.RandomState(0).randn(1, 16, 16, 3).astype(np.float32)
    assert np.array_equal(ref.occlude(x, [0], [0], 16, fill=[1, 2, 3])[0], np.broadcast_to(np.float32([1, 2, 3]), (16, 16, 3)))
    assert np.array_equal(ref.occlude(x, [0], [-1], 16)[0], x[0])


def test_rise_known_answers():
    H, W, s = 20, 29, 3
    cell = ref.rise_cell(H, W, s)
    assert cell == (7, 10) == E.rise_cell(H, W, s)
    grid, shift = ref.rise_grids([5] * 6, range(6), s, 1.0, 11, cell)
    assert grid.all() and (shift[:, 0] < 7).all() and (shift[:, 1] < 10).all() and (shift >= 0).all()
    m = ref.rise_masks(grid, shift, H, W, s, cell)
    assert np.array_equal(m, np.ones_like(m))                                             # p = 1: m = 1
    grid, shift = ref.rise_grids([5] * 6, range(6), s, 0.5, 11, cell)
    m = ref.rise_masks(grid, shift, H, W, s, cell)
    assert m.min() >= 0.0 and m.max() <= 1.0 and 0 < grid.sum() < grid.size
    v = 0.375
    S, A = ref.rise_map(np.full((1, 6, 2), v), grid[None], shift[None], H, W, s, 0.5, cell)
    assert np.abs(S[0, 0] - v * m.sum(axis=0) / (6 * 0.5)).max() <= 1e-15 and np.array_equal(S, A)
    # the draw depends on (seed, key, k) alone
    g2, s2 = ref.rise_grids([9, 5, 5], [0, 3, 4], s, 0.5, 11, cell)
    assert np.array_equal(g2[1:], grid[3:5]) and np.array_equal(s2[1:], shift[3:5]) and not np.array_equal(g2[0], grid[0])
    assert not np.array_equal(ref.rise_grids([5], [3], s, 0.5, 12, cell)[0], grid[3:4])


def test_mask_formula_is_the_half_pixel_upsample():
    # a 2 x 2 grid (s = 1) of cell 4, no shift: pixel centres (y + 0.5) / 4 - 0.5 in grid units, clamped at the border
    G = np.array([[0, 1, 1, 0]], dtype=np.uint8)
    m = ref.rise_masks(G, [[0, 0]], 4, 4, 1, (4, 4))[0]
    f = np.clip((np.arange(4) + 0.5) / 4 - 0.5, 0, 1)
    want = (1 - f)[:, None] * ((1 - f)[None, :] * 0 + f[None, :] * 1) + f[:, None] * ((1 - f)[None, :] * 1 + f[None, :] * 0)
    assert np.abs(m - want).max() <= 1e-15


@pytest.mark.parametrize("p", [0.25, 0.5])
def test_mask_mean_is_p_within_four_standard_errors(p):
    """Given its shift a mask's mean over the image is sum_e w_e G_e with sum_e w_e = 1 (bilinear weights), so its expectation is p
    and its variance p (1 - p) sum_e w_e^2; the masks are independent.  The weights come from the restatement by linearity."""
    H = W = 16
    s, n = 4, 512
    cell = ref.rise_cell(H, W, s)
    grid, shift = ref.rise_grids([3] * n, range(n), s, p, 2024, cell)
    mean = ref.rise_masks(grid, shift, H, W, s, cell).mean()
    eye = np.eye((s + 1) ** 2, dtype=np.uint8)
    w2 = {}
    for dy, dx in {(int(a), int(b)) for a, b in shift}:
        w = ref.rise_masks(eye, [[dy, dx]] * len(eye), H, W, s, cell).mean(axis=(1, 2))
        assert abs(w.sum() - 1.0) <= 1e-12
        w2[(dy, dx)] = (w ** 2).sum()
    se = np.sqrt(p * (1 - p) * sum(w2[(int(a), int(b))] for a, b in shift)) / n
    assert abs(mean - p) <= 4 * se, (mean, p, se)
    assert abs(grid.mean() - p) <= 4 * np.sqrt(p * (1 - p) / grid.size)


# ---------------------------------------------------------------------------------------------------- the boundary
def test_library_exports_the_five_entries():
    lib = _capi.load()
    for name in NAMES:
        assert name in _capi.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(_capi.SYMBOLS[name][1])
    assert lib.lrp_abi_version() == _capi.LRP_ABI_VERSION == 10                           # additive: no version bump


def test_c_entries_refuse_before_any_device_work():
    lib = _capi.load()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    INV, RNG = _capi.LRP_ERR_INVALID, _capi.LRP_ERR_RANGE

    def refused(rc, code):
        assert rc == code and len(lib.lrp_last_error()) > 0

    occ = lambda H, W, ph, pw, sh, sw: lib.lrp_op_occlude(p, p, p, p, p, 1, 1, H, W, 3, ph, pw, sh, sw, None)
    omap = lambda H, W, ph, pw, sh, sw: lib.lrp_op_occlusion_map(p, p, 1, 1, H, W, ph, pw, sh, sw, None)
    for f in (occ, omap):
        refused(f(16, 16, 4, 4, 5, 4), INV)                                               # sh > ph
        refused(f(16, 16, 17, 4, 4, 4), INV)                                              # ph > H
        refused(f(16, 16, 4, 4, 4, 0), INV)                                               # sw < 1
        refused(f(16, 16, 4, 17, 4, 4), INV)                                              # pw > W
        refused(f(300, 300, 2, 2, 1, 1), RNG)                                             # 299 * 299 > 65536 windows
    refused(lib.lrp_op_occlude(None, p, p, p, p, 1, 1, 16, 16, 3, 4, 4, 4, 4, None), INV)
    refused(lib.lrp_op_occlude(p, p, p, p, p, 0, 1, 16, 16, 3, 4, 4, 4, 4, None), INV)
    grids = lambda s, pp, ch, cw: lib.lrp_op_rise_grids(p, p, 1, s, pp, 0, 16, 16, ch, cw, p, p, None)
    apply_ = lambda s, ch, cw: lib.lrp_op_rise_apply(p, p, p, p, p, p, 1, 1, 16, 16, 3, s, ch, cw, None)
    rmap = lambda s, pp, ch, cw: lib.lrp_op_rise_map(p, p, p, p, 1, 4, 1, 16, 16, s, pp, ch, cw, None)
    for s in (0, 64):
        refused(grids(s, 0.5, 16, 16), RNG)
        refused(apply_(s, 16, 16), RNG)
        refused(rmap(s, 0.5, 16, 16), RNG)
    for pp in (0.0, 1.5, -0.25, float("nan")):
        refused(grids(4, pp, 4, 4), INV)
        refused(rmap(4, pp, 4, 4), INV)
    for ch, cw in ((3, 4), (4, 3)):                                                       # below ceil(16 / 4)
        refused(grids(4, 0.5, ch, cw), INV)
        refused(apply_(4, ch, cw), INV)
        refused(rmap(4, 0.5, ch, cw), INV)
    refused(grids(5, 0.5, 3, 4), INV)                                                     # ceil(16 / 5) = 4
    refused(lib.lrp_op_rise_grids(p, p, 0, 4, 0.5, 0, 16, 16, 4, 4, p, p, None), INV)
    refused(lib.lrp_op_rise_map(p, p, p, None, 1, 4, 1, 16, 16, 4, 0.5, 4, 4, None), INV)


# ---------------------------------------------------------------------------------------------------- the driver and the classes
def test_driver_argument_errors():
    with pytest.raises(ValueError):
        SAL.OcclusionSaliency(None, (4, 4), stride=(5, 4))
    with pytest.raises(ValueError):
        SAL.OcclusionSaliency(None, (0, 4))
    with pytest.raises(ValueError):
        SAL.OcclusionSaliency(None, (4, 4, 4))
    with pytest.raises(ValueError):
        SAL.OcclusionSaliency(None, 4, score="probability")
    with pytest.raises(ValueError):
        SAL.OcclusionSaliency(None, 4, fill=[0.0, 1.0])
    with pytest.raises(ValueError):
        SAL.RISESaliency(None, 0)
    with pytest.raises(ValueError):
        SAL.RISESaliency(None, 2.5)
    for s in (0, 64):
        with pytest.raises(NotImplementedError):
            SAL.RISESaliency(None, 8, s=s)
    for p in (0.0, 1.0001):
        with pytest.raises(ValueError):
            SAL.RISESaliency(None, 8, p=p)
    with pytest.raises(ValueError):
        SAL.RISESaliency(None, 8, seed=-1)
    with pytest.raises(ValueError):
        SAL.RISESaliency(None, 8, keys=[0, 2 ** 32])
    with pytest.raises(ValueError):
        SAL.RISESaliency(None, 8, score="p")
    with pytest.raises(ValueError):
        E.occlusion_geometry(16, 16, (17, 4))
    with pytest.raises(NotImplementedError):
        E.occlusion_geometry(300, 300, 2, 1)


def test_class_argument_errors_come_before_an_engine_is_made():
    import lrp_imagecaptioning_amd.explainers as EX
    from lrp_imagecaptioning_amd import analyzer as A
    with pytest.raises(ValueError):
        EX.ExplainImgCaptioningAdaptiveAttentionOcclusion(None, stride=3)                  # no window
    with pytest.raises(ValueError):
        EX.ExplainImgCaptioningGridTDOcclusion(None, window=4, stride=5)
    with pytest.raises(ValueError):
        EX.ExplainImgCaptioningAdaptiveAttentionRISE(None)                                # no n_masks
    with pytest.raises(NotImplementedError):
        EX.ExplainImgCaptioningGridTDRISE(None, n_masks=8, s=64)
    with pytest.raises(ValueError):
        EX.ExplainImgCaptioningGridTDRISE(None, n_masks=8, p=0)
    for cls in ("AdaptiveAttentionOcclusion", "AdaptiveAttentionRISE", "GridTDOcclusion", "GridTDRISE"):
        assert issubclass(getattr(EX, "ExplainImgCaptioning" + cls), EX._SaliencyMixin)
    assert not any("occlusion" in k.lower() or "rise" in k.lower() for k in A.analyzers)   # the dict mirrors the reference's keys
