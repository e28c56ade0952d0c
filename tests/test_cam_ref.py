"""CPU checks of the CAM family: known answers of the numpy restatement (tests/cam_ref.py), the C boundary (symbols and refusals,
which launch nothing) and the argument errors of the Python wrappers, the drivers and the classes (no GPU needed)."""
import ctypes

import numpy as np
import pytest
import torch

import cam_ref as ref
from lrp_imagecaptioning_amd import _capi
from lrp_imagecaptioning_amd import engine as E
from lrp_imagecaptioning_amd import saliency as SAL

NAMES = ("lrp_op_cam", "lrp_op_cam_weighted", "lrp_op_scorecam_apply", "lrp_op_feature_ablate")


# ---------------------------------------------------------------------------------------------------- known answers
def test_one_live_channel_reduces_every_form_to_that_channels_map():
    """L = 4, D = 8, channel 5 alone carries features and a positive gradient: every coarse map is a positive multiple of the
    channel's map, so every cam is the channel's own normalised expansion"""
    g, up, live = 2, 3, 5
    F, G = np.zeros((4, 8)), np.zeros((4, 8))
    F[:, live] = [0.5, 2.0, 0.0, 1.25]
    G[:, live] = [0.25, 0.5, 0.125, 1.0]
    want = {"gradcam": F[:, live] * G[:, live].mean(),
            "gradcam++": F[:, live] * (G[:, live] / (2.0 + F[:, live].sum() * G[:, live])).sum(),
            "xgradcam": F[:, live] * (F[:, live] * G[:, live]).sum() / (F[:, live].sum() + 1e-7),
            "layercam": F[:, live] * G[:, live], "hirescam": F[:, live] * G[:, live]}
    M = ref.expand_matrix(g, up)
    for mode in ref.MODES:
        A, Aa = ref.coarse(F, G, mode)
        assert np.allclose(A, want[mode], rtol=1e-14, atol=0) and np.array_equal(A, Aa), mode
        cam, _ = ref.cam(F, G, mode, g, up)
        e = M @ want[mode].reshape(g, g) @ M.T
        assert np.allclose(cam, e / (e.max() + 1e-6), rtol=1e-13, atol=0), mode
    # the three forms with channel weights give the SAME cam up to the 1e-6 of the normalisation: the channel's own expansion
    e = M @ F[:, live].reshape(g, g) @ M.T
    for mode in ("gradcam", "gradcam++", "xgradcam"):
        cam, _ = ref.cam(F, G, mode, g, up)
        assert np.abs(cam - e / e.max()).max() < 1e-4, mode


def test_hirescam_equals_gradcam_when_the_gradient_is_constant_over_positions():
    rs = np.random.RandomState(0)
    F = np.maximum(rs.randn(9, 24), 0)
    G = np.repeat(rs.randn(1, 24), 9, axis=0)
    a, _ = ref.coarse(F, G, "hirescam")
    b, _ = ref.coarse(F, G, "gradcam")
    assert np.allclose(a, b, rtol=1e-13, atol=1e-15)


def test_layercam_equals_hirescam_when_the_gradient_is_nonnegative():
    rs = np.random.RandomState(1)
    F, G = np.maximum(rs.randn(9, 24), 0), np.abs(rs.randn(9, 24))
    assert np.array_equal(ref.coarse(F, G, "layercam")[0], ref.coarse(F, G, "hirescam")[0])
    cam, _ = ref.cam(F, -G, "layercam", 3, 4)
    assert not cam.any()                                                # nowhere positive: exact zeros


def test_weightings_known_answers():
    s = np.array([0.0, np.log(3.0)])
    w, _ = ref.weights(1.0, s, 0.0, "softmax")
    assert np.allclose(w, [0.25, 0.75], rtol=1e-15)
    q = np.array([0.0, 1.5, -0.25])                                     # multiples of 2^-2: the shift by 1000 is exact
    assert np.array_equal(ref.weights(1.0, q + 1000.0, 0.0, "softmax")[0], ref.weights(1.0, q, 0.0, "softmax")[0])
    assert np.array_equal(ref.weights(9.0, np.array([1.0, 4.0]), 0.5, "linear")[0], [0.5, 3.5])
    assert np.array_equal(ref.weights(-2.0, np.array([1.0, -4.0]), 0.0, "ablation")[0], [-1.5, 1.0])
    assert not ref.weights(0.0, np.array([1.0, -4.0]), 0.0, "ablation")[0].any()


def test_mask_of_a_constant_channel_is_zeros_and_the_range_is_the_unit_interval():
    assert not ref.scorecam_mask(np.full(9, 3.25, dtype=np.float32), 3, 4).any()
    rs = np.random.RandomState(2)
    for g, up in ((2, 3), (3, 4), (7, 5), (14, 2)):
        m = ref.scorecam_mask(rs.randn(g * g).astype(np.float32), g, up)
        assert m.shape == (g * up, g * up) and m.dtype == np.float32
        assert m.min() >= 0.0 and m.max() <= 1.0
        if up % 2 == 1:                                                 # an odd cell has a pixel on the node: both ends are reached
            assert m.min() == 0.0 and m.max() == 1.0
    # the node values themselves: at the centre pixel of a cell of odd side the mask IS the normalised value
    v = np.array([1.0, 3.0, 2.0, 5.0], dtype=np.float32)
    m = ref.scorecam_mask(v, 2, 3)
    assert np.array_equal(m[1::3, 1::3].reshape(-1), (v - 1.0) / 4.0)
    # an even cell never samples a node of the interior, but the clamped border does: the corners hold the corner cells
    m = ref.scorecam_mask(v, 2, 2)
    assert m[0, 0] == 0.0 and m[3, 3] == 1.0


def test_apply_and_ablate_special_rows():
    rs = np.random.RandomState(3)
    x = rs.uniform(-120, 130, size=(2, 6, 6, 3)).astype(np.float32)
    feat = np.maximum(rs.randn(2, 4, 8), 0).astype(np.float32)
    feat[1, :, 2] = 0.0                                                 # a dead channel
    fill = [-3.5, 10.25, 0.0]
    out = ref.scorecam_apply(x, feat, [0, 1, 1, 2, 0], [-1, 8, 2, 0, 9], 2, 3, fill)
    assert np.array_equal(out[0], x[0])
    assert (out[1] == np.asarray(fill, dtype=np.float32)).all() and np.array_equal(out[2], out[1])
    assert np.isnan(out[3]).all() and np.isnan(out[4]).all()
    ab = ref.feature_ablate(feat, [0, 1, 0, 1], [-1, 3, 8, -2])
    assert np.array_equal(ab[0], feat[0]) and not ab[1][:, 3].any() and np.array_equal(np.delete(ab[1], 3, 1), np.delete(feat[1], 3, 1))
    assert np.isnan(ab[2]).all() and np.isnan(ab[3]).all()


# ---------------------------------------------------------------------------------------------------- the C boundary
def test_symbols_are_bound():
    lib = _capi.load()
    for n in NAMES:
        assert n in _capi.SYMBOLS and hasattr(lib, n)
    assert E.CAM_MODES == {m: i for i, m in enumerate(ref.MODES)}
    assert E.CAM_WEIGHTS == {m: i for i, m in enumerate(ref.WEIGHTS)}


def test_entries_refuse_bad_arguments_before_any_hip_call():
    """Every refusal below returns before a launch: the pointers are host memory that is never read"""
    lib = _capi.load()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    bad = _capi.LRP_ERR_INVALID
    # lrp_op_cam(feat, idx, grads, M, gb, cam, out, n, B, g, upscale, D, C, mode, stream)
    assert lib.lrp_op_cam(None, p, p, p, None, p, None, 1, 1, 2, 3, 8, 0, 0, None) == bad
    assert lib.lrp_op_cam(p, p, p, p, p, p, None, 1, 1, 2, 3, 8, 3, 0, None) == bad          # gate without its output
    assert lib.lrp_op_cam(p, p, p, p, None, p, None, 0, 1, 2, 3, 8, 0, 0, None) == bad
    assert lib.lrp_op_cam(p, p, p, p, None, p, None, 1, 1, 17, 1, 8, 0, 0, None) == bad       # g > 16
    assert lib.lrp_op_cam(p, p, p, p, None, p, None, 1, 1, 16, 29, 8, 0, 0, None) == bad      # S = 464
    assert lib.lrp_op_cam(p, p, p, p, None, p, None, 1, 1, 2, 3, 12, 0, 0, None) == bad       # D % 8
    assert lib.lrp_op_cam(p, p, p, p, None, p, None, 1, 1, 2, 3, 4104, 0, 0, None) == bad
    assert lib.lrp_op_cam(p, p, p, p, None, p, None, 1, 1, 2, 3, 8, 0, 5, None) == bad        # mode
    assert lib.lrp_op_cam(p, p, p, p, None, p, None, 1, 1, 2, 3, 8, 0, -1, None) == bad
    assert lib.lrp_op_cam(p, p, p, p, p, p, p, 1, 1, 2, 3, 8, 65, 0, None) == bad             # C
    assert lib.lrp_op_cam(p, p, p, p, None, p, None, 1, 1, 2, 3, 8, 0, 7, None) == bad and b"mode" in lib.lrp_last_error()
    # lrp_op_cam_weighted(scores, feat, idx, M, cam, map, n_img, R, T, B, g, upscale, D, mode, stream)
    assert lib.lrp_op_cam_weighted(p, p, p, p, None, None, 1, 9, 1, 1, 2, 3, 8, 0, None) == bad   # no output
    assert lib.lrp_op_cam_weighted(None, p, p, p, p, None, 1, 9, 1, 1, 2, 3, 8, 0, None) == bad
    assert lib.lrp_op_cam_weighted(p, p, p, p, p, None, 1, 9, 1, 1, 2, 3, 8, 1, None) == bad      # linear needs R = 10
    assert lib.lrp_op_cam_weighted(p, p, p, p, p, None, 1, 10, 1, 1, 2, 3, 8, 0, None) == bad
    assert lib.lrp_op_cam_weighted(p, p, p, p, p, None, 1, 9, 0, 1, 2, 3, 8, 0, None) == bad
    assert lib.lrp_op_cam_weighted(p, p, p, p, p, None, 1, 9, 1, 1, 2, 3, 8, 3, None) == bad      # mode
    assert lib.lrp_op_cam_weighted(p, p, p, p, p, None, 1, 13, 1, 1, 2, 3, 12, 0, None) == bad    # D % 8
    # lrp_op_scorecam_apply(x, feat, idx, k, fill, out, n, B, g, upscale, C, D, stream)
    assert lib.lrp_op_scorecam_apply(p, p, p, p, None, p, 1, 1, 2, 3, 3, 8, None) == bad
    assert lib.lrp_op_scorecam_apply(p, p, p, p, p, p, 0, 1, 2, 3, 3, 8, None) == bad
    assert lib.lrp_op_scorecam_apply(p, p, p, p, p, p, 65536, 1, 2, 3, 3, 8, None) == bad
    assert lib.lrp_op_scorecam_apply(p, p, p, p, p, p, 1, 1, 17, 3, 3, 8, None) == bad
    assert lib.lrp_op_scorecam_apply(p, p, p, p, p, p, 1, 1, 2, 0, 3, 8, None) == bad
    assert lib.lrp_op_scorecam_apply(p, p, p, p, p, p, 1, 1, 2, 3, 0, 8, None) == bad
    assert lib.lrp_op_scorecam_apply(p, p, p, p, p, p, 1, 1, 2, 3, 3, 0, None) == bad
    # lrp_op_feature_ablate(feat, idx, k, out, n, B, L, D, stream)
    assert lib.lrp_op_feature_ablate(p, p, None, p, 1, 1, 4, 8, None) == bad
    assert lib.lrp_op_feature_ablate(p, p, p, p, 0, 1, 4, 8, None) == bad
    assert lib.lrp_op_feature_ablate(p, p, p, p, 1, 1, 0, 8, None) == bad
    assert lib.lrp_op_feature_ablate(p, p, p, p, 1, 1, 1 << 16, 1 << 16, None) == bad


# ---------------------------------------------------------------------------------------------------- the Python wrappers
def test_wrappers_refuse_bad_arguments_before_any_gpu_call():
    """CPU tensors throughout: a refusal that came after a launch (or after an upload) could not be reached here"""
    f8, d8 = torch.zeros((2, 4, 8)), torch.zeros((3, 4, 8))
    with pytest.raises(ValueError, match="unknown CAM method"):
        E.op_cam(f8, [0, 1, 1], d8, 2, 3, method="eigencam")
    with pytest.raises(ValueError, match="multiple of 8"):
        E.op_cam(torch.zeros((2, 4, 12)), [0, 1, 1], torch.zeros((3, 4, 12)), 2, 3)
    with pytest.raises(ValueError):
        E.op_cam(f8, [0, 1, 1], d8, 17, 1)
    with pytest.raises(ValueError, match="unknown weighting"):
        E.op_cam_weighted(torch.zeros((1, 9, 2), dtype=torch.float64), f8, [0], 2, 3, weights="sigmoid")
    with pytest.raises(ValueError, match="multiple of 8"):
        E.op_cam_weighted(torch.zeros((1, 13, 2), dtype=torch.float64), torch.zeros((2, 4, 12)), [0], 2, 3)
    with pytest.raises(ValueError):
        E.op_scorecam_apply(torch.zeros((2, 6, 9, 3)), f8, [0], [0], 2, 3)                    # not a device tensor, not square
    with pytest.raises(ValueError):
        E.op_feature_ablate(np.zeros((2, 4, 8), dtype=np.float32), [0], [0])
    # the geometry every driver checks before it touches the engine
    assert E.cam_geometry(196, 224, 224) == (14, 16) and E.cam_geometry(49, 224, 224) == (7, 32) and E.cam_geometry(64, 32, 32) == (8, 4)
    with pytest.raises(ValueError, match="square"):
        E.cam_geometry(196, 224, 256)                                                         # a non-square image
    with pytest.raises(ValueError, match="square"):
        E.cam_geometry(196, 220, 220)                                                         # a side that is no multiple of 14
    with pytest.raises(ValueError, match="square"):
        E.cam_geometry(200, 224, 224)                                                         # L is no square
    with pytest.raises(NotImplementedError):
        E.cam_geometry(17 * 17, 17 * 8, 17 * 8)


def test_drivers_and_classes_refuse_bad_arguments():
    with pytest.raises(ValueError, match="unknown CAM method"):
        SAL.GradientCAMSaliency.check_arguments(method="eigencam")
    with pytest.raises(ValueError):
        SAL.GradientCAMSaliency.check_arguments(guided="yes")
    with pytest.raises(ValueError):
        SAL.ScoreCAMSaliency.check_arguments(weights="ablation")
    with pytest.raises(ValueError):
        SAL.ScoreCAMSaliency.check_arguments(score="probability")
    with pytest.raises(ValueError):
        SAL.ScoreCAMSaliency.check_arguments(fill=[0.0, 1.0])
    with pytest.raises(ValueError):
        SAL.AblationCAMSaliency.check_arguments(score="p")
    for m in ref.MODES:
        SAL.GradientCAMSaliency.check_arguments(method=m, guided=True)
    assert SAL.CAM_METHODS == ref.MODES
    # the classes check their keywords before an engine is created (none can be, here)
    import lrp_imagecaptioning_amd.explainers as EX
    for name, kw in (("ExplainImgCaptioningAdaptiveAttentionCAM", {"method": "cam"}), ("ExplainImgCaptioningGridTDCAM", {"guided": 2}),
                     ("ExplainImgCaptioningAdaptiveAttentionScoreCAM", {"weights": "hard"}),
                     ("ExplainImgCaptioningGridTDScoreCAM", {"score": "x"}),
                     ("ExplainImgCaptioningAdaptiveAttentionAblationCAM", {"score": "x"}),
                     ("ExplainImgCaptioningGridTDAblationCAM", {"score": "x"})):
        with pytest.raises(ValueError):
            getattr(EX, name)(None, None, None, **kw)
    from lrp_imagecaptioning_amd.analyzer import analyzers
    assert not [k for k in analyzers if "cam" in str(k).lower() and "guided" not in str(k).lower()]
