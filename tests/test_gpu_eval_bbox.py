"""-m gpu: bounding-box correctness evaluation on the device (lrp_eval_*, evaluation.py) against the numpy restatement of
evaluate_bbox.py (tests/bbox_eval_ref.py)."""
import numpy as np
import pytest
import torch

import bbox_eval_ref as ref
from gpu_util import report
from lrp_imagecaptioning_amd import engine as E
from lrp_imagecaptioning_amd import evaluation as EV
from lrp_imagecaptioning_amd.synthetic import adaptive_weights, gridtd_weights, resnet_weights, vgg_weights

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _relevance_batch(rs, n, h, w, dtype):
    R = (rs.randn(n, h, w, 3) * rs.choice([1e-3, 1.0, 50.0], size=(n, 1, 1, 1))).astype(dtype)
    R[0] = 0                                                  # all zero -> zeros
    R[1] = 0
    R[1, 3, 5, 1] = -2.5                                      # a single non-zero
    R[2] = rs.randint(-2, 3, size=(h, w, 3))                  # ties
    R[3, :, :, :] = np.abs(R[3])                              # all positive: the -1 chain is all zero
    return R


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("sign", [-1, 1])
def test_relevance_maps_bitwise(dtype, sign):
    rs = np.random.RandomState(1)
    R = _relevance_batch(rs, 9, 224, 224, dtype)
    got = E.eval_relevance_maps(torch.as_tensor(R).to(DEV), sign).cpu().numpy()
    assert got.dtype == dtype
    for i in range(len(R)):
        want = ref.relevance_map(R[i:i + 1], sign)
        if want.dtype != dtype:                               # project() of an all-zero map: float64 zeros
            assert not want.any()
            want = want.astype(dtype)
        assert np.array_equal(got[i].view(np.uint8), want.view(np.uint8)), i


@pytest.mark.parametrize("g,up", [(14, 16), (7, 32)])
def test_attention_maps_match_restatement(g, up):
    rs = np.random.RandomState(g)
    att = rs.rand(5, g * g).astype(np.float32)
    att[1] /= att[1].sum()
    att[2] = 0
    att[3] -= 0.5                                             # negative values: the (x + 1) / 2 branch
    got = E.eval_attention_maps(torch.as_tensor(att).to(DEV), g, up).cpu().numpy()
    assert got.shape == (5, g * up, g * up) and got.dtype == np.float64
    for i in range(5):
        want = ref.attention_map(att[i], g, up)
        assert np.abs(got[i] - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300) or not want.any(), i
        if not want.any():
            assert not got[i].any()


def _literal_per_box(m, nbs, thresholds):
    m = np.array(m, copy=True)
    return np.array([[ref.overlap(nb, m, t) for t in thresholds] for nb in nbs])


def test_box_scores_match_restatement_and_are_deterministic():
    rs = np.random.RandomState(5)
    n, h, w = 320, 224, 224
    R = _relevance_batch(rs, n, h, w, np.float32)
    maps = E.eval_relevance_maps(torch.as_tensor(R).to(DEV), -1)
    mh = maps.cpu().numpy()
    entries, thr, nbs = [], [], []
    for m in range(n):
        k = rs.randint(1, 9)
        boxes = []
        for _ in range(k):
            x0, y0 = rs.randint(-30, 224), rs.randint(-30, 224)
            boxes.append([x0, y0, x0 + rs.randint(0, 260), y0 + rs.randint(0, 260)])
        nbs.append(boxes)
        entries += [(m,) + EV.normalise_box(b, (1.0, 1.0), h, w) for b in boxes]
        thr.append(EV.effective_thresholds(k))
    thr = np.concatenate(thr).astype(np.float32).astype(np.float64)
    got = E.eval_box_scores(maps, np.array(entries, dtype=np.int32), thr).cpu().numpy()
    want = ref.box_scores_f64(mh, entries, thr)
    err = np.abs(got - want).max()
    assert err <= 1e-9, err
    # the reference's own mixed float32 / float64 loop
    for m in range(0, n, 8):
        k = len(nbs[m])
        row = sum(len(b) for b in nbs[:m])
        lit_m = _literal_per_box(mh[m], nbs[m], ref.THRESHOLDS)
        assert np.abs(got[row:row + k] - lit_m).max() <= 1e-6
    again = E.eval_box_scores(maps, np.array(entries, dtype=np.int32), thr).cpu().numpy()
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))
    sel = [i for i, e in enumerate(entries) if e[0] == 17]
    alone = E.eval_box_scores(maps, np.array([entries[i] for i in sel], dtype=np.int32), thr[sel]).cpu().numpy()
    assert np.array_equal(alone.view(np.uint64), got[sel].view(np.uint64))
    report("eval_box_scores", max_abs_f64=err, entries=len(entries))


# ------------------------------------------------------------------------------------------ end to end
CFG = [("c1", 3, 16, False), ("c2", 16, 16, True), ("c3", 16, 32, False), ("c4", 32, 32, True), ("c5", 32, 64, False)]
WORDS = ["a", "man", "dog", "riding", "bike", "the", "hot", "table", "on", "women"]
EXT = {"person": ["man", "women"], "bicycle": ["bike"]}
FILT = ["a", "the"]


class _Datum(object):
    def __init__(self, f):
        self.img_filename = f


def _category(rs, hw, ncat=4):
    cats = {"person": 1, "bicycle": 2, "hot dog": 3, "dog": 4, "dining table": 5}
    bbox = {}
    for cid in cats.values():
        bbox[cid] = []
        for _ in range(rs.randint(1 if cid != 5 else 0, 4)):
            x0, y0 = rs.uniform(-10, 1.2 * hw), rs.uniform(-10, 1.2 * hw)
            bbox[cid].append([x0, y0, x0 + rs.uniform(0, 1.5 * hw), y0 + rs.uniform(0, 1.5 * hw)])
    return {"categories": cats, "bbox": bbox, "resize_ratio": (0.7, 1.3)}


def _explainer(cls_name, kind, V=40, H=32, max_images=1, cfg=CFG, hw=32, resnet=None, seed=0):
    import lrp_imagecaptioning_amd.explainers as EX
    rs = np.random.RandomState(seed)
    if resnet is None:
        w = vgg_weights(rs, cfg, bias_std=0.3)
        L, D = (hw // 2 ** sum(bool(c[3]) for c in cfg)) ** 2, cfg[-1][2]
    else:
        w = resnet_weights(rs, resnet["stacks"], stem=resnet["stem"], bias_std=0.2)
        L, D = (hw // 32) ** 2, resnet["stacks"][-1][0] * 4
    w.update((adaptive_weights if kind == "adaptive" else gridtd_weights)(rs, L, D, H, H, V))
    spec = EX.CaptionModelSpec(w, img_encoder="vgg16" if resnet is None else "resnet101", hidden_dim=H, embedding_dim=H, L=L,
                               D=D, vocab_size=V, cnn_cfg=cfg, img_hw=(hw, hw), resnet=resnet)
    word_of = {i: WORDS[i % len(WORDS)] for i in range(2, V + 1)}
    dp = EX.DatasetProviderStub(EX.CaptionPreprocessorStub(word_of=word_of))
    return getattr(EX, cls_name)(spec, None, dp, max_caption_length=8, max_images=max_images), rs


def _host_lrp(ex, ev, X, cap, category):
    """The per-word path: _explain_lstm_single_word_sequence + _explain_CNN + numpy scoring."""
    ex._forward_beam_search((None, X), cap)
    g, up = ev._reshape_size[0], ev._upscale

    def word(t):
        R, att = ex._explain_lstm_single_word_sequence(t)
        return [ref.relevance_map(ex._explain_CNN(X, R)), ref.attention_map(att, g, up)]
    return ref.evaluate_image(word, cap, ex._preprocessor._word_of, category, EXT, FILT, 2)


def _host_baseline(ex, X, cap, category):
    ex._forward_beam_search((None, X), cap)
    word = lambda t: [ref.relevance_map(np.asarray(ex._explain_CNN(X, ex._lstm_decoder_backward(t))))]
    return ref.evaluate_image(word, cap, ex._preprocessor._word_of, category, EXT, FILT, 1)


def _same(got, want, tol=1e-9):
    assert len(got) == len(want)
    worst = 0.0
    for g, w in zip(got[:-1], want[:-1]):
        assert list(g) == list(w) or set(g) == set(w)
        for cid in w:
            assert set(g[cid]) == set(w[cid]), cid
            for k in w[cid]:
                worst = max(worst, abs(g[cid][k] - w[cid][k]))
    assert got[-1] == want[-1]
    assert worst <= tol, worst
    return worst


CAPS = [[3, 4, 5, 6, 7, 8, 9, 1], [11, 12, 4, 14, 9, 1], [8, 9, 13, 1], [5, 6, 2, 4, 1]]


@pytest.mark.parametrize("kind,cls", [("adaptive", "ExplainImgCaptioningAdaptiveAttention"),
                                      ("gridtd", "ExplainImgCaptioningGridTDModel")])
def test_evaluate_batch_matches_per_word_path(kind, cls):
    ex, rs = _explainer(cls, kind, max_images=2)
    X = rs.uniform(-120, 130, size=(4, 32, 32, 3)).astype(np.float32)
    cats = {"img%d" % b: _category(rs, 32) for b in range(4)}
    ev = EV.EvaluationBboxCOCO(cats, 8, 3, "eps", "vgg16", ex, category_extension=EXT, word_filter=FILT)
    got = ev.evaluate_batch(X, list(cats), CAPS)
    worst = 0.0
    for b in range(4):
        worst = max(worst, _same(got[b], _host_lrp(ex, ev, X[b:b + 1], CAPS[b], cats["img%d" % b])))
    assert any(got[b][0] for b in range(4))
    report("eval_bbox_e2e", kind=kind, max_abs=worst)


def test_evaluate_batch_equals_evaluate_with_beam_search():
    ex, rs = _explainer("ExplainImgCaptioningAdaptiveAttention", "adaptive", max_images=6, seed=2)
    X = rs.uniform(-120, 130, size=(6, 32, 32, 3)).astype(np.float32)
    cats = {"img%d" % b: _category(rs, 32) for b in range(6)}
    ev = EV.EvaluationBboxCOCO(cats, 8, 3, "eps", "vgg16", ex, category_extension=EXT, word_filter=FILT)
    got = ev.evaluate_batch(X, list(cats))
    for b in range(6):
        one = ev.evaluate((None, X[b:b + 1]), [_Datum("img%d" % b)])
        assert one == got[b], b


@pytest.mark.parametrize("cls,batched", [("ExplainImgCaptioningAdaptiveAttentionGradient", True),
                                         ("ExplainImgCaptioningGridTDGradientTimesInput", True),
                                         ("ExplainImgCaptioningAdaptiveAttentionGuidedGradcam", False)])
def test_baseline_matches_host_path(cls, batched):
    kind = "gridtd" if "GridTD" in cls else "adaptive"
    ex, rs = _explainer(cls, kind, max_images=2, seed=4)
    assert ex._batched_cnn == batched
    X = rs.uniform(-120, 130, size=(3, 32, 32, 3)).astype(np.float32)
    cats = {"img%d" % b: _category(rs, 32) for b in range(3)}
    ev = EV.EvaluationBboxCOCOBaseline(cats, 8, 3, "eps", "vgg16", ex, category_extension=EXT, word_filter=FILT)
    got = ev.evaluate_batch(X, list(cats), CAPS[:3])
    for b in range(3):
        _same(got[b], _host_baseline(ex, X[b:b + 1], CAPS[b], cats["img%d" % b]))


def test_resnet_7x7_attention_matches_host_path():
    rn = {"stem": 8, "stacks": ((8, 1), (8, 1), (8, 1), (8, 1))}
    ex, rs = _explainer("ExplainImgCaptioningAdaptiveAttention", "adaptive", hw=224, resnet=rn, max_images=2, seed=6)
    X = rs.uniform(-120, 130, size=(2, 224, 224, 3)).astype(np.float32)
    cats = {"img%d" % b: _category(rs, 224) for b in range(2)}
    ev = EV.EvaluationBboxCOCO(cats, 8, 3, "eps", "resnet101", ex, category_extension=EXT, word_filter=FILT)
    assert ev._reshape_size == (7, 7) and ev._upscale == 32
    got = ev.evaluate_batch(X, list(cats), CAPS[:2])
    for b in range(2):
        _same(got[b], _host_lrp(ex, ev, X[b:b + 1], CAPS[b], cats["img%d" % b]))


def test_full_size_vgg16_adaptive_b8():
    from lrp_imagecaptioning_amd.synthetic import VGG16_CFG
    ex, rs = _explainer("ExplainImgCaptioningAdaptiveAttention", "adaptive", cfg=VGG16_CFG, hw=224, H=64, V=60,
                        max_images=8, seed=8)
    X = rs.uniform(-120, 130, size=(8, 224, 224, 3)).astype(np.float32)
    cats = {"img%d" % b: _category(rs, 224) for b in range(8)}
    caps = [CAPS[b % 4] for b in range(8)]
    ev = EV.EvaluationBboxCOCO(cats, 8, 3, "eps", "vgg16", ex, category_extension=EXT, word_filter=FILT)
    got = ev.evaluate_batch(X, list(cats), caps)
    worst = 0.0
    for b in (0, 5):
        worst = max(worst, _same(got[b], _host_lrp(ex, ev, X[b:b + 1], caps[b], cats["img%d" % b])))
    report("eval_bbox_vgg16_b8", max_abs=worst)
