"""CPU checks of the bounding-box evaluation (evaluate_bbox.py): the host planning of lrp_eval_box_scores (threshold
carry-over, box normalisation, word -> category matching), the pyramid_expand matrix, the aggregation table and the
argument checks of the lrp_eval_* entry points (no GPU needed)."""
import ctypes

import numpy as np
import pytest

import bbox_eval_ref as ref
from lrp_imagecaptioning_amd import evaluation as EV


def _literal_scores(m, boxes, ratio, thresholds):
    """The reference loop of one word, recording every (box, threshold) score."""
    m = np.array(m, copy=True)
    out = []
    for box in boxes:
        nb = [int(box[0] * ratio[0]), int(box[1] * ratio[1]), int(box[2] * ratio[0]), int(box[3] * ratio[1])]
        out.append([ref.overlap(nb, m, thr) for thr in thresholds])
    return np.array(out, dtype=np.float64)


def _random_boxes(rs, n, h, w):
    kinds = [lambda: [0, 0, w, h], lambda: [5, 5, 5, 9], lambda: [w - 3, h - 4, w + 40, h + 9],
             lambda: [-30, -20, 10, 12], lambda: [-5, 3, -1, 40]]
    out = []
    for _ in range(n):
        if rs.rand() < 0.4:
            out.append(kinds[rs.randint(len(kinds))]())
        else:
            x0, y0 = rs.randint(0, w), rs.randint(0, h)
            out.append([x0, y0, x0 + rs.randint(1, w), y0 + rs.randint(1, h)])
    return out


@pytest.mark.parametrize("mode", ["reference", "independent"])
def test_effective_thresholds_reproduce_in_place_loop(mode):
    rs = np.random.RandomState(7)
    h, w = 40, 48
    ratio = (0.9, 1.1)
    for trial in range(30):
        m = rs.rand(h, w).astype(np.float32) * (rs.rand(h, w) < 0.7)
        m = ref.project(m) if trial % 3 else ref.relevance_map(rs.randn(1, h, w, 3).astype(np.float32))
        boxes = _random_boxes(rs, rs.randint(1, 6), h, w)
        if mode == "reference":
            want = _literal_scores(m, boxes, ratio, ref.THRESHOLDS)
        else:
            want = np.array([[_literal_scores(m, [b], ratio, [t])[0, 0] for t in ref.THRESHOLDS] for b in boxes])
        thr = EV.effective_thresholds(len(boxes), ref.THRESHOLDS, mode)
        if m.dtype == np.float32:
            thr = thr.astype(np.float32).astype(np.float64)
        entries = [(0,) + EV.normalise_box(b, ratio, h, w) for b in boxes]
        got = ref.box_scores_f64([m], entries, thr)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
    t = EV.effective_thresholds(3)
    assert (t[0] == ref.THRESHOLDS).all() and (t[1:] == 0.9).all()


def test_box_normalisation_follows_slice_semantics():
    rs = np.random.RandomState(3)
    h, w = 30, 20
    for _ in range(500):
        box = list(rs.uniform(-50, 60, size=4))
        ratio = tuple(rs.uniform(0.2, 2.0, size=2))
        nb = [int(box[i] * ratio[i % 2]) for i in range(4)]
        a = np.zeros((h, w))
        a[nb[1]:nb[3], nb[0]:nb[2]] = 1
        y0, y1, x0, x1 = EV.normalise_box(box, ratio, h, w)
        assert 0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w
        b = np.zeros((h, w))
        b[y0:y1, x0:x1] = 1
        assert (a == b).all(), (nb, (y0, y1, x0, x1))


def test_word_category_matching():
    word_of = {3: "a", 4: "man", 5: "riding", 6: "bike", 7: "hot", 8: "dog", 9: "the", 10: "women", 11: "table", 1: "<e>"}
    cats = {"person": 1, "bicycle": 2, "hot dog": 3, "dog": 4, "dining table": 5, "a": 6}
    ext = {"person": ["man", "women", "person"], "bicycle": ["bike", "bicycle"]}
    filt = ["a", "the"]
    caps = [[3, 4, 5, 3, 6, 1], [9, 10, 11, 7, 8, 8, 1], [3, 9, 1], [4, 6, 4, 1]]
    for cap in caps:
        words, key_of = EV.match_categories(cap, word_of, cats, ext, filt)
        rwords, rkey = ref.match(cap, word_of, cats, ext, filt)
        assert {k: set(v) for k, v in words.items()} == rwords
        assert key_of == rkey
        assert list(words) == list(rwords)                                  # same category order
    words, _ = EV.match_categories(caps[1], word_of, cats, ext, filt)
    assert words[3] == [(4, "hot"), (5, "dog"), (6, "dog")] and words[4] == [(5, "dog"), (6, "dog")]
    assert 6 not in words                                                   # the filtered word never matches
    assert EV.match_categories(caps[0], word_of, cats, None, filt)[0] == {}   # no synonyms: 'man' / 'bike' are not names


@pytest.mark.parametrize("g,up", [(14, 16), (7, 32)])
def test_expand_matrix_matches_pyramid_expand(g, up):
    from lrp_imagecaptioning_amd.engine import eval_expand_matrix
    from lrp_imagecaptioning_amd.postprocess import pyramid_expand
    M = eval_expand_matrix(g, up, 20.0)
    assert M.shape == (g * up, g)
    rs = np.random.RandomState(g)
    for A in (rs.rand(g, g), rs.randn(g, g), np.eye(g)):
        want = pyramid_expand(A, upscale=up, sigma=20)
        got = M @ A @ M.T
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_correctness_table_hand_computed():
    thr = (0, 0.5)
    store = {}
    EV.accumulate(store, {1: {"0": 0.5, "0.5": 0.25}, 2: {"0": 1.0, "0.5": 0}}, {1: "person", 2: "dog"}, thr)
    EV.accumulate(store, {1: {"0": 0.2, "0.5": 0.1}}, {1: "person"}, thr)
    assert store[1] == {"score": {"0": [0.5, 0.2], "0.5": [0.25, 0.1]}, "category": "person", "count": 2.}
    assert store[2]["count"] == 1.
    tab = EV.correctness_table(store, thr)
    m0 = (0.5 + 0.2 + 1.0) / 3
    s0 = np.sqrt(((0.5 - m0) ** 2 + (0.2 - m0) ** 2 + (1.0 - m0) ** 2) / 3)
    assert abs(tab["0"][0] - m0) < 1e-15 and abs(tab["0"][1] - s0) < 1e-15
    m1 = 0.35 / 3
    assert abs(tab["0.5"][0] - m1) < 1e-15
    assert abs(tab["0.5"][1] - np.std([0.25, 0.1, 0.0])) < 1e-15


def test_invalid_arguments_without_gpu():
    from lrp_imagecaptioning_amd import _capi
    lib = _capi.load()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    E = _capi.LRP_ERR_INVALID
    assert lib.lrp_eval_relevance_maps(p, p, 0, 1, 4, 3, 2, None) == E and b"sign" in lib.lrp_last_error()
    assert lib.lrp_eval_relevance_maps(p, p, 0, 1, 4, 3, 0, None) == E
    assert lib.lrp_eval_relevance_maps(None, p, 0, 1, 4, 3, -1, None) == E and b"null" in lib.lrp_last_error()
    assert lib.lrp_eval_relevance_maps(p, p, 2, 1, 4, 3, -1, None) == E
    assert lib.lrp_eval_box_scores(p, 0, 1, 4, 4, p, p, 1, 17, p, None) == E and b"K" in lib.lrp_last_error()
    assert lib.lrp_eval_box_scores(p, 0, 1, 4, 4, p, p, 1, 0, p, None) == E
    assert lib.lrp_eval_box_scores(p, 0, 1, 4, 4, None, p, 1, 10, p, None) == E
    assert lib.lrp_eval_box_scores(p, 0, 1, 4, 4, p, p, 1, 10, None, None) == E
    assert lib.lrp_eval_attention_maps(p, None, p, 1, 14, 16, None) == E
    assert lib.lrp_eval_attention_maps(p, p, p, 1, 17, 16, None) == E
    assert lib.lrp_eval_expand_matrix(14, 16, 20.0, None) == E
    assert lib.lrp_eval_expand_matrix(14, 16, -1.0, p) == E
    assert lib.lrp_eval_expand_matrix(0, 16, 20.0, p) == E


def test_evaluator_arguments():
    class _Ex(object):
        _preprocessor = None
        L = 196

        class _model(object):
            img_hw = (224, 224)
    with pytest.raises(ValueError):
        EV.EvaluationBboxCOCO({}, 20, 3, "eps", "vgg16", _Ex(), sign=0)
    with pytest.raises(ValueError):
        EV.EvaluationBboxCOCO({}, 20, 3, "eps", "vgg16", _Ex(), box_thresholds="carry")
    with pytest.raises(NotImplementedError):
        EV.EvaluationBboxCOCO({}, 20, 3, "eps", "inception_v3", _Ex())
    ev = EV.EvaluationBboxCOCO({}, 20, 3, "eps", "vgg16", _Ex())
    assert ev._reshape_size == (14, 14) and ev._upscale == 16 and ev.sign == -1
