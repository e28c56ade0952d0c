"""CPU checks of the word examination (exaimin_word.py): ROC / AUC without sklearn, the word -> position matching, the
layout and chunking of word_statistics (on a stub engine), and the argument checks of lrp_op_gradcam / lrp_exam_maps
(no GPU needed)."""
import ctypes

import numpy as np
import pytest
import torch

import word_exam_ref as ref
from lrp_imagecaptioning_amd import examination as XW

ROC_CASES = [
    ([1, 0, 1, 0, 1], [0.9, 0.8, 0.7, 0.6, 0.5]),                        # no ties
    ([1, 0, 1, 0, 0, 1], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]),                # one score only: the diagonal
    ([1, 1, 0, 0, 1, 0, 1], [0.3, 0.7, 0.7, 0.3, 0.3, 0.1, 0.9]),        # ties across labels
    ([0, 0, 1, 1], [0.9, 0.8, 0.2, 0.1]),                                # perfectly wrong
    ([0, 1, 1, 1, 0], [-1.0, 0.0, 0.0, 2.0, 2.0]),
]


@pytest.mark.parametrize("labels,scores", ROC_CASES)
def test_roc_auc_equals_pair_count(labels, scores):
    fpr, tpr, thr = XW.roc_curve(labels, scores)
    assert len(fpr) == len(tpr) == len(thr) == len(set(scores)) + 1      # one point per distinct score, after the origin
    assert fpr[0] == 0 and tpr[0] == 0 and fpr[-1] == 1 and tpr[-1] == 1
    assert (np.diff(fpr) >= 0).all() and (np.diff(tpr) >= 0).all() and (np.diff(thr) < 0).all()
    for f, t, th in zip(fpr[1:], tpr[1:], thr[1:]):                      # every point is the sweep at its threshold
        pred = np.asarray(scores) >= th
        y = np.asarray(labels).astype(bool)
        assert f == (pred & ~y).sum() / float((~y).sum()) and t == (pred & y).sum() / float(y.sum())
    assert abs(XW.auc(fpr, tpr) - ref.auc_pairs(labels, scores)) <= 1e-15


def test_roc_auc_random_with_ties():
    rs = np.random.RandomState(3)
    for _ in range(20):
        n = rs.randint(4, 60)
        labels = rs.randint(0, 2, size=n)
        labels[:2] = [0, 1]
        scores = rs.randint(0, 6, size=n) / 5.0
        fpr, tpr, _ = XW.roc_curve(labels, scores)
        assert abs(XW.auc(fpr, tpr) - ref.auc_pairs(labels, scores)) <= 1e-14


def test_single_label_input_raises():
    with pytest.raises(ValueError):
        XW.roc_curve([1, 1, 1], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        XW.roc_curve([0, 0], [0.1, 0.2])
    with pytest.raises(ValueError):
        XW.roc_curve([0, 1], [0.1])
    with pytest.raises(ValueError):
        XW.auc([0.0], [0.0])
    with pytest.raises(ValueError):
        XW.auc([0.0, 1.0, 0.5], [0.0, 1.0, 1.0])


def test_first_index_plus_one():
    cap = "a man and a dog and a man"
    assert XW.get_index(cap, "man") == ref.get_index(cap, "man") == 2
    assert XW.get_index(cap, "dog") == 5 and XW.get_index(cap, "a") == 1
    assert XW.get_index(cap, "do") is None and XW.get_index(cap, "men") is None
    plan = XW.plan_words(["i0", "i1"], [cap, "the hot table"], [[], []], ["dog", "table", "man", "bike"])
    assert plan == [[("dog", 5), ("man", 2)], [("table", 3)]]
    with pytest.raises(ValueError):
        XW.plan_words(["i0"], [cap, cap], [[]], ["dog"])


class _StubEngine(object):
    max_images, max_tokens = 2, 2

    def __init__(self):
        self.calls = []

    def encode_images(self, x):
        self.calls.append(("encode", len(x)))

    def decoder_forward(self, caps):
        self.calls.append(("forward", [list(c) for c in caps]))


class _StubExplainer(object):
    L = 16

    class _model(object):
        img_hw = (64, 64)

    class _dataset_provider(object):
        image_preprocessor = None
        caption_preprocessor = None

    def __init__(self):
        self._engine = _StubEngine()
        self.caption = [1]
        self._state_cache = {"x": 1}


class _StubExaminer(XW.WordExaminer):
    _stats = ("lrp_mean", "attention_mean")

    def _statistics(self, ii, ts):
        self._explainer._engine.calls.append(("stats", list(ii), list(ts)))
        v = np.array([[10 * i + t for i, t in zip(ii, ts)], [-(10 * i + t) for i, t in zip(ii, ts)]], dtype=np.float64)
        return torch.as_tensor(v)


class _Spec(object):
    img_encoder = "vgg16"


def test_word_statistics_layout_and_chunks():
    ex = _StubExplainer()
    xm = _StubExaminer(_Spec(), None, ex, 8, 3)
    assert xm._reshape_size == (4, 4) and xm._upscale == 16
    pred = ["a man riding a bike", "the hot table", "a dog on the table and a man", "women riding"]
    true = [["a man on a bike"], ["a table"], ["a dog", "one table"], ["women"]]
    caps = [[3, 4, 5, 3, 6, 1], [7, 8, 9, 1], [3, 4, 5, 6, 7, 8, 3, 9, 1], [4, 5, 1]]
    names = ["i0", "i1", "i2", "i3"]
    got = xm.word_statistics(np.zeros((4, 64, 64, 3)), names, pred, true, ["man", "dog", "table"], captions=caps)
    assert sorted(got) == ["i0", "i1", "i2"]                                # i3 has no category word
    assert set(got["i2"]) == {"predict_caption", "true_captions", "lrp_mean", "attention_mean"}
    assert got["i2"]["predict_caption"] == pred[2] and got["i2"]["true_captions"] == true[2]
    assert got["i0"]["lrp_mean"] == [("man", 2.0)] and got["i1"]["attention_mean"] == [("table", -13.0)]
    assert got["i2"]["lrp_mean"] == [("man", 8.0), ("dog", 2.0), ("table", 5.0)]       # category_list order, image 0 of chunk 2
    calls = ex._engine.calls
    assert [c for c in calls if c[0] == "stats"] == [("stats", [0, 1], [2, 3]), ("stats", [0, 0], [8, 2]), ("stats", [0], [5])]
    assert [c for c in calls if c[0] == "encode"] == [("encode", 2), ("encode", 2)]
    assert ex.caption is None and ex._state_cache == {}
    with pytest.raises(NotImplementedError):                                # a position past the id caption
        xm.word_statistics(np.zeros((1, 64, 64, 3)), ["i0"], [pred[2]], [[]], ["man"], captions=[[3, 4, 1]])
    # labels and AUC of the result
    labels, scores = XW.word_labels(got, "lrp_mean")
    assert (labels, scores) == ref.labels_scores(got, "lrp_mean")
    assert labels == [1, 1, 0, 1, 1]
    fpr, tpr, a = XW.category_roc_auc(got, "lrp_mean")
    assert abs(a - ref.auc_pairs(labels, scores)) <= 1e-15
    b = {"i": {"true_captions": ["a dog"], "beta": [("dog", 0.25), ("man", 0.5)]}}
    assert XW.word_labels(b, "beta") == ([1, 0], [0.75, 0.5])                # the beta score is 1 - beta
    assert XW.word_labels(b, "beta", score=lambda v: v) == ([1, 0], [0.25, 0.5])


def test_invalid_arguments_without_gpu():
    from lrp_imagecaptioning_amd import _capi
    lib = _capi.load()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    E = _capi.LRP_ERR_INVALID

    def cam(feat=p, idx=p, grads=p, M=p, gb=None, cam=p, out=None, n=1, B=1, g=14, up=16, D=512, C=3):
        return lib.lrp_op_gradcam(feat, idx, grads, M, gb, cam, out, n, B, g, up, D, C, None)
    for kw in ({"feat": None}, {"idx": None}, {"grads": None}, {"M": None}, {"cam": None}):
        assert cam(**kw) == E and b"null" in lib.lrp_last_error(), kw
    assert cam(gb=p) == E and cam(out=p) == E                               # the gate's two pointers go together
    assert cam(g=0) == E and b"g" in lib.lrp_last_error()
    assert cam(g=17) == E
    assert cam(g=14, up=33) == E                                            # S = 462 > 448
    assert cam(up=0) == E
    assert cam(D=510) == E and b"D" in lib.lrp_last_error()
    assert cam(D=0) == E and cam(D=8192) == E
    assert cam(n=0) == E and cam(B=0) == E
    assert cam(gb=p, out=p, C=0) == E

    def exam(R=p, fp64=0, n=1, H=32, W=32, C=3, pool=0, k=0, absval=0, maps=p, means=p):
        return lib.lrp_exam_maps(R, fp64, n, H, W, C, pool, k, absval, maps, means, None)
    assert exam(R=None) == E and b"null" in lib.lrp_last_error()
    assert exam(maps=None, means=None) == E and b"null" in lib.lrp_last_error()
    assert exam(pool=1, k=5) == E and b"divide" in lib.lrp_last_error()     # H % k != 0
    assert exam(pool=2, k=16, W=40) == E
    assert exam(pool=1, k=0) == E
    assert exam(pool=3, k=4) == E
    assert exam(fp64=2) == E and exam(absval=2) == E
    assert exam(n=0) == E and exam(H=0) == E and exam(C=0) == E
