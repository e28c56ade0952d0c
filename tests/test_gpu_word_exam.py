"""-m gpu: the word examination on the device (lrp_exam_maps, examination.py) and the batched Guided Grad-CAM
(LRPEngine.guided_gradcam, explain_words, EvaluationBboxCOCOBaseline(device_gradcam=True)) against the numpy restatements
of tests/word_exam_ref.py and tests/bbox_eval_ref.py and against the unchanged per-word paths."""
import numpy as np
import pytest
import torch

import bbox_eval_ref as bref
import word_exam_ref as ref
from conftest import rel_l1
from gpu_util import report
from lrp_imagecaptioning_amd import engine as E
from lrp_imagecaptioning_amd import evaluation as EV
from lrp_imagecaptioning_amd import examination as XW
from test_gpu_eval_bbox import CAPS, EXT, FILT, _category, _explainer, _host_baseline, _relevance_batch, _same

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_MAPS = 6
_BATCH = {}


def batch(hw, dtype):
    """An all-zero map, a single non-zero, integer ties, an all-positive map and mixed scales; map 4 also has channels
    of very different size, where the order of the channel sum shows.  Shared and never modified."""
    key = (hw, np.dtype(dtype).name)
    if key not in _BATCH:
        rs = np.random.RandomState(hw)
        R = _relevance_batch(rs, N_MAPS, hw, hw, dtype)
        R[4] *= np.array([1.0, 1e3, 1e-3], dtype=dtype)
        R.setflags(write=False)
        _BATCH[key] = R
    return _BATCH[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _literal(R, i, pool, k, dtype):
    want = ref.exam_map(R[i:i + 1], pool, k)
    if want.dtype != dtype:                                   # the reference's zeros of an all-zero map are float64
        assert not want.any()
        want = want.astype(dtype)
    return want


@pytest.mark.parametrize("pool,k", [(None, None), ("max", 4), ("max", 16)])
@pytest.mark.parametrize("hw", [32, 224])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_maps_bitwise_and_means(dtype, hw, pool, k):
    R = batch(hw, dtype)
    Rd = torch.as_tensor(np.array(R)).to(DEV)                # a copy: the cached batch is read-only
    maps, means = E.exam_maps(Rd, pool=pool, k=k)
    maps, means = maps.cpu().numpy(), means.cpu().numpy()
    out_dtype = dtype if pool is None else np.float64
    side = hw if pool is None else hw // k
    assert maps.dtype == out_dtype and maps.shape == (N_MAPS, side, side) and means.dtype == np.float64
    for i in range(N_MAPS):
        assert np.array_equal(_bits(maps[i]), _bits(_literal(R, i, pool, k, out_dtype))), i
    assert not maps[0].any() and means[0] == 0
    amaps, ameans = E.exam_maps(Rd, pool=pool, k=k, absval=True)
    amaps, ameans = amaps.cpu().numpy(), ameans.cpu().numpy()
    assert np.array_equal(_bits(amaps), _bits(np.abs(maps)))
    # means: map values are bounded by 1, so this is fp64 reassociation over <= 50 176 terms
    err = max(np.abs(means - maps.astype(np.float64).mean(axis=(1, 2))).max(),
              np.abs(ameans - np.abs(maps).astype(np.float64).mean(axis=(1, 2))).max())
    own = max(abs(means[i] - float(np.mean(maps[i]))) for i in range(N_MAPS))        # the reference's np.mean in the map's dtype
    report("exam_maps_mean", dtype=np.dtype(dtype).name, hw=hw, pool=str(pool), k=k or 0, max_abs_vs_f64=err,
           max_abs_vs_reference_mean=own)
    print("exam_maps", dtype, hw, pool, k, "means vs f64 %.3e, vs the reference's own np.mean %.3e" % (err, own))
    assert err <= 1e-12, err
    # the statistic alone, and one map alone
    none, only = E.exam_maps(Rd, pool=pool, k=k, want_maps=False)
    assert none is None and np.array_equal(_bits(only.cpu().numpy()), _bits(means))
    m1, s1 = E.exam_maps(Rd[4:5], pool=pool, k=k)
    assert np.array_equal(_bits(m1.cpu().numpy()[0]), _bits(maps[4])) and np.array_equal(_bits(s1.cpu().numpy()), _bits(means[4:5]))


@pytest.mark.parametrize("k", [4, 16])
@pytest.mark.parametrize("hw", [32, 224])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ave_pooled_maps(dtype, hw, k):
    R = batch(hw, dtype)
    want = []
    for i in range(N_MAPS):
        # the bound below is fp64 reassociation (~1e-12) divided by pooled absmax / max|m|: assert that ratio first
        m = ref.channel_mean(R[i:i + 1]).astype(np.float64)
        pooled = m.reshape(hw // k, k, hw // k, k).transpose(0, 2, 1, 3).reshape(hw // k, hw // k, k * k).sum(axis=-1) / (k * k)
        assert np.abs(pooled).max() >= 1e-3 * np.abs(m).max(), i
        want.append(ref.exam_map_f64(R[i:i + 1], "ave", k))
    want = np.stack(want)
    maps, means = E.exam_maps(torch.as_tensor(np.array(R)).to(DEV), pool="ave", k=k)
    maps, means = maps.cpu().numpy(), means.cpu().numpy()
    assert maps.dtype == np.float64 and maps.shape == want.shape
    err = np.abs(maps - want).max()
    lit = max(np.abs(maps[i] - ref.exam_map(R[i:i + 1], "ave", k)).max() for i in range(N_MAPS))
    report("exam_maps_ave", dtype=np.dtype(dtype).name, hw=hw, k=k, max_abs_vs_f64=err, max_abs_vs_reference_loop=lit)
    print("exam_maps ave", dtype, hw, k, "vs f64 %.3e, vs the reference's loop (not asserted) %.3e" % (err, lit))
    assert err <= 1e-9, err
    assert not maps[0].any()
    assert np.abs(means - maps.mean(axis=(1, 2))).max() <= 1e-12
    m1, _ = E.exam_maps(torch.as_tensor(np.array(R[2:3])).to(DEV), pool="ave", k=k)
    assert np.array_equal(_bits(m1.cpu().numpy()[0]), _bits(maps[2]))


def test_exam_maps_refuses_bad_arguments():
    R = torch.zeros((1, 32, 32, 3), device=DEV)
    with pytest.raises(ValueError):
        E.exam_maps(R, pool="max", k=5)
    with pytest.raises(ValueError):
        E.exam_maps(R, pool="min", k=4)
    with pytest.raises(ValueError):
        E.exam_maps(R[0])
    with pytest.raises(ValueError):
        E.exam_maps(R.to(torch.float16))


# ------------------------------------------------------------------------------------------ explainers
def _composition(ex, X, t):
    """The float64-cam host path of one word: guided backprop of the engine x grad_cam64 -> (H, W, 3) float64."""
    from lrp_imagecaptioning_amd.explainers import _GradientMixin
    d = ex._lstm_decoder_backward(t)
    gb = _GradientMixin._explain_CNN(ex, X, d)
    g = int(np.sqrt(ex.L))
    cam = ref.grad_cam64(ex._engine.get_features()[0].cpu().numpy(), d[0], g, ex._model.img_hw[0] // g)
    return gb[0].astype(np.float64) * cam[..., None]


RESNET = {"stem": 8, "stacks": ((8, 1), (8, 1), (8, 1), (8, 1))}


@pytest.mark.parametrize("cls,hw,resnet", [("ExplainImgCaptioningAdaptiveAttentionGuidedGradcam", 16, None),
                                           ("ExplainImgCaptioningGridTDGuidedGradcam", 16, None),
                                           ("ExplainImgCaptioningAdaptiveAttentionGuidedGradcam", 224, RESNET)])
def test_explain_words_matches_per_word_paths(cls, hw, resnet):
    kind = "gridtd" if "GridTD" in cls else "adaptive"
    ex, rs = _explainer(cls, kind, max_images=2, hw=hw, resnet=resnet, seed=3)
    X = rs.uniform(-120, 130, size=(2, hw, hw, 3)).astype(np.float32)
    caps = CAPS[:2]
    ones, l1, err = [], 0.0, 0.0
    for b in range(2):
        ex._forward_beam_search((None, X[b:b + 1]), caps[b])
        ts = list(range(1, len(caps[b])))
        got, cam = ex.explain_words(ts, want_cam=True)
        assert got.dtype == torch.float64 and tuple(got.shape) == (len(ts), hw, hw, 3) and tuple(cam.shape) == (len(ts), hw, hw)
        assert torch.equal(ex.explain_sentence_cnn(), got)
        d = ex._engine.decoder_gradient([0] * len(ts), ts)[0]
        assert torch.equal(ex.grad_cam_device(d), cam)
        assert torch.equal(ex.grad_cam_device(d.reshape(len(ts), int(np.sqrt(ex.L)), -1, ex.D).cpu().numpy()), cam)
        got = got.cpu().numpy()
        ones.append(got)
        for j, t in enumerate(ts):
            word = ex._explain_CNN(X[b:b + 1], ex._lstm_decoder_backward(t))[0]     # the unchanged per-word host path
            if np.abs(word).sum() > 0:
                l1 = max(l1, rel_l1(got[j], word))
            else:
                assert not got[j].any()
            want = _composition(ex, X[b:b + 1], t)
            err = max(err, np.abs(got[j] - want).max() / max(np.abs(want).max(), 1e-300))
            assert np.abs(got[j] - want).max() <= 1e-12 * np.abs(want).max(), (b, t)
    assert any(o.any() for o in ones)
    report("explain_words", cls=cls, hw=hw, rel_l1_vs_per_word=l1, max_rel_vs_f64_composition=err)
    print("explain_words", cls, hw, "rel L1 vs per-word %.3e, vs float64 composition %.3e" % (l1, err))
    assert l1 < 1e-4, l1
    assert ex._batched_cnn is False
    # both images in one chain (max_images = 2): every map bit-identical to its one-image run
    eng = ex._engine
    eng.encode_images(X)
    eng.decoder_forward(caps)
    units = [(b, t) for b in range(2) for t in range(1, len(caps[b]))]
    both = eng.guided_gradcam([u[0] for u in units], [u[1] for u in units]).cpu().numpy()
    assert np.array_equal(_bits(both), _bits(np.concatenate(ones)))


# ------------------------------------------------------------------------------------------ evaluator
def test_evaluator_device_gradcam():
    cls = "ExplainImgCaptioningAdaptiveAttentionGuidedGradcam"
    ex, rs = _explainer(cls, "adaptive", max_images=2, seed=4)
    X = rs.uniform(-120, 130, size=(3, 32, 32, 3)).astype(np.float32)
    cats = {"img%d" % b: _category(rs, 32) for b in range(3)}
    kw = dict(category_extension=EXT, word_filter=FILT)
    ev = EV.EvaluationBboxCOCOBaseline(cats, 8, 3, "eps", "vgg16", ex, device_gradcam=True, **kw)
    got = ev.evaluate_batch(X, list(cats), CAPS[:3])
    assert ex._batched_cnn is False
    assert any(got[b][0] for b in range(3))
    off = EV.EvaluationBboxCOCOBaseline(cats, 8, 3, "eps", "vgg16", ex, device_gradcam=False, **kw).evaluate_batch(X, list(cats), CAPS[:3])
    default = EV.EvaluationBboxCOCOBaseline(cats, 8, 3, "eps", "vgg16", ex, **kw).evaluate_batch(X, list(cats), CAPS[:3])
    assert off == default                                     # the keyword's default is today's path ...
    worst, moved = 0.0, 0.0
    for b in range(3):
        Xb, cat = X[b:b + 1], cats["img%d" % b]
        _same(default[b], _host_baseline(ex, Xb, CAPS[b], cat))           # ... which is the per-word host path
        ex._forward_beam_search((None, Xb), CAPS[b])
        word = lambda t: [bref.relevance_map(_composition(ex, Xb, t)[None])]
        want = bref.evaluate_image(word, CAPS[b], ex._preprocessor._word_of, cat, EXT, FILT, 1)
        worst = max(worst, _same(got[b], want))
        for cid in default[b][0]:
            for k, v in default[b][0][cid].items():
                moved = max(moved, abs(v - got[b][0][cid][k]))
    report("eval_bbox_device_gradcam", max_abs_vs_f64_cam_host=worst, max_abs_vs_default_per_word_path=moved)
    print("device_gradcam scores: vs float64-cam host path %.3e, vs the default per-word path (not asserted) %.3e" % (worst, moved))
    # a plain gradient explainer ignores the keyword
    ex2, _ = _explainer("ExplainImgCaptioningAdaptiveAttentionGradient", "adaptive", max_images=2, seed=4)
    a = EV.EvaluationBboxCOCOBaseline(cats, 8, 3, "eps", "vgg16", ex2, device_gradcam=True, **kw).evaluate_batch(X, list(cats), CAPS[:3])
    assert a == EV.EvaluationBboxCOCOBaseline(cats, 8, 3, "eps", "vgg16", ex2, **kw).evaluate_batch(X, list(cats), CAPS[:3])


# ------------------------------------------------------------------------------------------ word_statistics
CATEGORIES = ["bike", "dog", "table"]
TRUE = [["a bike on a table"], ["a dog", "one dog"], ["women"], ["the cat"]]


def _setup(cls, kind):
    ex, rs = _explainer(cls, kind, max_images=2, seed=5)
    X = rs.uniform(-120, 130, size=(4, 32, 32, 3)).astype(np.float32)
    names = ["img%d" % b for b in range(4)]
    pred = [ex._preprocessor.decode_captions_from_list1d(c) for c in CAPS]
    return ex, X, names, pred


def _check_layout(got, names, pred):
    assert sorted(got) == [names[0], names[1], names[3]]                       # "on women riding" names no category
    assert [c for c, _ in got[names[0]][list(got[names[0]])[0]]] == ["bike", "table"]
    for b in (0, 1, 3):
        assert got[names[b]]["predict_caption"] == pred[b] and got[names[b]]["true_captions"] == TRUE[b]


def _check_auc(got, key):
    labels, scores = ref.labels_scores(got, key, (lambda v: 1 - v) if key == "beta" else (lambda v: v))
    assert sorted(set(labels)) == [0, 1]
    fpr, tpr, a = XW.category_roc_auc(got, key)
    assert abs(a - ref.auc_pairs(labels, scores)) <= 1e-12


@pytest.mark.parametrize("kind,cls", [("adaptive", "ExplainImgCaptioningAdaptiveAttention"),
                                      ("gridtd", "ExplainImgCaptioningGridTDModel")])
def test_word_statistics_lrp(kind, cls):
    ex, X, names, pred = _setup(cls, kind)
    xm = XW.WordExaminer(ex._model, None, ex, 8, 3)
    assert xm._reshape_size == (8, 8) and xm._upscale == 4
    got = xm.word_statistics(X, names, pred, TRUE, CATEGORIES, captions=CAPS)
    _check_layout(got, names, pred)
    worst = 0.0
    for b in (0, 1, 3):
        entry = got[names[b]]
        assert set(entry) == {"predict_caption", "true_captions", "lrp_mean", "attention_mean", "beta"}
        Xb = (None, X[b:b + 1])
        for j, (cat, _) in enumerate(entry["lrp_mean"]):
            t = ref.get_index(pred[b], cat)
            hp, atn = xm._explain_single_word(Xb, CAPS[b], t)                     # the per-word path
            assert hp.dtype == np.float32 and hp.shape == (32, 32) and atn.shape == (32, 32)
            beta = ex._engine.read_state("beta")[0, t, 0].item()
            assert entry["beta"][j] == (cat, beta)
            assert entry["attention_mean"][j][0] == cat
            worst = max(worst, abs(entry["lrp_mean"][j][1] - np.mean(hp.astype(np.float64))),
                        abs(entry["attention_mean"][j][1] - np.mean(atn)))
            assert np.array_equal(_bits(xm._get_explanation_single_word(Xb, CAPS[b], t)), _bits(hp))
    report("word_statistics", cls=cls, max_abs_vs_per_word=worst)
    assert worst <= 1e-9, worst
    for key in ("lrp_mean", "attention_mean", "beta"):
        _check_auc(got, key)
    # the pooled single-word form against the literal loops
    Xb = (None, X[3:4])
    rel = xm._relevance(Xb, CAPS[3], 3)[0].cpu().numpy()
    m = ref.channel_mean(rel).astype(np.float64)
    assert np.abs(m.reshape(8, 4, 8, 4).mean(axis=(1, 3))).max() >= 1e-3 * np.abs(m).max()   # see test_ave_pooled_maps
    for kind_ in ("max", "ave"):
        hp, atn = xm._explain_single_word_pooling(Xb, CAPS[3], 3, kind_)
        assert hp.shape == (8, 8) and atn.shape == (64,)
        assert np.abs(hp - ref.exam_map_f64(rel, kind_, 4)).max() <= 1e-9
        if kind_ == "max":
            assert np.array_equal(_bits(hp), _bits(ref.exam_map(rel, "max", 4)))
    att = ex._explain_lstm_single_word_sequence(3)[1]
    assert np.array_equal(_bits(atn), _bits(ref.project(att).astype(atn.dtype)))


def test_word_statistics_guided_gradcam():
    cls = "ExplainImgCaptioningAdaptiveAttentionGuidedGradcam"
    ex, X, names, pred = _setup(cls, "adaptive")
    xm = XW.WordExaminerGuidedgradcam(ex._model, None, ex, 8, 3)
    got = xm.word_statistics(X, names, pred, TRUE, CATEGORIES, captions=CAPS)
    _check_layout(got, names, pred)
    worst, host = 0.0, 0.0
    for b in (0, 1, 3):
        entry = got[names[b]]
        assert set(entry) == {"predict_caption", "true_captions", "guidedgradcam_mean"}
        Xb = X[b:b + 1]
        for cat, value in entry["guidedgradcam_mean"]:
            t = ref.get_index(pred[b], cat)
            ex._forward_beam_search((None, Xb), CAPS[b])
            hp = ref.exam_map(_composition(ex, Xb, t)[None])                      # the float64-cam composition
            worst = max(worst, abs(value - np.mean(np.abs(hp))))
            host = max(host, abs(value - np.mean(np.abs(xm._explain_single_word((None, Xb), CAPS[b], t)))))
    report("word_statistics", cls=cls, max_abs_vs_f64_composition=worst, max_abs_vs_per_word_f32_cam=host)
    print("guidedgradcam_mean: vs float64-cam composition %.3e, vs the float32-cam per-word path (not asserted) %.3e" % (worst, host))
    assert worst <= 1e-9, worst
    _check_auc(got, "guidedgradcam_mean")
