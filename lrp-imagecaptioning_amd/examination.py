"""Word examination (the reference's exaimin_word.py, cited XW:): for every frequent object word of a predicted caption
one statistic of its explanation; the ROC / AUC of that statistic separates grounded words from hallucinated ones.

    WordExaminer                XW:27-179   LRP heat-map + attention map of one word (plain and pooled)
    WordExaminerGuidedgradcam   XW:181-300  the Guided Grad-CAM map of one word
    word_statistics             XW:371-617  the statistics of all category words of a set of images, batched
    roc_curve / auc / category_roc_auc      XW:623-742 without sklearn (host only)

The single-word methods keep the reference's surface and return numpy maps.  `word_statistics` is the batched form the
reference lacks: all (image, word) units of `max_images` images go through one launch chain, the maps are normalised and
reduced on the device (lrp_exam_maps, lrp_eval_attention_maps, lrp_op_gradcam) and only the (n,) statistics come back.

Differences from the reference: the grid side and the upscale come from the explainer (not a hard-coded 14 / 16), the pool
block is upscale x upscale so that any grid up to 16 x 16 works, and `_explain_lstm_single_word_sequence` is called without
the `rule='eps'` argument E:537 does not accept.
"""
import numpy as np
import torch

from . import engine as _eng

SIGMA = 20
_ENCODERS = ("vgg16", "vgg19", "resnet101")


def get_index(caption, category):
    """XW:372-377: 1 + the first position of `category` among caption.split(' '), or None."""
    words = caption.split(" ")
    for t in range(len(words)):
        if category == words[t]:
            return t + 1
    return None


class WordExaminer(object):
    """XW:27-179 on the engine."""
    _stats = ("lrp_mean", "attention_mean", "beta")

    def __init__(self, model, weight_path, explainer, max_caption_length, beam_size):
        if model.img_encoder not in _ENCODERS:
            raise NotImplementedError("the img_encode is not valid, [vgg16, vgg19, resnet101]")
        self._img_encoder = model.img_encoder
        self._image_preprocessor = explainer._dataset_provider.image_preprocessor
        self._caption_preprocessor = explainer._dataset_provider.caption_preprocessor
        self._explainer = explainer
        self._max_caption_length = max_caption_length
        self._beam_size = beam_size
        self._color_conversion = "BGRtoRGB"
        g = int(round(np.sqrt(explainer.L)))
        self._reshape_size = (g, g)
        self._upscale = explainer._model.img_hw[0] // g

    # ---------------------------------------------------------------- the reference's surface
    def _preprocess_img(self, img_path):
        if self._image_preprocessor is None:
            from .harness import ImagePreprocessor
            self._image_preprocessor = ImagePreprocessor(self._img_encoder)
        imgs = self._image_preprocessor.preprocess_images(img_path)
        return (self._caption_preprocessor.SOS_TOKEN_LABEL_ENCODED, self._image_preprocessor.preprocess_batch(imgs))

    def _predict_caption(self, X):
        return self._explainer._beam_search(X, beam_size=self._beam_size)[0]

    def _relevance(self, X, captions, t):
        """-> ((1, H, W, 3) relevance tensor on the device, attention (L,) float32 array or None)."""
        ex = self._explainer
        ex._forward_beam_search(X, captions)
        R, attention = ex._explain_lstm_single_word_sequence(t)
        return ex._explain_CNN(X[1], R, as_tensor=True), np.asarray(attention, dtype=np.float32)

    def _explain_single_word(self, X, captions, t):
        """XW:79-111 -> (hp (H, W) in the relevance dtype, atn (S, S) float64)."""
        rel, attention = self._relevance(X, captions, t)
        g = self._reshape_size[0]
        hp = _eng.exam_maps(rel)[0][0].cpu().numpy()
        att = torch.as_tensor(attention.reshape(1, g * g)).to(rel.device)
        atn = _eng.eval_attention_maps(att, g, self._upscale, SIGMA)[0].cpu().numpy()
        return hp, atn

    def _get_explanation_single_word(self, X, captions, t):
        """XW:113-129."""
        rel, _ = self._relevance(X, captions, t)
        return _eng.exam_maps(rel)[0][0].cpu().numpy()

    def _explain_single_word_pooling(self, X, captions, t, poolingtype="max"):
        """XW:131-160 -> (hp (g, g) float64, atn (L,) = project(attention))."""
        rel, attention = self._relevance(X, captions, t)
        g = self._reshape_size[0]
        hp = self._pooled(rel, poolingtype)
        att = torch.as_tensor(attention.reshape(1, g, g, 1)).to(rel.device)
        atn = _eng.exam_maps(att)[0][0].cpu().numpy().reshape(-1)
        return hp, atn

    def _pooled(self, rel, poolingtype):
        if poolingtype not in ("max", "ave"):                # XW:150-153 pools for these two only
            return _eng.exam_maps(rel)[0][0].cpu().numpy()
        return _eng.exam_maps(rel, pool=poolingtype, k=self._upscale)[0][0].cpu().numpy()

    def analyze_single_word(self, img_path, t):
        self.img_path = img_path
        X = self._preprocess_img([img_path])
        return self._explain_single_word(X, self._predict_caption(X), t)

    def analyze_single_word_pooling(self, img_path, t, poolingtype="max"):
        self.img_path = img_path
        X = self._preprocess_img([img_path])
        return self._explain_single_word_pooling(X, self._predict_caption(X), t, poolingtype=poolingtype)

    # ---------------------------------------------------------------- batched statistics (new)
    def word_statistics(self, images, img_filenames, predicted_captions, true_captions, category_list, captions=None):
        """XW:371-617 for a set of images in one pass.  images (B, H, W, 3) preprocessed; predicted_captions: one string
        per image; true_captions: the list of annotated captions per image; captions: one id list per image (None: beam
        search).  For every image, each category word's first position in the predicted caption (+ 1) is explained, in
        chunks of `max_images` images and `max_tokens` words.  Returns the reference's save_dict
        {filename: {'predict_caption', 'true_captions', '<stat>': [(category, value), ...]}}; images without a category
        word have no entry."""
        images = np.asarray(images, dtype=np.float32)
        ex = self._explainer
        eng = ex._engine
        B = len(images)
        if captions is None:
            res = ex._beam_search((None, images), beam_size=self._beam_size)
            captions = [res[0]] if B == 1 else [r[0] for r in res]
        captions = [list(map(int, c)) for c in captions]
        plan = plan_words(img_filenames, predicted_captions, true_captions, category_list)
        for b, f in enumerate(img_filenames):
            for _, t in plan[b]:
                if t > len(captions[b]):
                    raise NotImplementedError("index out of range of captions")          # E:538-539
        save = {}
        for lo in range(0, B, eng.max_images):
            hi = min(B, lo + eng.max_images)
            units = [(b - lo, t, b, cat) for b in range(lo, hi) for cat, t in plan[b]]
            if not units:
                continue
            eng.encode_images(images[lo:hi])
            eng.decoder_forward(captions[lo:hi])
            vals = []
            for u0 in range(0, len(units), eng.max_tokens):
                chunk = units[u0:u0 + eng.max_tokens]
                vals.append(self._statistics([u[0] for u in chunk], [u[1] for u in chunk]))
            vals = torch.cat(vals, dim=1).cpu().numpy()           # (len(_stats), n): the only device-to-host copy
            for j, (_, _, b, cat) in enumerate(units):
                f = img_filenames[b]
                if f not in save:
                    save[f] = {s: [] for s in self._stats}
                    save[f]["predict_caption"] = predicted_captions[b]
                    save[f]["true_captions"] = true_captions[b]
                for i, s in enumerate(self._stats):
                    save[f][s].append((cat, float(vals[i, j])))
        ex.caption = None                                    # the engine's caches now hold the last chunk
        ex._state_cache = {}
        return save

    def _statistics(self, ii, ts):
        """(len(_stats), n) float64 tensor for the units (ii, ts) of the engine's current forward."""
        eng = self._explainer._engine
        g = self._reshape_size[0]
        R, _, att, _ = eng.explain_tokens(ii, ts, want_attention=True)
        lrp = _eng.exam_maps(R, want_maps=False)[1]
        atn = _eng.eval_attention_maps(att, g, self._upscale, SIGMA)
        atn = _eng.exam_maps(atn.unsqueeze(-1), want_maps=False)[1]         # the maps are projected already: x / 1
        i_dev = torch.as_tensor(np.asarray(ii, dtype=np.int64)).to(eng.device)
        t_dev = torch.as_tensor(np.asarray(ts, dtype=np.int64)).to(eng.device)
        beta = eng.read_state("beta")[i_dev, t_dev, 0].to(torch.float64)    # XW:411: beta[index], row 0 = the zero init
        return torch.stack([lrp, atn, beta])


class WordExaminerGuidedgradcam(WordExaminer):
    """XW:181-300: the same surface on a Guided Grad-CAM explainer; the single-word methods return hp only."""
    _stats = ("guidedgradcam_mean",)

    def _relevance(self, X, captions, t):
        ex = self._explainer
        ex._forward_beam_search(X, captions)
        rel = ex._explain_CNN(X[1], ex._lstm_decoder_backward(t))            # the per-word host path, float64
        return torch.as_tensor(np.ascontiguousarray(rel)).to(ex._engine.device), None

    def _explain_single_word(self, X, captions, t):
        """XW:235-255."""
        return _eng.exam_maps(self._relevance(X, captions, t)[0])[0][0].cpu().numpy()

    _get_explanation_single_word = _explain_single_word

    def _explain_single_word_pooling(self, X, captions, t, poolingtype="max"):
        """XW:257-281."""
        return self._pooled(self._relevance(X, captions, t)[0], poolingtype)

    def _statistics(self, ii, ts):
        """XW:487-489: mean(|hp|) of the batched Guided Grad-CAM maps (LRPEngine.guided_gradcam)."""
        out = self._explainer._engine.guided_gradcam(ii, ts)
        return _eng.exam_maps(out, absval=True, want_maps=False)[1].unsqueeze(0)


def plan_words(img_filenames, predicted_captions, true_captions, category_list):
    """Host planning of word_statistics: per image the [(category, t)] of XW:439-442, in category_list order."""
    if not (len(img_filenames) == len(predicted_captions) == len(true_captions)):
        raise ValueError("one predicted caption and one list of true captions per image")
    plan = []
    for cap in predicted_captions:
        words = cap.split()
        per = []
        for category in category_list:
            if category in words:
                index = get_index(cap, category)
                if index:
                    per.append((category, index))
        plan.append(per)
    return plan


# ---------------------------------------------------------------------------------------------------- ROC / AUC (host)
def roc_curve(labels, scores):
    """The threshold sweep `sklearn.metrics.roc_curve` performs (XW:649): one point per distinct score, from the highest
    down, after the origin.  -> (fpr, tpr, thresholds); thresholds[0] = inf.  Labels are 0 / 1; input with one label only
    has no ROC curve: ValueError."""
    y = np.asarray(labels).astype(bool).reshape(-1)
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    if len(y) != len(s):
        raise ValueError("labels and scores differ in length")
    P, N = int(y.sum()), int((~y).sum())
    if P == 0 or N == 0:
        raise ValueError("roc_curve needs at least one positive and one negative label")
    order = np.argsort(-s, kind="mergesort")
    y, s = y[order], s[order]
    last = np.r_[np.where(np.diff(s))[0], len(s) - 1]         # the last index of every run of equal scores
    tps = np.cumsum(y)[last]
    fps = (1 + last) - tps
    return np.r_[0.0, fps / float(N)], np.r_[0.0, tps / float(P)], np.r_[np.inf, s[last]]


def auc(fpr, tpr):
    """Trapezoidal area under (fpr, tpr) (XW:650); fpr must be monotonic."""
    x, y = np.asarray(fpr, dtype=np.float64), np.asarray(tpr, dtype=np.float64)
    if len(x) < 2 or len(x) != len(y):
        raise ValueError("auc needs at least two points")
    dx = np.diff(x)
    if (dx < 0).any() and (dx > 0).any():
        raise ValueError("fpr is not monotonic")
    sign = -1.0 if (dx < 0).any() else 1.0
    return float(sign * np.sum(dx * (y[1:] + y[:-1]) / 2.0))


def word_labels(save_dict, key, score=None):
    """XW:631-647: (labels, scores) of every (category, value) under `key`; a word is a true positive if it occurs in
    .split() of any true caption.  score: value -> score (default: the value; 1 - beta for key 'beta', XW:643)."""
    if score is None:
        score = (lambda v: 1 - v) if key == "beta" else (lambda v: v)
    labels, scores = [], []
    for entry in save_dict.values():
        for category, value in entry[key]:
            labels.append(int(any(category in cap.split() for cap in entry["true_captions"])))
            scores.append(score(value))
    return labels, scores


def category_roc_auc(save_dict, key, score=None):
    """XW:623-742 for one statistic -> (fpr, tpr, auc)."""
    labels, scores = word_labels(save_dict, key, score)
    fpr, tpr, _ = roc_curve(labels, scores)
    return fpr, tpr, auc(fpr, tpr)
