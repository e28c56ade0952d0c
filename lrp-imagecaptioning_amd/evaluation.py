"""Bounding-box correctness evaluation (the reference's evaluate_bbox.py, cited EB:): for every caption word that names an
annotated object, the share of the word's heat-map (and attention map) inside the object's boxes, at ten thresholds.

    EvaluationBboxCOCO          EB:38-272   LRP heat-map + attention map per object word
    EvaluationBboxCOCOBaseline  EB:273-358  gradient baselines (Gradient, Input x Gradient, Guided Grad-CAM)
    accumulate / correctness_table          EB:384-411 (score files) and EB:823-915 (table)

`evaluate(X, data)` keeps the reference's surface and return values.  `evaluate_batch` explains every object word of a
batch in one launch chain; the maps stay on the device (lrp_eval_relevance_maps / _attention_maps / _box_scores) and only
the (boxes x thresholds) scores come back.  Explainers whose `_explain_CNN` is host-side (the Guided Grad-CAM classes)
take the per-word path; their float64 maps are uploaded and scored in float64 — unless EvaluationBboxCOCOBaseline is
built with device_gradcam=True, which computes their Grad-CAM factor on the device and batches them like the others.

The category synonym table and the word filter list are constructor keywords (the reference's CATEGORY_EXTENSION and
FILTER, EB:11-21, are the caller's to pass).
"""
import numpy as np
import torch

from . import engine as _eng

THRESHOLDS = (0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)
_ENCODERS = ("vgg16", "vgg19", "resnet101")
SIGMA = 20


def match_categories(caption, word_of, categories, category_extension=None, word_filter=()):
    """EB:218-232: caption positions 0 .. len-2 -> ({cat_id: [(t, word), ...]}, {cat_id: category name}); t = position + 1.
    A word matches `key` if it is not filtered and lies in key.split() or in category_extension[key]."""
    ext = category_extension or {}
    words, key_of = {}, {}
    for idx in range(len(caption) - 1):
        word = word_of.get(int(caption[idx]))
        if word is None or word in word_filter:
            continue
        for key, cid in categories.items():
            if word in ext.get(key, ()) or word in key.split():
                if cid not in words:
                    words[cid], key_of[cid] = [], key
                if (idx + 1, word) not in words[cid]:
                    words[cid].append((idx + 1, word))
    return words, key_of


def normalise_box(box, resize_ratio, h, w):
    """EB:246-250 + numpy slicing `[box[1]:box[3], box[0]:box[2]]` -> (y0, y1, x0, x1) with 0 <= y0 <= y1 <= h."""
    nb = [int(box[i] * resize_ratio[i % 2]) for i in range(4)]
    y0, y1, _ = slice(nb[1], nb[3]).indices(h)
    x0, x1, _ = slice(nb[0], nb[2]).indices(w)
    return y0, max(y0, y1), x0, max(x0, x1)


def effective_thresholds(n_boxes, thresholds=THRESHOLDS, mode="reference"):
    """(n_boxes, K) thresholds each box of one word is scored at.  'reference': EB:191-208 zeroes map values <= thr in
    place inside the boxes x thresholds loop of a word, so every (box, threshold) sees the map cut at the running maximum
    of the thresholds applied so far (with the ten ascending values: the second and later boxes are scored at 0.9 ten
    times).  'independent': every box at every threshold."""
    thr = np.asarray(thresholds, dtype=np.float64)
    if mode == "independent":
        return np.tile(thr, (n_boxes, 1))
    if mode != "reference":
        raise ValueError("box_thresholds must be 'reference' or 'independent'")
    return np.maximum.accumulate(np.tile(thr, n_boxes)).reshape(n_boxes, len(thr)) if n_boxes else np.zeros((0, len(thr)))


def accumulate(store, scores, category_key, thresholds=THRESHOLDS):
    """EB:384-402: add one image's {cat_id: {str(thr): score}} to a score file's layout
    {cat_id: {'score': {str(thr): [...]}, 'category': name, 'count': n}}; returns `store`."""
    for cid, per in scores.items():
        if cid not in store:
            store[cid] = {"score": {str(t): [] for t in thresholds}, "category": category_key[cid], "count": 0.}
        store[cid]["count"] += 1
        for t in thresholds:
            store[cid]["score"][str(t)].append(per[str(t)])
    return store


def correctness_table(store, thresholds=THRESHOLDS):
    """EB:864-909: per threshold, (sum of all scores / sum of counts, std of the pooled score list)."""
    count = sum(v["count"] for v in store.values())
    out = {}
    for t in thresholds:
        pooled = [s for v in store.values() for s in v["score"][str(t)]]
        total = sum(np.array(v["score"][str(t)]).sum() for v in store.values())
        out[str(t)] = (total / count, float(np.std(np.array(pooled))))
    return out


class EvaluationBboxCOCO(object):
    """EB:38-272 on the engine."""
    _maps = ("lrp", "attention")

    def __init__(self, category_dict, max_caption_length, beam_size, rule, img_encode, explainer, category_extension=None,
                 word_filter=(), sign=-1, thresholds=THRESHOLDS, box_thresholds="reference"):
        if img_encode not in _ENCODERS:
            raise NotImplementedError("the img_encode is not valid, [vgg16, vgg19, resnet101]")
        if sign not in (1, -1):
            raise ValueError("sign must be +1 or -1")
        if not 1 <= len(thresholds) <= 16:
            raise ValueError("between 1 and 16 thresholds")
        effective_thresholds(1, thresholds, box_thresholds)                       # validates the mode
        self._preprocessor = explainer._preprocessor
        self._max_caption_length = max_caption_length
        self._beam_size = beam_size
        self._rule = rule
        self._category_dict = category_dict
        self._explainer = explainer
        self._img_encoder = img_encode
        self._color_conversion = "BGRtoRGB"
        g = int(round(np.sqrt(explainer.L)))             # 14 / 16 for VGG, 7 / 32 for ResNet-101 at 224 x 224
        self._reshape_size = (g, g)
        self._upscale = explainer._model.img_hw[0] // g
        self.category_extension = dict(category_extension or {})
        self.word_filter = tuple(word_filter)
        self.sign = int(sign)
        self.thresholds = tuple(thresholds)
        self.box_thresholds = box_thresholds

    # ---------------------------------------------------------------- public surface
    def evaluate(self, X, data):
        """EB:263-271: beam-search caption of X's image, then the scores of its object words."""
        img_filename = data[0].img_filename
        caption = self._explainer._beam_search(X, beam_size=self._beam_size)[0]
        return self.evaluate_batch(np.asarray(X[1], dtype=np.float32)[:1], [img_filename], [caption])[0]

    def evaluate_batch(self, images, img_filenames, captions=None):
        """images (B, H, W, 3) preprocessed; captions: one id list per image (None: beam search, like `evaluate`).
        Returns one `evaluate` result per image."""
        images = np.asarray(images, dtype=np.float32)
        B = len(images)
        if captions is None:
            res = self._explainer._beam_search((None, images), beam_size=self._beam_size)
            captions = [res[0]] if B == 1 else [r[0] for r in res]
        plans = [self._plan(list(map(int, c)), self._category_dict[f]) for c, f in zip(captions, img_filenames)]
        scores = self._score(images, captions, plans)
        out = []
        for b, (words, key_of, entries) in enumerate(plans):
            per = [{cid: {} for cid in words} for _ in self._maps]
            for (cid, _, _, _), row in zip(entries, scores[b]):
                for i in range(len(self._maps)):
                    d = per[i][cid]
                    for t, s in zip(self.thresholds, row[i]):
                        d.setdefault(str(t), 0)
                        if s > d[str(t)]:
                            d[str(t)] = float(s)
            out.append(tuple(per) + (key_of,))
        self._explainer.caption = None                   # the engine's caches now hold the last chunk
        self._explainer._state_cache = {}
        return out

    # ---------------------------------------------------------------- planning (host, no maps)
    def _plan(self, caption, category):
        words, key_of = match_categories(caption, self._preprocessor._word_of, category["categories"],
                                         self.category_extension, self.word_filter)
        h, w = self._explainer._model.img_hw
        entries = []                                     # (cat_id, t, box (y0, y1, x0, x1), thresholds (K,))
        for cid, ws in words.items():
            boxes = [normalise_box(bx, category["resize_ratio"], h, w) for bx in category["bbox"][cid]]
            thr = effective_thresholds(len(boxes), self.thresholds, self.box_thresholds)
            for t, _ in ws:
                entries += [(cid, t, bx, thr[j]) for j, bx in enumerate(boxes)]
        return words, key_of, entries

    # ---------------------------------------------------------------- scoring (device)
    def _score(self, images, captions, plans):
        """-> per image, per entry, (len(_maps), K) scores."""
        ex = self._explainer
        eng = ex._engine
        out = [[None] * len(p[2]) for p in plans]
        batched = self._batched(ex)
        step = eng.max_images if batched else 1
        for lo in range(0, len(images), step):
            hi = min(len(images), lo + step)
            units = sorted({(b - lo, t) for b in range(lo, hi) for (_, t, _, _) in plans[b][2]})
            if not units:
                continue
            if batched:
                eng.encode_images(images[lo:hi])
                eng.decoder_forward([list(map(int, c)) for c in captions[lo:hi]])
            else:
                ex._forward_beam_search((None, images[lo:hi]), captions[lo])
            for u0 in range(0, len(units), eng.max_tokens):
                chunk = units[u0:u0 + eng.max_tokens]
                maps = self._maps_of(chunk, images[lo:hi], batched)
                idx = {u: i for i, u in enumerate(chunk)}
                rows, where = [], []
                for b in range(lo, hi):
                    for e, (_, t, bx, thr) in enumerate(plans[b][2]):
                        if (b - lo, t) in idx:
                            rows.append(((idx[(b - lo, t)],) + tuple(bx), thr))
                            where.append((b, e))
                boxes = np.array([r[0] for r in rows], dtype=np.int32)
                thr = np.stack([r[1] for r in rows])
                thr32 = thr.astype(np.float32).astype(np.float64)     # numpy compares a float32 map with float32(thr)
                res = [_eng.eval_box_scores(m, boxes, thr32 if m.dtype == torch.float32 else thr) for m in maps]
                res = torch.stack(res, dim=1).cpu().numpy()      # (nb, len(_maps), K): the only device-to-host copy
                for (b, e), r in zip(where, res):
                    out[b][e] = r
        return out

    def _batched(self, ex):
        return getattr(ex, "_batched_cnn", True)

    def _maps_of(self, units, images, batched):
        ex = self._explainer
        eng = ex._engine
        ii, ts = [u[0] for u in units], [u[1] for u in units]
        g, up = self._reshape_size[0], self._upscale
        if batched:
            R, _, att, _ = eng.explain_tokens(ii, ts, want_attention=True)
            return [_eng.eval_relevance_maps(R, self.sign), _eng.eval_attention_maps(att, g, up, SIGMA)]
        R, att = [], []
        for t in ts:                                      # per word, host-side _explain_CNN (float64)
            r_feat, a = ex._explain_lstm_single_word_sequence(t)
            R.append(np.asarray(ex._explain_CNN(images[:1], r_feat))[0])
            att.append(np.asarray(a, dtype=np.float32))
        R = torch.as_tensor(np.stack(R)).to(eng.device)
        att = torch.as_tensor(np.stack(att)).to(eng.device)
        return [_eng.eval_relevance_maps(R, self.sign), _eng.eval_attention_maps(att, g, up, SIGMA)]


class EvaluationBboxCOCOBaseline(EvaluationBboxCOCO):
    """EB:273-358: the gradient baselines (decoder gradient -> CNN walk); no attention map.
    evaluate / evaluate_batch return (gradient_score, category_key) per image.

    device_gradcam=True (opt-in): a Guided Grad-CAM explainer takes the batched branch too — `max_images` images and
    `max_tokens` words per chain through LRPEngine.guided_gradcam (Grad-CAM in fp64 on the device, lrp_op_gradcam); its
    float64 maps are scored in float64 and only the scores come back.  The default keeps the per-word host path."""
    _maps = ("gradient",)

    def __init__(self, *args, **kwargs):
        self.device_gradcam = bool(kwargs.pop("device_gradcam", False))
        super(EvaluationBboxCOCOBaseline, self).__init__(*args, **kwargs)

    def _on_device_gradcam(self, ex):
        return self.device_gradcam and hasattr(ex, "grad_cam_device")

    def _batched(self, ex):
        return self._on_device_gradcam(ex) or getattr(ex, "_batched_cnn", True)

    def _maps_of(self, units, images, batched):
        ex = self._explainer
        eng = ex._engine
        ii, ts = [u[0] for u in units], [u[1] for u in units]
        if batched and self._on_device_gradcam(ex):
            return [_eng.eval_relevance_maps(eng.guided_gradcam(ii, ts), self.sign)]
        if batched:
            d, _ = eng.decoder_gradient(ii, ts, want_r_words=False)
            return [_eng.eval_relevance_maps(eng.cnn_walk(ii, d, ex._walk), self.sign)]
        R = [np.asarray(ex._explain_CNN(images[:1], ex._lstm_decoder_backward(t)))[0] for t in ts]
        return [_eng.eval_relevance_maps(torch.as_tensor(np.stack(R)).to(eng.device), self.sign)]
