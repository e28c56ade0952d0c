"""A fresh numpy restatement of the reference's bounding-box evaluation (evaluate_bbox.py, EB:), the checker of
tests/test_eval_bbox_host.py and tests/test_gpu_eval_bbox.py.  Literal where the reference's arithmetic matters: float32
where the reference is float32, and the boxes x thresholds loop zeroes the word's map IN PLACE."""
import numpy as np

from lrp_imagecaptioning_amd.postprocess import pyramid_expand

THRESHOLDS = [0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]


def project(x):
    """EB:62-71."""
    absmax = np.max(np.abs(x))
    if absmax == 0:
        return np.zeros(x.shape)
    x = 1.0 * x / absmax
    if np.sum(x < 0):
        x = (x + 1) / 2
    return x


def relevance_map(R, sign=-1):
    """EB:80-84 for one (1, H, W, 3) relevance in its own dtype -> (H, W)."""
    hm = R[:, :, :, ::-1]
    hm = sign * hm
    hm = np.maximum(hm, 0)
    hm = np.mean(hm, axis=-1)
    return project(hm)[0]


def attention_map(att, g, upscale, sigma=20):
    """EB:78 + :85 with the project's pyramid_expand restatement."""
    return project(pyramid_expand(np.asarray(att).reshape(g, g), upscale=upscale, sigma=sigma))


def overlap(bbox, relevance, threshold, f64=False):
    """EB:191-208, mutating `relevance`.  f64: the same threshold decisions (in the map's dtype), sums in float64."""
    bbox_mask = np.zeros(relevance.shape)
    bbox_mask[bbox[1]:bbox[3], bbox[0]:bbox[2]] = 1
    relevance_mask = relevance <= threshold
    if np.sum(relevance_mask > 0):
        relevance[relevance_mask] = 0
    total = np.sum(relevance, dtype=np.float64) if f64 else np.sum(relevance)
    if total == 0:
        return 0
    ratio = 1.0 * np.sum(np.multiply(bbox_mask, relevance), dtype=np.float64) / total
    return 1. if ratio > 1 else ratio


def word_scores(maps, boxes, resize_ratio, thresholds=THRESHOLDS, into=None, f64=False):
    """EB:239-261 for one word: `maps` (one or two maps, each a private copy the loop mutates), boxes in annotation units.
    Updates / returns [ {str(thr): max score} per map ]."""
    into = into if into is not None else [dict() for _ in maps]
    maps = [np.array(m, copy=True) for m in maps]
    for box in boxes:
        nb = [int(box[0] * resize_ratio[0]), int(box[1] * resize_ratio[1]), int(box[2] * resize_ratio[0]),
              int(box[3] * resize_ratio[1])]
        for thr in thresholds:
            for m, d in zip(maps, into):
                d.setdefault(str(thr), 0)
                s = overlap(nb, m, thr, f64)
                if s > d[str(thr)]:
                    d[str(thr)] = s
    return into


def box_scores_f64(maps, entries, thr):
    """float64 scores of (map, y0, y1, x0, x1) entries at per-entry thresholds, on the given maps (no mutation)."""
    out = np.zeros(np.asarray(thr).shape)
    for e, (m, y0, y1, x0, x1) in enumerate(entries):
        v = np.asarray(maps[m], dtype=np.float64)
        for k, t in enumerate(thr[e]):
            c = np.where(v > t, v, 0.0)
            tot = c.sum()
            r = 0.0 if tot == 0 else c[y0:y1, x0:x1].sum() / tot
            out[e, k] = min(r, 1.0)
    return out


def match(caption, word_of, categories, ext, word_filter):
    """EB:218-232 -> ({cat_id: set((t, word))}, {cat_id: key})."""
    words, key_of = {}, {}
    for idx in range(len(caption) - 1):
        word = word_of.get(caption[idx])
        for key in categories.keys():
            if key in ext.keys():
                if word not in word_filter and word in ext[key]:
                    if categories[key] not in words:
                        words[categories[key]] = set()
                        key_of[categories[key]] = key
                    words[categories[key]].add((idx + 1, word))
            if word is not None and word not in word_filter and word in key.split():
                if categories[key] not in words:
                    words[categories[key]] = set()
                    key_of[categories[key]] = key
                words[categories[key]].add((idx + 1, word))
    return words, key_of


def evaluate_image(explain_word, caption, word_of, category, ext, word_filter, n_maps, thresholds=THRESHOLDS, f64=True):
    """EB:210-261 with a given caption; explain_word(t) -> list of n_maps maps (host); f64: see overlap()."""
    words, key_of = match(caption, word_of, category["categories"], ext, word_filter)
    res = [dict() for _ in range(n_maps)]
    for cid, ws in words.items():
        per = [dict() for _ in range(n_maps)]
        for t, _ in sorted(ws):
            word_scores(explain_word(t), category["bbox"][cid], category["resize_ratio"], thresholds, per, f64)
        for i in range(n_maps):
            res[i][cid] = per[i]
    return tuple(res) + (key_of,)
