#!/usr/bin/env python3
"""Bounding-box correctness evaluation (evaluation.py) on the full-size synthetic VGG16 + adaptive-attention bundle:
32 images, captions of the beam-3 search's lengths, 3 object words per caption with 2 boxes each.
  (1) GPU time of the three lrp_eval_* launches for the batch (median of REPS, HIP events);
  (2) evaluate_batch images/s against one evaluate_batch call per image (same captions, no beam search in either);
  (3) the host numpy work the reference does for the same words: map preparation, pyramid_expand, ten-threshold scores."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import lrp_imagecaptioning_amd.explainers as EX
    from lrp_imagecaptioning_amd import engine as E
    from lrp_imagecaptioning_amd import evaluation as EV
    from lrp_imagecaptioning_amd.postprocess import pyramid_expand
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, images, vgg_weights
    B, V, reps = int(os.environ.get("B", 32)), 10000, int(os.environ.get("REPS", 5))
    rs = np.random.RandomState(0)
    w = vgg_weights(rs)
    w.update(adaptive_weights(rs, 196, 512, 512, 512, V))
    word_of = {i: "w%d" % i for i in range(1, V + 1)}
    dp = EX.DatasetProviderStub(EX.CaptionPreprocessorStub(word_of=word_of))
    ex = EX.ExplainImgCaptioningAdaptiveAttention(EX.CaptionModelSpec(w, vocab_size=V), None, dp, max_caption_length=20,
                                                  max_images=B)
    X = images(rs, B)
    beams = [c[0] for c in ex._beam_search((None, X), beam_size=3)]      # timed path's input: the beam-3 search runs
    # random weights caption an image with one word over and over, which would make every position an object word: the
    # scored captions are the beam lengths filled with distinct random words instead
    caps = [list(rs.choice(np.arange(3, V + 1), size=max(len(c) - 1, 4), replace=False)) + [1] for c in beams]
    cats = {}
    for b, c in enumerate(caps):                        # up to 3 distinct caption words are "objects", 2 boxes each
        ws = list(dict.fromkeys(c[:-1]))[:3]
        cats["img%d" % b] = {"categories": {"w%d" % i: 100 + j for j, i in enumerate(ws)},
                             "bbox": {100 + j: [list(rs.uniform(0, 500, 2)) + list(rs.uniform(300, 640, 2)) for _ in range(2)]
                                      for j in range(len(ws))},
                             "resize_ratio": (224 / 640., 224 / 480.)}
    names = list(cats)
    ev = EV.EvaluationBboxCOCO(cats, 20, 3, "eps", "vgg16", ex)
    plans = [ev._plan(c, cats[f]) for c, f in zip(caps, names)]
    nw = sum(len({e[1] for e in p[2]}) for p in plans)
    nb = sum(len(p[2]) for p in plans)

    # (1) the three launches on this batch's maps
    ex._engine.encode_images(X)
    ex._engine.decoder_forward(caps)
    units = sorted({(b, e[1]) for b, p in enumerate(plans) for e in p[2]})
    idx = {u: i for i, u in enumerate(units)}
    R, _, att, _ = ex._engine.explain_tokens([u[0] for u in units], [u[1] for u in units], want_attention=True)
    ent = np.array([(idx[(b, e[1])],) + tuple(e[2]) for b, p in enumerate(plans) for e in p[2]], dtype=np.int32)
    thr = np.concatenate([np.stack([e[3] for e in p[2]]) for p in plans if p[2]]).astype(np.float32).astype(np.float64)
    ent_d, thr_d = torch.as_tensor(ent).cuda(), torch.as_tensor(thr).cuda()
    calls = {"relevance_maps": lambda: E.eval_relevance_maps(R, -1),
             "attention_maps": lambda: E.eval_attention_maps(att, 14, 16),
             "box_scores_x2": None}
    rm, am = calls["relevance_maps"](), calls["attention_maps"]()
    calls["box_scores_x2"] = lambda: (E.eval_box_scores(rm, ent_d, thr_d), E.eval_box_scores(am, ent_d, thr_d))
    res = {}
    for k, fn in calls.items():
        fn()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in evs:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        res[k] = float(np.median([a.elapsed_time(b) for a, b in evs]))
    print("batch: %d images, %d object words, %d (word, box) entries; GPU ms (median of %d): %s; total %.3f ms" % (
        B, nw, nb, reps, ", ".join("%s %.3f" % kv for kv in res.items()), sum(res.values())))

    # (2) batched against per image
    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t
    ev.evaluate_batch(X, names, caps)
    tb = np.median([wall(lambda: ev.evaluate_batch(X, names, caps)) for _ in range(3)])
    t1 = wall(lambda: [ev.evaluate_batch(X[b:b + 1], [names[b]], [caps[b]]) for b in range(B)])
    print("evaluate_batch: %.1f images/s (%.1f ms per batch); one call per image: %.1f images/s" % (B / tb, tb * 1e3, B / t1))

    # (3) the reference's host work on the same words (one core of this host)
    Rh, ah = R[:8].cpu().numpy(), att[:8].cpu().numpy()

    def host_word(i):
        hm = np.mean(np.maximum(-1 * Rh[i:i + 1, :, :, ::-1], 0), axis=-1)
        hm = hm / (np.max(np.abs(hm)) or 1.0)
        a = pyramid_expand(ah[i].reshape(14, 14), upscale=16, sigma=20)
        a = a / np.max(np.abs(a))
        for m in (hm[0], a):
            m = m.copy()
            for _ in range(2):
                mask = np.zeros(m.shape)
                mask[20:180, 30:200] = 1
                for t in EV.THRESHOLDS:
                    m[m <= t] = 0
                    tot = np.sum(m)
                    _ = np.sum(mask * m) / tot if tot else 0
    th = wall(lambda: [host_word(i) for i in range(8)]) / 8
    print("host numpy, per word with 2 boxes (map preparation + pyramid_expand + 2 x 2 x 10 scores): %.1f ms; "
          "for this batch %.2f s" % (th * 1e3, th * nw))


if __name__ == "__main__":
    main()
