#!/usr/bin/env python3
"""Batched Guided Grad-CAM and word examination (engine.guided_gradcam, examination.py) on the full-size synthetic VGG16 +
adaptive-attention bundle: 8 images x their caption words, one process.
  (1) Guided Grad-CAM per heat-map through LRPEngine.guided_gradcam against the unchanged per-word `_explain_CNN` loop;
  (2) the lrp_op_gradcam launch alone at n = 320 (HIP events), cam only and with the gate;
  (3) word_statistics per word against the per-word WordExaminer._explain_single_word loop (+ numpy means)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import lrp_imagecaptioning_amd.explainers as EX
    from lrp_imagecaptioning_amd import engine as E
    from lrp_imagecaptioning_amd import examination as XW
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, images, vgg_weights
    B, V, reps = int(os.environ.get("B", 8)), 10000, int(os.environ.get("REPS", 5))
    rs = np.random.RandomState(0)
    w = vgg_weights(rs)
    w.update(adaptive_weights(rs, 196, 512, 512, 512, V))
    word_of = {i: "w%d" % i for i in range(1, V + 1)}
    X = images(rs, B)

    def explainer(cls):
        dp = EX.DatasetProviderStub(EX.CaptionPreprocessorStub(word_of=word_of))
        return getattr(EX, cls)(EX.CaptionModelSpec(w, vocab_size=V), None, dp, max_caption_length=20, max_images=B)

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    lrp = explainer("ExplainImgCaptioningAdaptiveAttention")
    beams = [c[0] for c in lrp._beam_search((None, X), beam_size=3)]
    # random weights caption an image with one word over and over: the captions are the beam lengths filled with
    # distinct random words instead (profiles/bbox_eval_bench.py)
    caps = [[int(i) for i in rs.choice(np.arange(3, V + 1), size=max(len(c) - 1, 4), replace=False)] + [1] for c in beams]
    units = [(b, t) for b, c in enumerate(caps) for t in range(1, len(c))]
    ii, ts = [u[0] for u in units], [u[1] for u in units]
    print("%d images, %d caption words" % (B, len(units)))

    # (1) Guided Grad-CAM: one chain for all words against the per-word loop
    gg = explainer("ExplainImgCaptioningAdaptiveAttentionGuidedGradcam")
    eng = gg._engine
    eng.encode_images(X)
    eng.decoder_forward(caps)
    eng.guided_gradcam(ii, ts)
    tb = np.median([wall(lambda: eng.guided_gradcam(ii, ts)) for _ in range(reps)])
    parts = {"decoder_gradient": lambda: eng.decoder_gradient(ii, ts, want_r_words=False)}
    d = parts["decoder_gradient"]()[0]
    parts["cnn_walk"] = lambda: eng.cnn_walk(ii, d, "guided_backprop")
    gb = parts["cnn_walk"]()
    feat = eng.get_features()
    parts["op_gradcam"] = lambda: E.op_gradcam(feat, ii, d, 14, 16, gb=gb)
    pt = {k: np.median([wall(fn) for _ in range(reps)]) for k, fn in parts.items()}
    nloop, tl = 0, 0.0
    for b in range(min(B, 2)):                              # the per-word loop of two images is enough for a rate
        gg._forward_beam_search((None, X[b:b + 1]), caps[b])
        gg._explain_CNN(X[b:b + 1], gg._lstm_decoder_backward(1))
        for t in range(1, len(caps[b])):
            tl += wall(lambda: gg._explain_CNN(X[b:b + 1], gg._lstm_decoder_backward(t)))
            nloop += 1
    print("guided grad-cam per heat-map: batched chain %.3f ms (%s); per-word _explain_CNN loop %.3f ms (%d words)" % (
        tb / len(units) * 1e3, ", ".join("%s %.3f" % (k, v / len(units) * 1e3) for k, v in pt.items()), tl / nloop * 1e3, nloop))

    # (2) the launch alone at n = 320
    n = 320
    rep = (n + len(units) - 1) // len(units)
    d320, gb320, i320 = d.repeat(rep, 1, 1)[:n].contiguous(), gb.repeat(rep, 1, 1, 1)[:n].contiguous(), (ii * rep)[:n]
    for name, fn in (("cam only", lambda: E.op_gradcam(feat, i320, d320, 14, 16)),
                     ("cam + gate", lambda: E.op_gradcam(feat, i320, d320, 14, 16, gb=gb320))):
        fn()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in evs:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        print("lrp_op_gradcam n = %d, %s: %.3f ms (median of %d, HIP events around the wrapper)" % (
            n, name, float(np.median([a.elapsed_time(b) for a, b in evs])), reps))
    del d320, gb320, gb, d

    # (3) word_statistics: three category words per caption
    names = ["img%d" % b for b in range(B)]
    pred = [" ".join(word_of[i] for i in c[:-1]) for c in caps]
    cats = sorted({word_of[i] for c in caps for i in c[:3]})
    true = [[pred[b]] if b % 2 else ["nothing"] for b in range(B)]
    for label, xm in (("LRP + attention + beta", XW.WordExaminer(lrp._model, None, lrp, 20, 3)),
                      ("guided grad-cam", XW.WordExaminerGuidedgradcam(gg._model, None, gg, 20, 3))):
        got = xm.word_statistics(X, names, pred, true, cats, captions=caps)
        nw = sum(len(v[xm._stats[0]]) for v in got.values())
        tb = np.median([wall(lambda: xm.word_statistics(X, names, pred, true, cats, captions=caps)) for _ in range(3)])

        def per_word(b):
            for cat, _ in got[names[b]][xm._stats[0]]:
                r = xm._explain_single_word((None, X[b:b + 1]), caps[b], XW.get_index(pred[b], cat))
                for m in (r if isinstance(r, tuple) else (np.abs(r),)):
                    np.mean(m)
        per_word(0)
        tw = sum(wall(lambda: per_word(b)) for b in range(min(B, 2)))
        n2 = sum(len(got[names[b]][xm._stats[0]]) for b in range(min(B, 2)))
        print("word_statistics (%s): %d words, %.3f ms per word (encoder + decoder forward included); per-word "
              "_explain_single_word loop %.3f ms per word (%d words)" % (label, nw, tb / nw * 1e3, tw / n2 * 1e3, n2))


if __name__ == "__main__":
    main()
