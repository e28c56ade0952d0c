#!/usr/bin/env python3
"""LIME and KernelSHAP word saliency (saliency.py) at the bench configuration: full-size synthetic VGG16 + adaptive-attention
bundle at 224 x 224, one image of 10 words, max_images = 32, one process; one line on ResNet-101 + grid-TD.
  LIME        1000 Bernoulli samples of a 7 x 7 grid (d = 49) + the image = 1001 slots
  KernelSHAP  2048 Shapley samples of the same grid + the image + the base = 2050 slots
Timed: a whole explain() (wall clock around a device synchronisation, median of REPS); the parts of a chunk of 32 slots alone
(HIP events, median); the draws, the fit and the map of the whole run.  Writes profiles/segment_saliency.txt (or the path given as
the first argument); what that file holds from its "Notes." line on (hand-written) is kept as it is."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import lrp_imagecaptioning_amd.explainers as EX
    from lrp_imagecaptioning_amd import engine as E
    from lrp_imagecaptioning_amd import saliency as SAL
    from lrp_imagecaptioning_amd.synthetic import RESNET101_STACKS, adaptive_weights, gridtd_weights, images, resnet_weights, vgg_weights
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "segment_saliency.txt")
    M, T, V, reps = 32, 10, 10000, int(os.environ.get("REPS", 3))
    n_lime, n_shap, cells = int(os.environ.get("LIME_SAMPLES", 1000)), int(os.environ.get("SHAP_SAMPLES", 2048)), 7
    d = cells * cells
    rs = np.random.RandomState(0)
    dp = EX.DatasetProviderStub(EX.CaptionPreprocessorStub())
    X = images(rs, 1)
    cap = [int(i) for i in rs.choice(np.arange(3, V + 1), size=T, replace=False)] + [1]

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    def events(fn, n=None):
        n = n or max(reps, 5)
        fn()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in evs:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return float(np.median([a.elapsed_time(b) for a, b in evs]))

    def explain_line(name, drv, rows):
        drv.explain(X, [cap])
        t = float(np.median([wall(lambda: drv.explain(X, [cap])) for _ in range(reps)]))
        chunks = -(-rows // M)
        res = drv.explain(X, [cap])
        return ("%-44s %5d slots, %3d chunks: %8.1f ms per explain() (%.3f ms per chunk, %.4f ms per slot), maps finite: %s, status %s"
                % (name, rows, chunks, t * 1e3, t * 1e3 / chunks, t * 1e3 / rows, bool(torch.isfinite(res["maps"]).all()),
                   res["status"].tolist()))

    w = vgg_weights(rs)
    w.update(adaptive_weights(rs, 196, 512, 512, 512, V))
    ex = EX.ExplainImgCaptioningAdaptiveAttention(EX.CaptionModelSpec(w, vocab_size=V), None, dp, max_caption_length=20, max_images=M)
    eng = ex._engine
    dev = eng.device
    x_dev = torch.as_tensor(X).to(dev)
    lines = ["LIME and KernelSHAP word saliency: VGG16 at 224 x 224, adaptive attention, V = %d, one image of %d words, max_images = %d, "
             "%d x %d grid (d = %d)" % (V, T, M, cells, cells, d)]
    lines.append(explain_line("LIME %d samples, p = 0.5, ridge 1" % n_lime, SAL.LIMESaliency(ex, n_lime, cells=cells, score="logp"), 1 + n_lime))
    lines.append(explain_line("KernelSHAP %d samples, ridge 0" % n_shap, SAL.KernelSHAPSaliency(ex, n_shap, cells=cells, score="logp"),
                              2 + n_shap))

    # one chunk of 32 slots, part by part
    i32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32)).to(dev)
    lab = torch.as_tensor(SAL.grid_segments(224, 224, cells)).to(dev).unsqueeze(0).contiguous()
    idx = i32([0] * M)
    fill = torch.zeros(3, dtype=torch.float32, device=dev)
    bits32 = E.op_segment_draws([0] * M, np.arange(M), d, "bernoulli", 0.5, 0, device=dev)
    t_apply = events(lambda: E.op_segment_apply(x_dev, idx, bits32, lab, d, fill))
    rows32 = E.op_segment_apply(x_dev, idx, bits32, lab, d, fill)
    t_enc = events(lambda: eng.encode_images(rows32))
    t_dec = events(lambda: eng.decoder_forward([cap] * M))
    slot, tt = i32(np.repeat(np.arange(M), T)), i32(np.tile(np.arange(1, T + 1), M))
    col = i32(np.tile(np.asarray(cap[:T]) - 1, M))
    t_sc = events(lambda: E.perturb_word_scores(eng, slot, tt, col))
    lines += ["one chunk of %d slots, HIP events around each part (host wrapper included), median:" % M,
              "  apply   lrp_op_segment_apply %.3f ms" % t_apply,
              "  encode  encode_images %.3f ms" % t_enc,
              "  decoder decoder_forward %.3f ms (caption of %d words)" % (t_dec, T),
              "  scores  lrp_perturb_word_scores %.3f ms (%d units)" % (t_sc, M * T)]

    # once per run: the draws, the fit (T padded to 16 words as the driver pads it) and the map
    lines.append("once per explain(), one image, T padded to 16 words:")
    for name, mode, K, ridge, shap in (("LIME", "bernoulli", n_lime, 1.0, False), ("KernelSHAP", "shapley", n_shap, 0.0, True)):
        t_draw = events(lambda: E.op_segment_draws([0] * K, np.arange(K), d, mode, 0.5, 0, device=dev))
        bits = E.op_segment_draws([0] * K, np.arange(K), d, mode, 0.5, 0, device=dev).view(1, K, 4)
        y = torch.randn((1, K, 16), dtype=torch.float64, device=dev)
        delta = torch.randn((1, 16), dtype=torch.float64, device=dev) if shap else None
        wtab = np.ones(d + 1)
        if shap:
            wtab[0] = wtab[d] = 0.0
        else:
            wtab = SAL.lime_weights(d, 0.25)
        wt = torch.as_tensor(wtab).to(dev)
        t_fit = events(lambda: E.op_segment_fit(bits, wt, y, d, ridge, delta))
        phi, _, status = E.op_segment_fit(bits, wt, y, d, ridge, delta)
        t_map = events(lambda: E.op_segment_map(phi, lab, d))
        lines.append("  %-10s draws lrp_op_segment_draws %d rows: %.3f ms | fit lrp_op_segment_fit K = %d, d = %d, 16 words: %.3f ms (status %s) | "
                     "map lrp_op_segment_map: %.3f ms" % (name, K, t_draw, K, d, t_fit, status.tolist(), t_map))
    K, dmax = 2048, E.SEG_MAX_D
    bits = E.op_segment_draws([0] * K, np.arange(K), dmax, "bernoulli", 0.5, 0, device=dev).view(1, K, 4)
    y = torch.randn((1, K, 16), dtype=torch.float64, device=dev)
    t_fit = events(lambda: E.op_segment_fit(bits, SAL.lime_weights(dmax, 0.25), y, dmax, 1.0))
    lines.append("  the largest fit: LIME form, K = %d, d = %d, 16 words: %.3f ms" % (K, dmax, t_fit))

    # the apply kernel as a stream
    lines.append("apply kernel as a stream (bytes read + written), next to torch's device-to-device copy of the same rows:")
    for n in (M, 256):
        idx_n = i32([0] * n)
        b_n = E.op_segment_draws([0] * n, np.arange(n), d, "bernoulli", 0.5, 0, device=dev)
        src = x_dev.expand(n, -1, -1, -1).contiguous()
        dst = torch.empty_like(src)
        nbytes = 2.0 * n * 224 * 224 * 3 * 4
        for what, fn in (("lrp_op_segment_apply", lambda: E.op_segment_apply(x_dev, idx_n, b_n, lab, d, fill)), ("copy_", lambda: dst.copy_(src))):
            t = events(fn, 9)
            lines.append("  n = %3d  %-21s %.4f ms  %.2f TB/s" % (n, what, t, nbytes / (t * 1e-3) / 1e12))
    del ex, eng
    torch.cuda.empty_cache()

    # ResNet-101 + grid-TD
    rs = np.random.RandomState(0)
    w = resnet_weights(rs)
    w.update(gridtd_weights(rs, 49, 2048, 512, 512, V))
    spec = EX.CaptionModelSpec(w, img_encoder="resnet101", hidden_dim=512, embedding_dim=512, L=49, D=2048, vocab_size=V,
                               img_hw=(224, 224), resnet={"stem": 64, "stacks": RESNET101_STACKS})
    exr = EX.ExplainImgCaptioningGridTDModel(spec, None, dp, max_caption_length=20, max_images=M)
    lines.append("ResNet-101 at 224 x 224, grid-TD decoder, the same image and caption:")
    lines.append(explain_line("LIME %d samples, p = 0.5, ridge 1" % n_lime, SAL.LIMESaliency(exr, n_lime, cells=cells, score="logp"), 1 + n_lime))

    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    notes = ""
    if os.path.exists(out_path):
        with open(out_path) as f:
            old = f.read()
        notes = old[old.find("\nNotes."):] if "\nNotes." in old else ""
    with open(out_path, "w") as f:
        f.write(text + notes)


if __name__ == "__main__":
    main()
