#!/usr/bin/env python3
"""The CAM family as word saliencies (saliency.py) at the bench configuration: full-size synthetic VGG16 + adaptive-attention
bundle at 224 x 224, one image of 10 words, max_images = 32, one process.
  gradient forms  lrp_op_cam, each mode next to lrp_op_gradcam on the same 10 units (HIP events, median), and a whole explain()
  Score-CAM       512 masked forwards + the image: a whole explain(), the parts of a chunk of 32 slots, the fold
  Ablation-CAM    512 ablated feature rows + the image, decoder forwards only: a whole explain(), the parts of a chunk
  the apply kernel as a stream, next to torch's device-to-device copy of the same rows
Writes profiles/cam_family.txt (or the path given as the first argument); what that file holds from its "Notes." line on
(hand-written) is kept as it is."""
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
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, images, vgg_weights
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cam_family.txt")
    M, T, V, reps = 32, 10, 10000, int(os.environ.get("REPS", 3))
    g, up, D = 14, 16, 512
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
        res = drv.explain(X, [cap])
        per = (", %3d chunks: %.3f ms per chunk, %.4f ms per slot" % (-(-rows // M), t * 1e3 / -(-rows // M), t * 1e3 / rows)) if rows else ""
        return "%-34s %8.1f ms per explain()%s, maps finite: %s" % (name, t * 1e3, per, bool(torch.isfinite(res["maps"]).all()))

    w = vgg_weights(rs)
    w.update(adaptive_weights(rs, 196, 512, 512, 512, V))
    ex = EX.ExplainImgCaptioningAdaptiveAttention(EX.CaptionModelSpec(w, vocab_size=V), None, dp, max_caption_length=20, max_images=M)
    eng = ex._engine
    dev = eng.device
    x_dev = torch.as_tensor(X).to(dev)
    lines = ["CAM family word saliency: VGG16 at 224 x 224 (L = 196, D = 512), adaptive attention, V = %d, one image of %d words, "
             "max_images = %d" % (V, T, M)]

    # Score-CAM and Ablation-CAM first: they run in the engine's default precision, the gradient forms switch it to fp32
    lines.append(explain_line("Score-CAM softmax, 512 masks", SAL.ScoreCAMSaliency(ex), 1 + D))
    lines.append(explain_line("Score-CAM linear, 513 masks", SAL.ScoreCAMSaliency(ex, "linear"), 2 + D))
    lines.append(explain_line("Ablation-CAM, 512 feature rows", SAL.AblationCAMSaliency(ex), 1 + D))

    i32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32)).to(dev)
    eng.encode_images(x_dev)
    feat = eng.get_features()
    idx, ks = i32([0] * M), i32(np.arange(M))
    fill = torch.zeros(3, dtype=torch.float32, device=dev)
    t_apply = events(lambda: E.op_scorecam_apply(x_dev, feat, idx, ks, g, up, fill))
    rows32 = E.op_scorecam_apply(x_dev, feat, idx, ks, g, up, fill)
    t_abl = events(lambda: E.op_feature_ablate(feat, idx, ks))
    frows32 = E.op_feature_ablate(feat, idx, ks)
    t_enc = events(lambda: eng.encode_images(rows32))
    t_set = events(lambda: eng.set_features(frows32))
    t_dec = events(lambda: eng.decoder_forward([cap] * M))
    slot, tt = i32(np.repeat(np.arange(M), T)), i32(np.tile(np.arange(1, T + 1), M))
    col = i32(np.tile(np.asarray(cap[:T]) - 1, M))
    t_sc = events(lambda: E.perturb_word_scores(eng, slot, tt, col))
    S = torch.randn((1, 2 + D, 16), dtype=torch.float64, device=dev)
    folds = ["%s %.3f ms" % (m, events(lambda: E.op_cam_weighted(S[:, :1 + D + (m == "linear")].contiguous(), feat, [0], g, up, m)))
             for m in ("softmax", "linear", "ablation")]
    lines += ["one chunk of %d slots, HIP events around each part (host wrapper included), median:" % M,
              "  apply   lrp_op_scorecam_apply %.3f ms | lrp_op_feature_ablate %.3f ms" % (t_apply, t_abl),
              "  enter   encode_images %.3f ms | set_features %.3f ms" % (t_enc, t_set),
              "  decoder decoder_forward %.3f ms (caption of %d words)" % (t_dec, T),
              "  scores  lrp_perturb_word_scores %.3f ms (%d units)" % (t_sc, M * T),
              "once per explain(), one image, T padded to 16 words: lrp_op_cam_weighted (16 maps of 224 x 224) " + ", ".join(folds)]

    lines.append("apply kernel as a stream (bytes read + written), next to torch's device-to-device copy of the same rows:")
    for n in (M, 256):
        idx_n, k_n = i32([0] * n), i32(np.arange(n) % D)
        src = x_dev.expand(n, -1, -1, -1).contiguous()
        dst = torch.empty_like(src)
        nbytes = 2.0 * n * 224 * 224 * 3 * 4
        for what, fn in (("lrp_op_scorecam_apply", lambda: E.op_scorecam_apply(x_dev, feat, idx_n, k_n, g, up, fill)),
                         ("copy_", lambda: dst.copy_(src))):
            t = events(fn, 9)
            lines.append("  n = %3d  %-21s %.4f ms  %.2f TB/s" % (n, what, t, nbytes / (t * 1e-3) / 1e12))

    # the gradient forms, on the same 10 units in the same run (fp32 forward, as the drivers run them)
    for guided in (False, True):
        for m in SAL.CAM_METHODS:
            lines.append(explain_line("%s%s, 10 units" % (m, " guided" if guided else ""), SAL.GradientCAMSaliency(ex, m, guided=guided), 0))
    eng.encode_images(x_dev)
    eng.decoder_forward([cap])
    ii, ts = [0] * T, list(range(1, T + 1))
    d, _ = eng.decoder_gradient(ii, ts, want_r_words=False)
    gb = eng.cnn_walk(ii, d, "guided_backprop")
    feat = eng.get_features()
    lines.append("lrp_op_cam on 10 units of one image, HIP events (host wrapper included), median of 9; cam only | with the gate:")
    lines.append("  %-22s %.4f ms | %.4f ms" % ("lrp_op_gradcam", events(lambda: E.op_gradcam(feat, ii, d, g, up), 9),
                                               events(lambda: E.op_gradcam(feat, ii, d, g, up, gb=gb), 9)))
    for m in SAL.CAM_METHODS:
        lines.append("  %-22s %.4f ms | %.4f ms" % ("lrp_op_cam " + m, events(lambda: E.op_cam(feat, ii, d, g, up, m), 9),
                                                   events(lambda: E.op_cam(feat, ii, d, g, up, m, gb=gb), 9)))
    same = torch.equal(E.op_cam(feat, ii, d, g, up, "gradcam"), E.op_gradcam(feat, ii, d, g, up))
    lines.append("  mode gradcam equals lrp_op_gradcam bit for bit on these units: %s" % same)
    t_grad = events(lambda: eng.decoder_gradient(ii, ts, want_r_words=False))
    t_walk = events(lambda: eng.cnn_walk(ii, d, "guided_backprop"))
    lines.append("  next to them: decoder_gradient %.3f ms, cnn_walk('guided_backprop') %.3f ms (10 units)" % (t_grad, t_walk))

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
