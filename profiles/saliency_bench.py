#!/usr/bin/env python3
"""Occlusion and RISE word saliency (saliency.py) at the bench configuration: full-size synthetic VGG16 + adaptive-attention
bundle at 224 x 224, one image of 10 words, max_images = 32, one process.
  occlusion  16 x 16 window, stride 8: 27 x 27 = 729 windows + the unoccluded row = 730 slots, 23 chunks
  RISE       4000 masks of a 9 x 9 grid (s = 8, p = 0.5) + the unmasked row = 4001 slots, 126 chunks
Timed: a whole explain() (wall clock around a device synchronisation, median of REPS); the four parts of a chunk of 32 slots
alone (HIP events, median of REPS); the two map kernels; the apply kernels as streams (bytes read + written per second) next to a
device-to-device copy of the same rows.  Writes profiles/saliency.txt (or the path given as the first argument); what that file
holds from its "Notes." line on (the hand-written notes and the bench A/B against the parent commit) is kept as it is."""
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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "saliency.txt")
    M, T, V, reps = 32, 10, 10000, int(os.environ.get("REPS", 3))
    K, s, p = int(os.environ.get("MASKS", 4000)), 8, 0.5
    window, stride = (16, 16), (8, 8)
    rs = np.random.RandomState(0)
    w = vgg_weights(rs)
    w.update(adaptive_weights(rs, 196, 512, 512, 512, V))
    dp = EX.DatasetProviderStub(EX.CaptionPreprocessorStub())
    ex = EX.ExplainImgCaptioningAdaptiveAttention(EX.CaptionModelSpec(w, vocab_size=V), None, dp, max_caption_length=20, max_images=M)
    eng = ex._engine
    dev = eng.device
    X = images(rs, 1)
    cap = [int(i) for i in rs.choice(np.arange(3, V + 1), size=T, replace=False)] + [1]
    x_dev = torch.as_tensor(X).to(dev)

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

    occ = SAL.OcclusionSaliency(ex, window, stride, score="logp")
    rise = SAL.RISESaliency(ex, K, s=s, p=p, seed=0, score="logp")
    Hn, Wn = E.occlusion_geometry(224, 224, window, stride)
    lines = ["occlusion and RISE word saliency: VGG16 at 224 x 224, adaptive attention, V = %d, one image of %d words, max_images = %d"
             % (V, T, M)]
    for name, drv, rows in (("occlusion %dx%d stride %d" % (window[0], window[1], stride[0]), occ, 1 + Hn * Wn),
                            ("RISE %d masks, s = %d, p = %g" % (K, s, p), rise, 1 + K)):
        drv.explain(X, [cap])
        t = float(np.median([wall(lambda: drv.explain(X, [cap])) for _ in range(reps)]))
        chunks = -(-rows // M)
        lines.append("%-32s %5d slots, %3d chunks: %8.1f ms per explain() (%.3f ms per chunk, %.4f ms per slot), maps finite: %s"
                     % (name, rows, chunks, t * 1e3, t * 1e3 / chunks, t * 1e3 / rows,
                        bool(torch.isfinite(drv.explain(X, [cap])["maps"]).all())))

    # one chunk of 32 slots, part by part
    i32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32)).to(dev)
    idx, ks = i32([0] * M), i32(np.arange(M))
    grid, shift = E.op_rise_grids([0] * M, np.arange(M), s, p, 0, 224, 224, device=dev)
    fill = torch.zeros(3, dtype=torch.float32, device=dev)
    t_occ = events(lambda: E.op_occlude(x_dev, idx, ks, window, stride, fill))
    t_rise = events(lambda: E.op_rise_apply(x_dev, idx, grid, shift, s, fill))
    t_grids = events(lambda: E.op_rise_grids([0] * M, np.arange(M), s, p, 0, 224, 224, device=dev))
    rows32 = E.op_rise_apply(x_dev, idx, grid, shift, s, fill)
    t_enc = events(lambda: eng.encode_images(rows32))
    t_dec = events(lambda: eng.decoder_forward([cap] * M))
    slot, tt = i32(np.repeat(np.arange(M), T)), i32(np.tile(np.arange(1, T + 1), M))
    col = i32(np.tile(np.asarray(cap[:T]) - 1, M))
    t_sc = events(lambda: E.perturb_word_scores(eng, slot, tt, col))
    lines += ["one chunk of %d slots, HIP events around each part (host wrapper included), median:" % M,
              "  apply   lrp_op_occlude %.3f ms | lrp_op_rise_apply %.3f ms (lrp_op_rise_grids for the whole run: %.3f ms per %d rows)"
              % (t_occ, t_rise, t_grids, M),
              "  encode  encode_images %.3f ms" % t_enc,
              "  decoder decoder_forward %.3f ms (caption of %d words)" % (t_dec, T),
              "  scores  lrp_perturb_word_scores %.3f ms (%d units)" % (t_sc, M * T)]

    # the map kernels
    sc_o = torch.randn((1, 1 + Hn * Wn, 16), dtype=torch.float64, device=dev)
    t_om = events(lambda: E.op_occlusion_map(sc_o, 224, 224, window, stride))
    gK, sK = E.op_rise_grids([0] * K, np.arange(K), s, p, 0, 224, 224, device=dev)
    sc_r = torch.randn((1, K, 16), dtype=torch.float64, device=dev)
    t_rm = events(lambda: E.op_rise_map(sc_r, gK.view(1, K, -1), sK.view(1, K, 2), 224, 224, s, p))
    lines += ["map kernels, one image, T padded to 16 words:",
              "  lrp_op_occlusion_map %d windows: %.3f ms" % (Hn * Wn, t_om),
              "  lrp_op_rise_map      %d masks:   %.3f ms" % (K, t_rm)]

    # the apply kernels as streams
    lines.append("apply kernels as streams (bytes read + written), next to torch's device-to-device copy of the same rows:")
    for n in (M, 256):
        idx, ks = i32([0] * n), i32(np.arange(n) % (Hn * Wn))
        g, sh = E.op_rise_grids([0] * n, np.arange(n), s, p, 0, 224, 224, device=dev)
        src = x_dev.expand(n, -1, -1, -1).contiguous()
        dst = torch.empty_like(src)
        nbytes = 2.0 * n * 224 * 224 * 3 * 4
        for what, fn in (("lrp_op_occlude", lambda: E.op_occlude(x_dev, idx, ks, window, stride, fill)),
                         ("lrp_op_rise_apply", lambda: E.op_rise_apply(x_dev, idx, g, sh, s, fill)),
                         ("copy_", lambda: dst.copy_(src))):
            t = events(fn, 9)
            lines.append("  n = %3d  %-18s %.4f ms  %.2f TB/s" % (n, what, t, nbytes / (t * 1e-3) / 1e12))
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
