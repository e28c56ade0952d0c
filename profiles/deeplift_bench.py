#!/usr/bin/env python3
"""The DeepLIFT walk (lrp_set_deeplift_reference, LRP_WALK_DEEPLIFT) on an MI355X: what profiles/deeplift.txt records.

VGG16, 224 x 224, 32 images x 10 tokens (320 maps), LRP_PREC_FP32, one engine, one process:
  * encode ms without a reference and under mode 1 / mode 2 (behind the unchanged forward: one gate pass per layer; the first encode
    after a reference is set also runs the reference's own forward, which the timed repetitions do not repeat)
  * lrp_cnn_walk ms (HIP events around the call, median of REPS) for the fp32 `gradient` and `lrp` walks and the DeepLIFT walk in
    mode 1 (approximate_gradient=False, one chain) and mode 2 (True: two chains and the select)
  * lrp_workspace_bytes before a reference, with mode 1, with mode 2
  * per launch of the DeepLIFT walks (lrp_profile_records): the convs' ms, and for the streaming kernels (head, combine, final) ms
    next to the bytes they move, computed here from the shapes, as GB/s and as a share of the 6.3 TB/s a float4 copy reaches

Usage (GPU box, repository root): python profiles/deeplift_bench.py"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 3
COPY_TBS = 6.3


def _event_ms(fn, reps=REPS):
    import torch
    fn(); torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def stream_bytes(cfg, hw, n, chains):
    """bytes of the walk's streaming kernels, launch order (head first): float32 reads + writes per kernel, every row counted
    (a token reads its image's gate and kept input once; the reference's input is one image's worth and not counted)"""
    geo = []
    h = hw
    for name, cin, cout, pool in cfg:
        geo.append((name, cin, cout, h, pool))
        h = h // 2 if pool else h
    name, cin, cout, h, _ = geo[-1]
    per = h * h * cout
    out = [("head -> " + name, 4 * n * per * (1 + 1 + chains))]                       # head, gate, chains out
    for li in range(len(geo) - 1, 0, -1):
        name, cin, cout, h, _ = geo[li]
        below, up = geo[li - 1][0], 4 if geo[li - 1][4] else 1
        per = h * h * cin
        out.append(("%s -> %s%s" % (name, below, " (pool)" if up == 4 else ""), 4 * n * per * (chains + 1 + up + chains * up)))   # conv out, x, gate, chains out
    per = hw * hw * 3
    out.append(("image", 4 * n * per * (chains + 1 + 1)))
    return out


def main():
    import numpy as np
    import torch
    from bench import synth_weights
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import VGG16_CFG, images
    B, T, V = 32, 10, 10000
    n = B * T
    rs = np.random.RandomState(1)
    X = torch.as_tensor(images(rs, B)).cuda()
    idx = [b for b in range(B) for _ in range(T)]
    g = torch.Generator(device="cuda").manual_seed(2)
    head = torch.randn((n, 196, 512), device="cuda", generator=g)
    eng = LRPEngine(decoder="adaptive", V=V, max_images=B, max_tokens=n, max_caption_len=T + 1)
    eng.set_weights(synth_weights(0, V))
    eng.set_precision("fp32")
    out = torch.empty((n, 224, 224, 3), dtype=torch.float32, device="cuda")
    print("== VGG16 224 x 224, %d images x %d tokens (%d maps), LRP_PREC_FP32; ms, median of %d" % (B, T, n, REPS))
    ws0 = eng.workspace_bytes
    enc0 = _event_ms(lambda: eng.encode_images(X))
    base = {}
    for walk in ("gradient", "lrp"):
        base[walk] = _event_ms(lambda: eng.cnn_walk(idx, head, walk, out=out))
        eng.profile_enable(True)
        eng.cnn_walk(idx, head, walk, out=out); torch.cuda.synchronize()
        rec = [m for m, _ in eng.profile_records()]
        eng.profile_enable(False)
        base[walk + "_conv"] = sum(rec)
        print("no reference  encode %7.2f ms  %-8s walk %7.2f ms  (its %d launches %7.2f ms)  workspace %.2f GB" % (
            enc0, walk, base[walk], len(rec), sum(rec), ws0 / 1e9), flush=True)
    for mode, approx in ((1, False), (2, True)):
        eng.set_deeplift_reference(0.0, approx)
        eng.encode_images(X)                                 # (with the reference's forward)
        enc = _event_ms(lambda: eng.encode_images(X))
        ms = _event_ms(lambda: eng.cnn_walk(idx, head, "deeplift", out=out))
        finite = bool(torch.isfinite(out).all())
        eng.profile_enable(True)
        eng.cnn_walk(idx, head, "deeplift", out=out); torch.cuda.synchronize()
        rec = eng.profile_records()
        eng.profile_enable(False)
        conv = [m for m, f in rec if f > 0]
        stream = [m for m, f in rec if f == 0]
        print("mode %d        encode %7.2f ms (x%.2f)  deeplift walk %7.2f ms (x%.2f of gradient, x%.2f of lrp)  convs %7.2f ms (x%.2f of gradient's)  "
              "streaming kernels %6.2f ms  workspace %.2f GB (+%.2f)  finite %s" % (
                  mode, enc, enc / enc0, ms, ms / base["gradient"], ms / base["lrp"], sum(conv), sum(conv) / base["gradient_conv"], sum(stream),
                  eng.workspace_bytes / 1e9, (eng.workspace_bytes - ws0) / 1e9, finite), flush=True)
        print("       convs, top first: " + " ".join("%.2f" % m for m in conv))
        sb = stream_bytes(VGG16_CFG, 224, n, mode)
        assert len(sb) == len(stream), (len(sb), len(stream))
        for (name, nbytes), m in zip(sb, stream):
            print("       %-36s %6.3f ms  %6.2f GB  %5.2f TB/s  (%3.0f %% of a float4 copy's %.1f TB/s)" % (
                name, m, nbytes / 1e9, nbytes / m / 1e9, 100 * nbytes / m / 1e9 / COPY_TBS, COPY_TBS))
        print("       streaming kernels: %.1f %% of the walk" % (100 * sum(stream) / ms), flush=True)


if __name__ == "__main__":
    main()
