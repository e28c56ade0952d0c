#!/usr/bin/env python3
"""ResNet-101 encoder walks in LRP_PREC_FP32 on one handle: n = 320 heads over 32 images (config 4's shape), the LRP walk
against the gradient baselines (lrp_cnn_walk GRADIENT / INPUT_X_GRADIENT / GUIDED_BACKPROP).  ms per call, median of REPS
timed calls after a warm-up (the first gradient walk also packs the BN-scaled weights: reported apart)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import RESNET101_STACKS, images, resnet_weights
    B, T, reps = int(os.environ.get("B", 32)), 10, int(os.environ.get("REPS", 5))
    rs = np.random.RandomState(0)
    w = resnet_weights(rs)
    eng = LRPEngine(decoder="gridtd", img_hw=(224, 224), L=49, D=2048, H=32, E=32, V=50, max_images=B, max_tokens=B * T,
                    max_caption_len=T + 1, resnet={"stem": 64, "stacks": RESNET101_STACKS})
    eng.set_weights(w)
    eng.set_precision("fp32")
    X = torch.as_tensor(images(rs, B)).cuda()
    ws0 = eng.workspace_bytes
    eng.encode_images(X)
    ws1 = eng.workspace_bytes
    idx = [b for b in range(B) for _ in range(T)]
    head = torch.randn((B * T, 49, 2048), device="cuda")
    out = torch.empty((B * T, 224, 224, 3), dtype=torch.float32, device="cuda")

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    first = timed(lambda: eng.cnn_walk(idx, head, "gradient", out=out))       # includes the one-off weight packing
    ws2 = eng.workspace_bytes
    res = {}
    for walk in ("lrp", "gradient", "input_x_gradient", "guided_backprop"):
        eng.cnn_walk(idx, head, walk, out=out)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            eng.cnn_walk(idx, head, walk, out=out)
            b.record()
        torch.cuda.synchronize()
        res[walk] = float(np.median([a.elapsed_time(b) for a, b in ev]))
        assert torch.isfinite(out).all()
    print("ResNet-101 walks, fp32 mode, %d heads over %d images, ms per call (median of %d): %s" % (
        B * T, B, reps, ", ".join("%s %.2f" % kv for kv in res.items())))
    print("first gradient walk (packs the BN-scaled weights) %.2f ms; workspace: handle %.2f GB, + ReLU masks %.3f GB "
          "(first fp32 encode), + gradient weights %.3f GB (first gradient walk)" % (first, ws0 / 1e9, (ws1 - ws0) / 1e9, (ws2 - ws1) / 1e9))


if __name__ == "__main__":
    main()
