#!/usr/bin/env python3
"""SmoothGrad on the device against the host loop, and the Deconvnet walk next to guided backprop, on an MI355X: what
profiles/gradient_family.txt records.

  smoothgrad   VGG16 at 224 x 224, 4 images, n = 64 samples, max_batch = 32, exact fp32:
                 device   analyzer.SmoothGrad(...).analyze([X, head])      (LRPEngine.cnn_walk_augmented: augment, encode, walk and
                          the reduction on the device; the 4 maps come back)
                 host     the loop a user writes without it: numpy noise, analyzer.Gradient(...).analyze per chunk of 32 samples,
                          numpy mean (every sample goes up and every map comes down over PCIe)
               same process, alternating, median of REPS wall-clock times (time.perf_counter around the call, device idle before
               and after)
  walks        ms per lrp_cnn_walk (HIP events, median of REPS) for guided_backprop and deconvnet on the same encode: VGG16,
               32 tokens of 4 images; ResNet-101, 8 tokens of 4 images

Usage (GPU box, repository root): python profiles/gradient_family_bench.py"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 5


def _event_ms(fn, reps=REPS):
    import torch
    fn(); torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def smoothgrad():
    import numpy as np
    import torch
    from lrp_imagecaptioning_amd import analyzer as A
    from lrp_imagecaptioning_amd.synthetic import VGG16_CFG, vgg_weights
    rs = np.random.RandomState(0)
    w = vgg_weights(rs, VGG16_CFG, bias_std=0.05)
    spec = A.ImageModelSpec(w)
    B, n, mb, sigma = 4, 64, 32, 10.0
    X = rs.uniform(-120, 130, size=(B, 224, 224, 3)).astype(np.float32)
    head = rs.standard_normal((B, 14, 14, 512)).astype(np.float32)
    dev = A.SmoothGrad(spec, augment_by_n=n, noise_scale=sigma, seed=1, max_batch=mb)
    grad = A.Gradient(spec, max_batch=mb)

    def host_loop():
        noise = np.random.RandomState(1)
        S = np.repeat(X, n, axis=0)
        Hd = np.repeat(head, n, axis=0)
        maps = np.empty_like(S)
        for lo in range(0, B * n, mb):
            s = S[lo:lo + mb] + noise.normal(0, sigma, size=S[lo:lo + mb].shape).astype(np.float32)
            maps[lo:lo + mb] = grad.analyze([s, Hd[lo:lo + mb]])
        return maps.reshape((B, n) + maps.shape[1:]).mean(axis=1)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    timed(lambda: dev.analyze([X, head])); timed(host_loop)             # warm-up of both
    td, th = [], []
    for _ in range(REPS):
        a, od = timed(lambda: dev.analyze([X, head]))
        b, oh = timed(host_loop)
        td.append(a); th.append(b)
    md, mh = statistics.median(td), statistics.median(th)
    print("== SmoothGrad, VGG16 224 x 224, %d images x %d samples, max_batch %d, fp32; wall-clock ms, median of %d, alternating" % (B, n, mb, REPS))
    print("device route   %.1f ms   (%s)" % (md, " ".join("%.1f" % v for v in td)))
    print("host loop      %.1f ms   (%s)" % (mh, " ".join("%.1f" % v for v in th)))
    print("host / device  %.2f x" % (mh / md))
    # the two draw different noise (numpy's generator on the host, Philox on the device): the maps agree as two 64-sample estimates do
    print("relative L1 between the two estimates (different noise): %.3f" % (np.abs(od - oh).sum() / np.abs(oh).sum()))


def walks():
    import numpy as np
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import RESNET101_STACKS, VGG16_CFG, resnet_weights, vgg_weights
    rs = np.random.RandomState(0)
    print("== lrp_cnn_walk, ms per call (HIP events, median of %d), fp32 encode" % REPS)
    for name, ntok in (("vgg16", 32), ("resnet101", 8)):
        if name == "vgg16":
            eng = LRPEngine(decoder="adaptive", cnn_cfg=VGG16_CFG, L=196, D=512, H=8, E=8, V=4, max_images=4, max_tokens=ntok, max_caption_len=2)
            eng.set_weights(vgg_weights(rs, VGG16_CFG, bias_std=0.05))
            L, D = 196, 512
        else:
            eng = LRPEngine(decoder="gridtd", L=49, D=2048, H=32, E=32, V=50, max_images=4, max_tokens=ntok, max_caption_len=6,
                            resnet={"stem": 64, "stacks": RESNET101_STACKS})
            eng.set_weights(resnet_weights(rs))
            L, D = 49, 2048
        eng.set_precision("fp32")
        eng.encode_images(rs.uniform(-120, 130, size=(4, 224, 224, 3)).astype(np.float32))
        idx = [i % 4 for i in range(ntok)]
        head = eng._dev(rs.standard_normal((ntok, L, D)).astype(np.float32))
        out = eng.cnn_walk(idx, head, "gradient")
        ms = {wk: _event_ms(lambda: eng.cnn_walk(idx, head, wk, out=out)) for wk in ("guided_backprop", "deconvnet", "guided_backprop", "deconvnet")}
        print("%-9s %2d tokens of 4 images: guided_backprop %.2f ms, deconvnet %.2f ms (%.2f x)" % (
            name, ntok, ms["guided_backprop"], ms["deconvnet"], ms["deconvnet"] / ms["guided_backprop"]), flush=True)
        del eng


if __name__ == "__main__":
    walks()
    smoothgrad()
