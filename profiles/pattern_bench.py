#!/usr/bin/env python3
"""PatternNet / PatternAttribution (lrp_pattern_*, LRP_WALK_PATTERNNET / _PATTERN_ATTRIBUTION) on an MI355X: what
profiles/pattern.txt records.

VGG16, 224 x 224, 32 images x 10 heads (320 maps), LRP_PREC_FP32:
  * the fit: ms per batch of 32 images (encode excluded) and its split over the four steps — pre-activation conv, mask pass, the
    two products, the float64 accumulation — from lrp_profile_records; lrp_pattern_fit_end; what the pattern entries allocate
  * both walks, projected and not, against the gradient walk on the same handle (HIP events around the call, median of REPS)
  * per layer of the projected PatternNet walk: the conv's ms, and for the streaming step (row maximum + pattern_project_kernel)
    ms next to the bytes it moves, computed here from the shapes, as TB/s and as a share of the 6.3 TB/s a float4 copy reaches

Usage (GPU box, repository root): python profiles/pattern_bench.py"""
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


def stream_bytes(cfg, hw, n):
    """bytes of the streaming step per layer, launch order (top first): the accumulator is read twice (row maximum, projection),
    the gate of the layer below is read and S written at full resolution (four cells per item behind a pool)"""
    geo, h = [], hw
    for name, cin, cout, pool in cfg:
        geo.append((name, cin, h, pool))
        h = h // 2 if pool else h
    out = []
    for li in range(len(geo) - 1, 0, -1):
        name, cin, h, _ = geo[li]
        up = 4 if geo[li - 1][3] else 1
        out.append(("%s <- %s%s" % (geo[li - 1][0], name, " (pool)" if up == 4 else ""), 4 * n * h * h * cin * (2 + up + up)))
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
    out = torch.empty((n, 224, 224, 3), dtype=torch.float32, device="cuda")
    print("== VGG16 224 x 224, %d images x %d heads (%d maps), LRP_PREC_FP32; ms, median of %d" % (B, T, n, REPS))
    eng = LRPEngine(decoder="adaptive", V=V, max_images=B, max_tokens=n, max_caption_len=T + 1)
    eng.set_weights(synth_weights(0, V))
    eng.set_precision("fp32")
    ws0 = eng.workspace_bytes
    eng.encode_images(X)
    encode = _event_ms(lambda: eng.encode_images(X))
    grad = _event_ms(lambda: eng.cnn_walk(idx, head, "gradient", out=out))
    # ---- the fit
    eng.pattern_fit_begin("relu")
    ws_fit = eng.workspace_bytes
    eng.encode_images(X)
    eng.pattern_fit_batch(); torch.cuda.synchronize()       # (first call: nothing left to allocate, caches warm)
    times = []
    for _ in range(REPS):
        eng.encode_images(X)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); eng.pattern_fit_batch(); b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    eng.encode_images(X)
    eng.profile_enable(True)
    eng.pattern_fit_batch(); torch.cuda.synchronize()
    rec = eng.profile_records(cap=256)
    eng.profile_enable(False)
    assert len(rec) == 4 * len(VGG16_CFG), len(rec)
    split = [sum(m for m, _ in rec[k::4]) for k in range(4)]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); eng.pattern_fit_end(); b.record(); torch.cuda.synchronize()
    end = a.elapsed_time(b)
    print("fit    encode of 32 images %7.2f ms;  lrp_pattern_fit_batch %7.2f ms per batch of 32:  conv %6.2f | mask pass %6.2f | "
          "products %6.2f | accumulate %6.2f;  lrp_pattern_fit_end %6.2f ms" % (encode, statistics.median(times), split[0], split[1],
                                                                                 split[2], split[3], end))
    print("       per conv (ms: conv, mask pass, products, accumulate):")
    for li, (name, cin, cout, _) in enumerate(VGG16_CFG):
        print("         %-14s %6.3f %6.3f %6.3f %6.3f" % ((name,) + tuple(m for m, _ in rec[4 * li:4 * li + 4])))
    # ---- the walks
    eng.encode_images(X)
    res = {}
    for proj in (True, False):
        eng.set_pattern_projection(proj)
        for name in ("patternnet", "pattern_attribution"):
            res[(name, proj)] = _event_ms(lambda: eng.cnn_walk(idx, head, name, out=out))
    ws_walk = eng.workspace_bytes
    print("walks  gradient %7.2f ms | patternnet %7.2f (x%.2f), unprojected %7.2f | pattern_attribution %7.2f (x%.2f), unprojected %7.2f" % (
        grad, res[("patternnet", True)], res[("patternnet", True)] / grad, res[("patternnet", False)],
        res[("pattern_attribution", True)], res[("pattern_attribution", True)] / grad, res[("pattern_attribution", False)]))
    print("       workspace %.2f GB at create, +%.2f GB by lrp_pattern_fit_begin (kept activations, sums, fit scratch), +%.3f GB by "
          "fit_end and the first walk (patterns, packed matrices, partials)" % (ws0 / 1e9, (ws_fit - ws0) / 1e9, (ws_walk - ws_fit) / 1e9))
    eng.set_pattern_projection(True)
    eng.profile_enable(True)
    eng.cnn_walk(idx, head, "patternnet", out=out); torch.cuda.synchronize()
    rec = eng.profile_records(cap=256)
    eng.profile_enable(False)
    conv = [m for m, f in rec if f > 0]
    stream = [m for m, f in rec if f == 0]
    sb = stream_bytes(VGG16_CFG, 224, n)
    assert len(stream) == len(sb) + 2, (len(stream), len(sb))   # + the head, + the image-level tensor
    print("       projected patternnet: convs %7.2f ms, streaming steps %7.2f ms (head %.3f, image %.3f)" % (
        sum(conv), sum(stream), stream[0], stream[-1]))
    for (name, nbytes), m in zip(sb, stream[1:-1]):
        print("         %-40s %6.3f ms  %6.2f GB  %5.2f TB/s  (%3.0f %% of a float4 copy's %.1f TB/s)" % (
            name, m, nbytes / 1e9, nbytes / m / 1e9, 100 * nbytes / m / 1e9 / COPY_TBS, COPY_TBS))


if __name__ == "__main__":
    main()
