#!/usr/bin/env python3
"""The traced LRP walk (lrp_set_layer_trace, lrp_cnn_explain_traced) on an MI355X: what profiles/layer_trace.txt records.

VGG16, 224 x 224, 32 images x 10 tokens (320 maps), the default rule, in LRP_PREC_FP32 and in the default bf16x3, one engine per mode:
  * the untraced walk (lrp_cnn_explain) on a handle that never saw the switch, and with the switch on
  * the traced walk with statistics only, and with every tensor kept (HIP events around the call, median of REPS)
  * lrp_workspace_bytes at create, with the switch on, after the first traced call; the size of the keep-all buffer
  * per layer (lrp_profile_records): the conv's ms, and for the streaming kernel (trace_layer_kernel) ms next to the bytes it moves,
    computed here from the shapes, as TB/s and as a share of the 6.3 TB/s a float4 copy reaches

Usage (GPU box, repository root): python profiles/layer_trace_bench.py"""
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


def stream_bytes(cfg, hw, n, keep):
    """bytes of trace_layer_kernel per layer, launch order (top first), the default rule (one chain, the gate is the mask): reads of
    the accumulator, the kept input and the gate (all four cells of a window behind a pool), writes of S (at full resolution) and,
    with keep, of the kept tensor(s)"""
    geo, h = [], hw
    for name, cin, cout, pool in cfg:
        geo.append((name, cin, h, pool))
        h = h // 2 if pool else h
    out = []
    for li in range(len(geo) - 1, 0, -1):
        name, cin, h, _ = geo[li]
        up = 4 if geo[li - 1][3] else 1
        per = 4 * n * h * h * cin
        out.append(("%s <- %s%s" % (geo[li - 1][0], name, " (pool)" if up == 4 else ""), per * (2 + up + up + (1 + (up if up == 4 else 0) if keep else 0))))
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
    print("== VGG16 224 x 224, %d images x %d tokens (%d maps), default rule; ms, median of %d" % (B, T, n, REPS))
    for prec in ("fp32", "bf16x3"):
        eng = LRPEngine(decoder="adaptive", V=V, max_images=B, max_tokens=n, max_caption_len=T + 1)
        eng.set_weights(synth_weights(0, V))
        eng.set_precision(prec)
        ws0 = eng.workspace_bytes
        eng.encode_images(X)
        plain = _event_ms(lambda: eng.cnn_explain(idx, head, out=out))
        eng.set_layer_trace(True)
        ws_on = eng.workspace_bytes
        eng.encode_images(X)
        plain_on = _event_ms(lambda: eng.cnn_explain(idx, head, out=out))
        stats_only = _event_ms(lambda: eng.cnn_explain_traced(idx, head, out=out))
        ws_tr = eng.workspace_bytes
        _, total = eng._trace_info(n, (1 << len(eng.trace_tensors())) - 1)
        print("%-6s untraced walk %7.2f ms (switch on: %7.2f)  traced, statistics only %7.2f ms (x%.2f)  workspace %.2f GB at create, "
              "+%.2f GB kept activations, +%.3f GB partials" % (prec, plain, plain_on, stats_only, stats_only / plain, ws0 / 1e9,
                                                                (ws_on - ws0) / 1e9, (ws_tr - ws_on) / 1e9), flush=True)
        for keep in (False, True):
            eng.profile_enable(True)
            eng.cnn_explain_traced(idx, head, keep=keep, out=out); torch.cuda.synchronize()
            rec = eng.profile_records()
            eng.profile_enable(False)
            conv = [m for m, f in rec if f > 0]
            stream = [m for m, f in rec if f == 0]
            sb = stream_bytes(VGG16_CFG, 224, n, keep)
            assert len(sb) == len(stream), (len(sb), len(stream))
            print("       keep %-5s convs %7.2f ms, streaming kernels %7.2f ms" % (keep, sum(conv), sum(stream)))
            for (name, nbytes), m in zip(sb, stream):
                print("         %-40s %6.3f ms  %6.2f GB  %5.2f TB/s  (%3.0f %% of a float4 copy's %.1f TB/s)" % (
                    name, m, nbytes / 1e9, nbytes / m / 1e9, 100 * nbytes / m / 1e9 / COPY_TBS, COPY_TBS))
        torch.cuda.empty_cache()
        keep_all = _event_ms(lambda: eng.cnn_explain_traced(idx, head, keep=True, out=out))
        print("       traced, keep-all %7.2f ms (x%.2f), keep buffer %.2f GB (allocated by the caller per call: included)" % (
            keep_all, keep_all / plain, 4 * total / 1e9), flush=True)
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
