#!/usr/bin/env python3
"""The alpha-beta conv rule with beta > 0 on the ResNet encoder (lrp_set_cnn_rule on a ResNet handle) on an
MI355X: what profiles/resnet_alphabeta.txt records.

  parity   the nets of tests/test_gpu_resnet_alphabeta.py (3 images, one map each; fp32 and bf16x3; (2, 1), `mid` also at
           (1.5, 0.5)) against the float64 literal walk tests/resnet_ab_ref.py, the float32 literal graph's own figure beside each
  bench    ResNet-101 + grid-TD, 224 x 224, 32 images x 10 tokens, bf16x3 and fp32: encode, explain_tokens and the walk's conv
           launches at (1, 0) and (2, 1) in one process, workspace bytes

Each step runs in a process of its own under its own time limit; the run stops at the first step that fails.
Usage (GPU box, repository root): python profiles/resnet_alphabeta_bench.py"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEPS = (("parity", 240), ("bench", 420))               # seconds


def rel_l1(a, b):
    import numpy as np
    return float(np.abs(a.astype(np.float64) - b).sum() / np.abs(b).sum())


def step_parity():
    import test_gpu_resnet_alphabeta as G
    print("== parity: relative L1 per map vs the float64 literal walk | the float32 literal graph's own, per map")
    print("   (the tests' draws: bias_std 0.2, X ~ U(-120, 130), R = randn * feat; emit = the pair-emitting encode)")
    for net in G.NETS:
        for rule in ((2, 1), (1.5, 0.5)) if net == "mid" else ((2, 1),):
            c = G._case(net, *rule)
            ref32 = G._literal_float32(c["w"], c["spec"], c["X"], c["R"], *rule)
            own = " ".join("%.2e" % rel_l1(ref32[i], c["ref"][i]) for i in range(G.B))
            for prec in ("fp32", "bf16x3"):
                eng = G._engine(net, c["w"])
                eng.set_precision(prec)
                eng.set_cnn_rule(*rule)
                eng.encode_images(c["X"])
                out = eng.cnn_explain(list(range(G.B)), c["R"]).cpu().numpy()
                print("%-6s alpha %-4g beta %-4g %-7s %s | %s%s" % (net, rule[0], rule[1], prec,
                                                                   " ".join("%.2e" % rel_l1(out[i], c["ref"][i]) for i in range(G.B)), own,
                                                                   "  (emit)" if G.NETS[net][4] and prec == "bf16x3" else ""), flush=True)
                del eng


def _median_ms(fn, reps=3):
    import torch
    fn(); torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def step_bench():
    import numpy as np
    import torch
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import RESNET101_STACKS, captions, gridtd_weights, images, resnet_weights
    B, T, V = 32, 10, 10000
    rs = np.random.RandomState(0)
    w = resnet_weights(rs)
    w.update(gridtd_weights(rs, 49, 2048, 512, 512, V))
    X = torch.as_tensor(images(rs, B)).cuda()
    caps = captions(rs, B, T, V)
    idx = [b for b in range(B) for _ in range(T)]
    tpos = [t for _ in range(B) for t in range(1, T + 1)]
    print("== bench geometry: ResNet-101 + grid-TD, 224 x 224, %d images x %d tokens; explain_tokens = decoder explain + CNN walk" % (B, T))
    for prec in ("bf16x3", "fp32"):
        eng = LRPEngine(decoder="gridtd", img_hw=(224, 224), L=49, D=2048, H=512, E=512, V=V, max_images=B, max_tokens=B * T,
                        max_caption_len=T + 1, resnet={"stem": 64, "stacks": RESNET101_STACKS})
        eng.set_weights(w)
        eng.set_precision(prec)
        out = torch.empty((B * T, 224, 224, 3), dtype=torch.float32, device="cuda")
        res = {}
        for rule in ((1, 0), (2, 1)):
            eng.set_cnn_rule(*rule)
            enc = _median_ms(lambda: eng.encode_images(X))
            eng.decoder_forward(caps)
            total = _median_ms(lambda: eng.explain_tokens(idx, tpos, out=out))
            eng.profile_enable(True)
            eng.explain_tokens(idx, tpos, out=out); torch.cuda.synchronize()
            rec = [m for m, _ in eng.profile_records()]
            eng.profile_enable(False)
            assert bool(torch.isfinite(out).all())
            res[rule] = (enc, total, sum(rec), eng.workspace_bytes)
            print("%-6s rule %s: encode %.2f ms, explain_tokens %.2f ms, the walk's conv launches %.2f ms (%d records), workspace %.2f GB"
                  % (prec, rule, enc, total, sum(rec), len(rec), eng.workspace_bytes / 1e9), flush=True)
        a, b = res[(1, 0)], res[(2, 1)]
        print("%-6s (2,1) / (1,0): conv launches x%.2f, explain_tokens x%.2f, encode x%.2f (+%.2f ms), workspace +%.2f GB"
              % (prec, b[2] / a[2], b[1] / a[1], b[0] / a[0], b[0] - a[0], (b[3] - a[3]) / 1e9), flush=True)
        del eng, out
        torch.cuda.empty_cache()


def main():
    args = sys.argv[1:]
    if "--step" in args:
        return {"parity": step_parity, "bench": step_bench}[args[args.index("--step") + 1]]()
    for name, limit in STEPS:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], cwd=ROOT, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print("step %s ended with status %d: stopping here" % (name, rc), flush=True)
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
