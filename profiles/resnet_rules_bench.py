#!/usr/bin/env python3
"""The rule pair of the ResNet encoder's LRP walk (lrp_set_resnet_rules) on an MI355X: what
profiles/resnet_rules.txt records.

  parity   every case of tests/test_gpu_resnet_rules.py's parity test (tests/resnet_rule_cases.py: 3 images, one map each; fp32, and
           bf16x3 where the pair has no epsilon kind) against the float64 literal walk tests/resnet_rule_ref.py, the float32 literal
           graph's own figure beside each
  bench    ResNet-101 + grid-TD, 224 x 224, 32 images x 10 tokens, one process: encode, explain_tokens, the walk's conv launches
           and the workspace under the default, (2, 1), ZPlus, PresetAFlat, alpha2beta1-IgnoreBias and PresetBFlat (bf16x3), and
           under the default, Z and epsilon 0.25 (fp32).  encode - encode(default) is what the pair's gate pass costs.

Each step runs in a process of its own under its own time limit; the run stops at the first step that fails.
Usage (GPU box, repository root): python profiles/resnet_rules_bench.py"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEPS = (("parity", 300), ("bench", 540))               # seconds


def rel_l1(a, b):
    import numpy as np
    return float(np.abs(a.astype(np.float64) - b).sum() / np.abs(b).sum())


def step_parity():
    import resnet_rule_cases as RC
    import test_gpu_resnet_rules as G
    from gpu_util import band_rel_l1
    print("== parity: relative L1 per map vs the float64 literal walk | noise32 (the float32 literal graph's own, worst map) | worst band / its bar")
    print("   (the tests' draws: bias_std 0.2, X ~ U(-120, 130), R = randn * feat)")
    for net, pair, prec in G.PARITY:
        c = RC.case(net, pair)
        eng = G._engine(net, c["w"])
        eng.set_precision(prec)
        G._set(eng, pair)
        eng.encode_images(c["X"])
        out = eng.cnn_explain(G.IDX, c["R"]).cpu().numpy()
        band = max(band_rel_l1(out[i], c["ref"][i]) for i in range(RC.B))
        print("%-6s %-14s %-7s %s | %.2e | %.2e / %.2e" % (net, pair, prec, " ".join("%.2e" % rel_l1(out[i], c["ref"][i]) for i in range(RC.B)),
                                                          c["noise32"], band, c["band_bar"]), flush=True)
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
    AB = lambda a, b, bias=True: ("alphabeta", a, b, bias)
    plans = {"bf16x3": (("default", AB(1, 0), None), ("(2, 1)", AB(2, 1), None), ("ZPlus", AB(1, 0, False), None),
                        ("PresetAFlat", AB(1, 0), ("flat",)), ("a2b1-IgnoreBias", AB(2, 1, False), None), ("PresetBFlat", AB(2, 1), ("flat",))),
             "fp32": (("default", AB(1, 0), None), ("Z", ("epsilon", 0.0, True), None), ("epsilon 0.25", ("epsilon", 0.25, True), None))}
    print("== bench geometry: ResNet-101 + grid-TD, 224 x 224, %d images x %d tokens; explain_tokens = decoder explain + CNN walk" % (B, T))
    for prec, plan in plans.items():
        eng = LRPEngine(decoder="gridtd", img_hw=(224, 224), L=49, D=2048, H=512, E=512, V=V, max_images=B, max_tokens=B * T,
                        max_caption_len=T + 1, resnet={"stem": 64, "stacks": RESNET101_STACKS})
        eng.set_weights(w)
        eng.set_precision(prec)
        out = torch.empty((B * T, 224, 224, 3), dtype=torch.float32, device="cuda")
        base = None
        for name, rule, stem in plan:
            eng.set_resnet_rules(rule, stem)
            enc = _median_ms(lambda: eng.encode_images(X))
            eng.decoder_forward(caps)
            total = _median_ms(lambda: eng.explain_tokens(idx, tpos, out=out))
            eng.profile_enable(True)
            eng.explain_tokens(idx, tpos, out=out); torch.cuda.synchronize()
            rec = [m for m, _ in eng.profile_records()]
            eng.profile_enable(False)
            assert bool(torch.isfinite(out).all())
            base = base or (enc, total)
            print("%-6s %-16s encode %7.2f ms (%+7.2f), explain_tokens %7.2f ms (x%.2f), the walk's conv launches %7.2f ms (%d records), "
                  "workspace %.2f GB" % (prec, name, enc, enc - base[0], total, total / base[1], sum(rec), len(rec), eng.workspace_bytes / 1e9),
                  flush=True)
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
