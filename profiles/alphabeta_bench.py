#!/usr/bin/env python3
"""The alpha-beta conv rule with beta > 0 (lrp_set_cnn_rule) on an MI355X: what profiles/alphabeta.txt records.

  parity   the walk cases of tests/test_gpu_alphabeta.py (TINY 16x16 B=3, MID 32x32 B=2, WIDE 32x32 B=2; two maps per image,
           fp32 and bf16x3, (2,1) and (1.5,0.5)) against the float64 restatement tests/alphabeta_ref.py, the float32
           restatement's own figure beside each
  bench    VGG16, 224 x 224, 32 images x 10 tokens, bf16x3 and fp32: ms per walk and per launch for (2,1) next to the
           alpha1beta0 walk in the same process, encode ms with and without the inhibitor pass, workspace bytes
  full     one full-size parity figure (2 images x 2 maps) against the restatement; its float64 evaluation takes minutes on the
           CPU, so `--ref FILE.npz` reads / writes a cache of it

Without arguments the three steps run one after the other, each in a process of its own under its own time limit, and the run
stops at the first step that fails.  Usage (GPU box, repository root): python profiles/alphabeta_bench.py [--ref FILE.npz]"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEPS = (("parity", 240), ("bench", 420), ("full", 540))        # seconds


def rel_l1(a, b):
    import numpy as np
    return float(np.abs(a.astype(np.float64) - b).sum() / np.abs(b).sum())


def step_parity():
    import alphabeta_ref as AB
    import test_gpu_alphabeta as G
    print("== parity: max over the maps of relative L1 vs the float64 restatement | the float32 restatement's own | smallest |Z|")
    print("   (seed 7, bias_std 0.3, X ~ U(-120, 130), two maps per image; `f32 per map` = the float32 restatement, map by map)")
    for name, (cfg, hw, B) in G.NETS.items():
        w, X, idx, R, layers = G._net(name)
        zmin = AB.min_abs_denominator(layers, X)
        for rule in G.RULES:
            ref, ref32 = G._refs(name, rule)
            per_map = [rel_l1(ref32[i], ref[i]) for i in range(2 * B)]
            own = max(per_map)
            print("%-5s alpha %-4g beta %-4g f32 per map: %s" % (name, rule[0], rule[1], " ".join("%.2e" % e for e in per_map)), flush=True)
            for prec in ("fp32", "bf16x3"):
                eng = G._engine(cfg, hw, B, 2 * B, w, prec, rule)
                eng.encode_images(X)
                out = eng.cnn_explain(list(idx), R).cpu().numpy()
                err = max(rel_l1(out[i], ref[i]) for i in range(2 * B))
                print("%-5s alpha %-4g beta %-4g %-7s %.3e | %.3e | %.3e" % (name, rule[0], rule[1], prec, err, own, zmin), flush=True)
                del eng


def _walk_ms(eng, idx, tpos, out, reps=3):
    import torch
    eng.explain_tokens(idx, tpos, out=out); torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); eng.explain_tokens(idx, tpos, out=out); b.record()
    torch.cuda.synchronize()
    total = statistics.median(a.elapsed_time(b) for a, b in ev)
    eng.profile_enable(True)
    eng.explain_tokens(idx, tpos, out=out); torch.cuda.synchronize()
    rec = [m for m, _ in eng.profile_records()]
    eng.profile_enable(False)
    return total, rec


def _encode_ms(eng, X, reps=3):
    import torch
    eng.encode_images(X); torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); eng.encode_images(X); b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def step_bench():
    import numpy as np
    import torch
    from bench import synth_weights
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import VGG16_CFG, captions, images
    B, T, V = 32, 10, 10000
    rs = np.random.RandomState(1)
    X = torch.as_tensor(images(rs, B)).cuda()
    caps = captions(rs, B, T, V)
    idx = [b for b in range(B) for _ in range(T)]
    tpos = [t for _ in range(B) for t in range(1, T + 1)]
    names = [c[0] for c in VGG16_CFG][::-1]
    print("== bench geometry: VGG16 224 x 224, %d images x %d tokens; explain_tokens = decoder explain + CNN walk" % (B, T))
    for prec in ("bf16x3", "fp32"):
        eng = LRPEngine(decoder="adaptive", V=V, max_images=B, max_tokens=B * T, max_caption_len=T + 1)
        eng.set_weights(synth_weights(0, V))
        eng.set_precision(prec)
        out = torch.empty((B * T, 224, 224, 3), dtype=torch.float32, device="cuda")
        ws0 = eng.workspace_bytes
        res = {}
        for rule in ((1, 0), (2, 1)):
            eng.set_cnn_rule(*rule)
            enc = _encode_ms(eng, X)
            eng.decoder_forward(caps)
            total, rec = _walk_ms(eng, idx, tpos, out)
            res[rule] = (enc, total, rec)
            print("%-6s rule %s: encode %.2f ms, explain_tokens %.2f ms, walk launches %.2f ms (%d records), workspace %.2f GB"
                  % (prec, rule, enc, total, sum(rec), len(rec), eng.workspace_bytes / 1e9), flush=True)
            print("       per launch, top first: " + " ".join("%.2f" % m for m in rec), flush=True)
        a, b = res[(1, 0)], res[(2, 1)]
        print("%-6s (2,1) / (1,0): walk launches x%.2f, explain_tokens x%.2f, encode x%.2f (+%.2f ms inhibitor pass), workspace +%.2f GB"
              % (prec, sum(b[2]) / sum(a[2]), b[1] / a[1], b[0] / a[0], b[0] - a[0], (eng.workspace_bytes - ws0) / 1e9))
        print("       layers of the (2,1) records: " + " ".join(names))
        del eng, out
        torch.cuda.empty_cache()


def step_full(ref_path):
    import numpy as np
    import torch
    import alphabeta_ref as AB
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import VGG16_CFG, images, vgg_weights
    from oracle import cnn_lrp_ref as C
    rs = np.random.RandomState(0)
    w = vgg_weights(rs)
    layers = C.vgg_layers(w, VGG16_CFG)
    X = images(rs, 2)
    idx = [0, 1, 1, 0]
    print("== full size: VGG16 224 x 224, 2 images x 2 maps, rule (2, 1)", flush=True)
    if ref_path and os.path.exists(ref_path):
        z = np.load(ref_path)
        R, ref, ref32 = z["R"], z["ref"], z["ref32"]
    else:
        t = time.time()
        feat = C.forward(layers, X)
        R = (rs.standard_normal((4, 14, 14, 512)) * feat[idx]).astype(np.float32)
        ref = AB.analyze(layers, X[idx], R, 2, 1)
        ref32 = AB.analyze(layers, X[idx], R, 2, 1, dtype=torch.float32)
        print("float64 and float32 restatement: %.0f s on the CPU" % (time.time() - t), flush=True)
        if ref_path:
            np.savez(ref_path, R=R, ref=ref, ref32=ref32)
    print("float32 restatement, relative L1 per map vs its float64 evaluation: %s" % " ".join("%.3e" % rel_l1(ref32[i], ref[i]) for i in range(4)),
          flush=True)
    for prec in ("fp32", "bf16x3"):
        eng = LRPEngine(decoder="adaptive", cnn_cfg=VGG16_CFG, L=196, D=512, H=32, E=32, V=50, max_images=2, max_tokens=4, max_caption_len=4)
        eng.set_weights(w)
        eng.set_precision(prec)
        eng.set_cnn_rule(2, 1)
        eng.encode_images(X)
        out = eng.cnn_explain(idx, R).cpu().numpy()
        print("%-7s relative L1 per map vs the float64 restatement: %s" % (prec, " ".join("%.3e" % rel_l1(out[i], ref[i]) for i in range(4))),
              flush=True)
        del eng


def main():
    args = sys.argv[1:]
    ref = args[args.index("--ref") + 1] if "--ref" in args else None
    if "--step" in args:
        name = args[args.index("--step") + 1]
        return {"parity": step_parity, "bench": step_bench, "full": lambda: step_full(ref)}[name]()
    for name, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + (["--ref", ref] if ref else [])
        try:
            rc = subprocess.run(cmd, cwd=ROOT, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print("step %s ended with status %d: stopping here" % (name, rc), flush=True)
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
