#!/usr/bin/env python3
"""The conv rule table (lrp_set_cnn_rules) on an MI355X: what profiles/rule_table.txt records.

  bench    VGG16, 224 x 224, 32 images x 10 tokens: encode ms, explain_tokens ms, ms of the walk's launches and workspace for
           PresetAFlat and PresetBFlat (bf16x3) and the composite [bounded | (2,1) x lower half | epsilon(0.25) x upper half]
           (fp32), each next to the default walk in the same process and arithmetic
  full     full-size parity (2 images x 2 maps) of PresetAFlat in bf16x3 and of the composite in fp32 against the float64
           restatement tests/rule_table_ref.py; its evaluation takes minutes on the CPU, so `--ref FILE.npz` reads / writes a
           cache of it (`--ref-only`: compute the cache and stop; needs no GPU)

Without arguments the steps run one after the other, each in a process of its own under its own time limit, and the run stops
at the first step that fails.  Usage (GPU box, repository root): python profiles/rule_table_bench.py [--ref FILE.npz]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
STEPS = (("bench", 480), ("full", 420))                   # seconds
BOUNDS = (-124.0, 152.0)


def tables(n_conv):
    from lrp_imagecaptioning_amd.analyzer import rule_table
    half = (n_conv - 1) // 2
    composite = [("alphabeta", 2, 1, True)] * half + [("epsilon", 0.25, True)] * (n_conv - 1 - half)
    return {"presetAflat": rule_table("Alpha1Beta0", "Flat", n_conv), "presetBflat": rule_table("Alpha2Beta1", "Flat", n_conv),
            "composite": rule_table(composite, BOUNDS, n_conv)}


def rel_l1(a, b):
    import numpy as np
    return float(np.abs(a.astype(np.float64) - b).sum() / np.abs(b).sum())


def step_bench():
    import numpy as np
    import torch
    from alphabeta_bench import _encode_ms, _walk_ms
    from bench import synth_weights
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import VGG16_CFG, captions, images
    B, T, V = 32, 10, 10000
    rs = np.random.RandomState(1)
    X = torch.as_tensor(images(rs, B)).cuda()
    caps = captions(rs, B, T, V)
    idx = [b for b in range(B) for _ in range(T)]
    tpos = [t for _ in range(B) for t in range(1, T + 1)]
    tabs = tables(len(VGG16_CFG))
    print("== bench geometry: VGG16 224 x 224, %d images x %d tokens (320 maps); explain_tokens = decoder explain + CNN walk" % (B, T))
    for prec, names in (("bf16x3", ("presetAflat", "presetBflat")), ("fp32", ("composite",))):
        eng = LRPEngine(decoder="adaptive", V=V, max_images=B, max_tokens=B * T, max_caption_len=T + 1)
        eng.set_weights(synth_weights(0, V))
        eng.set_precision(prec)
        out = torch.empty((B * T, 224, 224, 3), dtype=torch.float32, device="cuda")
        ws0 = eng.workspace_bytes
        base = None
        for name in ("default",) + names:
            if name == "default":
                eng.set_cnn_rule(1, 0)
            else:
                eng.set_cnn_rules(tabs[name])
            enc = _encode_ms(eng, X)
            eng.decoder_forward(caps)
            total, rec = _walk_ms(eng, idx, tpos, out)
            base = base or (enc, total, sum(rec))
            print("%-6s %-11s encode %7.2f ms (x%.2f)  explain_tokens %7.2f ms (x%.2f)  walk launches %7.2f ms (x%.2f, %d records)  workspace %.2f GB (+%.2f)"
                  % (prec, name, enc, enc / base[0], total, total / base[1], sum(rec), sum(rec) / base[2], len(rec), eng.workspace_bytes / 1e9,
                     (eng.workspace_bytes - ws0) / 1e9), flush=True)
            print("       per launch, top first: " + " ".join("%.2f" % m for m in rec), flush=True)
        del eng, out
        torch.cuda.empty_cache()


def _full_ref(ref_path):
    import numpy as np
    import torch
    import rule_table_ref as RT
    from lrp_imagecaptioning_amd.synthetic import VGG16_CFG, images, vgg_weights
    from oracle import cnn_lrp_ref as C
    rs = np.random.RandomState(0)
    w = vgg_weights(rs)
    layers = C.vgg_layers(w, VGG16_CFG)
    X = images(rs, 2)
    idx = [0, 1, 1, 0]
    tabs = tables(len(VGG16_CFG))
    if ref_path and os.path.exists(ref_path):
        z = np.load(ref_path)
        return w, X, idx, z["R"], {n: (z[n + "_ref"], z[n + "_ref32"]) for n in ("presetAflat", "composite")}
    t = time.time()
    feat = C.forward(layers, X)
    R = (rs.standard_normal((4, 14, 14, 512)) * feat[idx]).astype(np.float32)
    refs = {n: (RT.analyze(layers, X[idx], R, tabs[n]), RT.analyze(layers, X[idx], R, tabs[n], dtype=torch.float32)) for n in ("presetAflat", "composite")}
    print("float64 and float32 restatements: %.0f s on the CPU" % (time.time() - t), flush=True)
    if ref_path:
        np.savez(ref_path, R=R, **{n + s: v for n, (a, b) in refs.items() for s, v in (("_ref", a), ("_ref32", b))})
    return w, X, idx, R, refs


def step_full(ref_path):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import VGG16_CFG
    print("== full size: VGG16 224 x 224, 2 images x 2 maps", flush=True)
    w, X, idx, R, refs = _full_ref(ref_path)
    tabs = tables(len(VGG16_CFG))
    for name, prec in (("presetAflat", "bf16x3"), ("presetAflat", "fp32"), ("composite", "fp32")):
        ref, ref32 = refs[name]
        print("%-11s float32 restatement, relative L1 per map vs its float64 evaluation: %s" % (name, " ".join("%.3e" % rel_l1(ref32[i], ref[i]) for i in range(4))))
        eng = LRPEngine(decoder="adaptive", cnn_cfg=VGG16_CFG, L=196, D=512, H=32, E=32, V=50, max_images=2, max_tokens=4, max_caption_len=4)
        eng.set_weights(w)
        eng.set_precision(prec)
        eng.set_cnn_rules(tabs[name])
        eng.encode_images(X)
        out = eng.cnn_explain(idx, R).cpu().numpy()
        print("%-11s %-7s relative L1 per map vs the float64 restatement: %s" % (name, prec, " ".join("%.3e" % rel_l1(out[i], ref[i]) for i in range(4))),
              flush=True)
        del eng


def main():
    args = sys.argv[1:]
    ref = args[args.index("--ref") + 1] if "--ref" in args else None
    if "--ref-only" in args:
        return _full_ref(ref)
    if "--step" in args:
        name = args[args.index("--step") + 1]
        return {"bench": step_bench, "full": lambda: step_full(ref)}[name]()
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
