#!/usr/bin/env python3
"""Per-launch A/B of the chunk loop of the 128 x 64 weights-in-registers tile (the walk's N <= 64 launches: block2_conv1 and the
folded block1_conv2) at the bench size (B = 32, 320 tokens): LRP_CONV_BREG2 = 0 / 1 alternating in one process on one engine,
PASSES passes each, after comparing the heat-maps of the two settings bit for bit.  A pass = 3 walks under the per-launch events
(the walk's records per layer).  Prints every pass and per class the median and range; WON = the new median lies below the old
minimum.  The switch is read by the walk's launcher only: the forward is the same code under both settings and is not timed.
Usage (GPU box, repository root): python profiles/breg2_ab.py [PASSES]    (output: profiles/breg2_ab.txt, section 2)"""
import os, sys, statistics
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PASSES = int(sys.argv[1]) if len(sys.argv) > 1 else 5
import torch
from bench import synth_weights
from lrp_imagecaptioning_amd.engine import LRPEngine, switches
from lrp_imagecaptioning_amd.synthetic import VGG16_CFG, captions, images
B, T, V = 32, 10, 10000
eng = LRPEngine(decoder="adaptive", V=V, max_images=B, max_tokens=B * T, max_caption_len=T + 1)
eng.set_weights(synth_weights(0, V))
rs = np.random.RandomState(1)
X = torch.as_tensor(images(rs, B)).cuda()
caps = captions(rs, B, T, V)
idx = [b for b in range(B) for _ in range(T)]
tpos = [t for _ in range(B) for t in range(1, T + 1)]
out = torch.empty((B * T, 224, 224, 3), dtype=torch.float32, device="cuda")
eng.encode_images(X); eng.decoder_forward(caps)
ref = {}
for on in (1, 0):
    with switches(LRP_CONV_BREG2=on):
        eng.explain_tokens(idx, tpos, out=out); torch.cuda.synchronize()
        ref[on] = out.clone()
print("heat-maps bit-identical on/off:", bool(torch.equal(ref[0], ref[1])), "finite:", bool(torch.isfinite(ref[1]).all()),
      "non-zero:", bool((ref[1].abs().sum() > 0).item()), flush=True)
del ref

names = [c[0] for c in VGG16_CFG][::-1]
res = {0: [], 1: []}
for p in range(PASSES):
    for on in (0, 1):
        with switches(LRP_CONV_BREG2=on):
            eng.explain_tokens(idx, tpos, out=out); torch.cuda.synchronize()
            eng.profile_enable(True)
            acc = None
            for _ in range(3):
                eng.explain_tokens(idx, tpos, out=out); torch.cuda.synchronize()
                rec = eng.profile_records()
                acc = rec if acc is None else [(a + b, f) for (a, f), (b, _) in zip(acc, rec)]
            eng.profile_enable(False)
            res[on].append([m / 3 for m, _ in acc])
        print("pass %d BREG2=%d walk %.3f ms: %s" % (p, on, sum(res[on][-1]), " ".join("%.3f" % m for m in res[on][-1])), flush=True)
print("records per walk:", len(res[0][0]), names[:len(res[0][0])])
print("%-14s %28s %28s" % ("class", "BREG2=0 med [min,max]", "BREG2=1 med [min,max]"))


def line(name, v0, v1):
    won = statistics.median(v1) < min(v0)
    print("%-14s %28s %28s %s" % (name, "%.3f [%.3f, %.3f]" % (statistics.median(v0), min(v0), max(v0)),
                                  "%.3f [%.3f, %.3f]" % (statistics.median(v1), min(v1), max(v1)), "WON" if won else ""))


for k in range(len(res[0][0])):
    line(names[k] if k < len(names) else str(k), [r[k] for r in res[0]], [r[k] for r in res[1]])
line("walk total", [sum(r) for r in res[0]], [sum(r) for r in res[1]])
