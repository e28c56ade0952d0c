#!/usr/bin/env python3
"""Does a build compute what another computes on the ResNet encoder?  What profiles/resnet_split_bitexact.txt records.

One row per case: SHA-256 (first 24 hex digits) of the features and of the heat-maps, taken over `out + 0.0` so that the sign of a
zero does not count, the lrp_launch_count delta of the encode (the first one of the handle: it packs what the mode and the rule
need) and of the walk, and lrp_workspace_bytes after the walk.  Run it on two builds and diff the tables:

  python profiles/resnet_split_bitexact.py [--lib PATH/liblrp_hip.so] > table.txt

Nets: `tiny` of tests/test_gpu_resnet.py (B = 2) and the five of tests/test_gpu_resnet_alphabeta.py (B = 3); two maps per image,
image indices 0 .. B-1 and back, so every index is repeated.  The relevance at the top is a seeded normal draw times the
features the build itself computed (a build whose features differ shows it in both digests).  Rows: every net in fp32 and bf16x3;
LRP_FWD_EMIT=0 and LRP_IMG_FUSED=0; the rules (2, 1) and (1.5, 0.5), (2, 1) with LRP_FWD_EMIT=0, (2, 1) then (1, 0); the walks
gradient, input_x_gradient, guided_backprop (fp32) and deconvnet (both modes), with and without the fused stem reverse; weights
set from device tensors, twice; a rule set before and after the weights; the default walk with profiling on (record count and
FLOP sum as well)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (stacks, stem, (H, W), seed, B)
NETS = {
    "tiny": (((4, 2), (8, 2)), 8, (32, 32), 3, 2),
    "ident": (((8, 2),), 8, (16, 16), 1, 3),
    "proj": (((8, 1),), 8, (16, 16), 3, 3),
    "mid": (((8, 2), (16, 3), (32, 2)), 16, (64, 64), 7, 3),
    "stem64": (((32, 2), (64, 2)), 64, (96, 96), 7, 3),
    "wide": (((64, 1), (128, 1), (256, 2), (512, 1)), 64, (160, 96), 0, 3),
}


def digest(t):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy() + 0.0).tobytes()).hexdigest()[:24]


def main():
    from lrp_imagecaptioning_amd import _capi
    if "--lib" in sys.argv:
        _capi.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    import numpy as np
    import torch
    from lrp_imagecaptioning_amd.engine import LRPEngine, switches
    from lrp_imagecaptioning_amd.synthetic import resnet_weights
    lib = _capi.load()

    def draw(net):
        stacks, stem, (h, wd), seed, B = NETS[net]
        rs = np.random.RandomState(seed)
        w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
        X = rs.uniform(-120, 130, (B, h, wd, 3)).astype(np.float32)
        idx = list(range(B)) + list(range(B))[::-1]
        d = 4 * 2 ** (len(stacks) - 1)
        Z = rs.standard_normal((2 * B, (h // d) * (wd // d), 4 * stacks[-1][0])).astype(np.float32)
        return w, X, idx, Z

    def engine(net, prec, w=None):
        stacks, stem, (h, wd), _, B = NETS[net]
        d = 4 * 2 ** (len(stacks) - 1)
        eng = LRPEngine(decoder="adaptive", img_hw=(h, wd), L=(h // d) * (wd // d), D=4 * stacks[-1][0], H=32, E=32, V=50, max_images=B,
                        max_tokens=2 * B, max_caption_len=6, resnet={"stem": stem, "stacks": stacks})
        if w is not None:
            eng.set_weights(w)
        eng.set_precision(prec)
        return eng

    def counted(fn):
        n0 = int(lib.lrp_launch_count())
        out = fn()
        torch.cuda.synchronize()
        return out, int(lib.lrp_launch_count()) - n0

    def row(name, eng, net, walk="lrp", extra=None):
        _, X, idx, Z = draw(net)
        _, n_enc = counted(lambda: eng.encode_images(X))
        feat = eng.get_features()
        R = torch.as_tensor(Z).to(feat.device) * feat[idx]
        fn = (lambda: eng.cnn_explain(idx, R)) if walk == "lrp" else (lambda: eng.cnn_walk(idx, R, walk))
        out, n_walk = counted(fn)
        assert bool(torch.isfinite(out).all()), name
        print("%-44s %s %s %3d %3d %d%s" % (name, digest(feat), digest(out), n_enc, n_walk, eng.workspace_bytes,
                                           extra() if extra else ""), flush=True)

    print("# case                                       sha256(features)[:24] sha256(heat-maps)[:24] encode_launches walk_launches "
          "workspace_bytes")
    W = {net: draw(net)[0] for net in NETS}
    for net in NETS:
        for prec in ("fp32", "bf16x3"):
            row("%s_%s" % (net, prec), engine(net, prec, W[net]), net)
    for net in ("stem64", "wide"):
        with switches(LRP_FWD_EMIT=0):
            row("%s_bf16x3_LRP_FWD_EMIT=0" % net, engine(net, "bf16x3", W[net]), net)
    for prec in ("fp32", "bf16x3"):
        with switches(LRP_IMG_FUSED=0):
            row("stem64_%s_LRP_IMG_FUSED=0" % prec, engine("stem64", prec, W["stem64"]), "stem64")
    for net in ("ident", "proj", "mid", "stem64", "wide"):
        for prec in ("fp32", "bf16x3"):
            eng = engine(net, prec, W[net])
            eng.set_cnn_rule(2, 1)
            row("%s_%s_rule_2_1" % (net, prec), eng, net)
    eng = engine("mid", "bf16x3", W["mid"])
    eng.set_cnn_rule(1.5, 0.5)
    row("mid_bf16x3_rule_1.5_0.5", eng, "mid")
    with switches(LRP_FWD_EMIT=0):
        eng = engine("stem64", "bf16x3", W["stem64"])
        eng.set_cnn_rule(2, 1)
        row("stem64_bf16x3_rule_2_1_LRP_FWD_EMIT=0", eng, "stem64")
    eng = engine("mid", "bf16x3", W["mid"])
    eng.set_cnn_rule(2, 1)
    row("mid_bf16x3_rule_2_1_first", eng, "mid")
    eng.set_cnn_rule(1, 0)
    row("mid_bf16x3_rule_2_1_then_1_0", eng, "mid")
    for walk in ("gradient", "input_x_gradient", "guided_backprop"):
        for net in ("tiny", "mid", "stem64"):
            row("%s_fp32_walk_%s" % (net, walk), engine(net, "fp32", W[net]), net, walk)
        with switches(LRP_IMG_FUSED=0):
            row("stem64_fp32_walk_%s_LRP_IMG_FUSED=0" % walk, engine("stem64", "fp32", W["stem64"]), "stem64", walk)
    for net in ("tiny", "mid", "stem64"):
        for prec in ("fp32", "bf16x3"):
            row("%s_%s_walk_deconvnet" % (net, prec), engine(net, prec, W[net]), net, "deconvnet")
    with switches(LRP_IMG_FUSED=0):
        row("stem64_bf16x3_walk_deconvnet_LRP_IMG_FUSED=0", engine("stem64", "bf16x3", W["stem64"]), "stem64", "deconvnet")
    # weights from device tensors, twice: the second time every packer finds its buffers
    wdev = {k: torch.as_tensor(v).cuda() for k, v in W["mid"].items()}
    eng = engine("mid", "bf16x3")
    eng.set_weights_from_device(wdev)
    row("mid_bf16x3_weights_from_device", eng, "mid")
    eng.set_weights_from_device(wdev)
    row("mid_bf16x3_weights_from_device_again", eng, "mid")
    # a rule before the weights (the rule's buffers are sized without them), and the weights once more behind it
    eng = engine("mid", "bf16x3")
    eng.set_cnn_rule(2, 1)
    eng.set_weights(W["mid"])
    row("mid_bf16x3_rule_2_1_before_weights", eng, "mid")
    eng.set_weights(W["mid"])
    row("mid_bf16x3_rule_2_1_weights_again", eng, "mid")
    eng = engine("mid", "bf16x3", W["mid"])
    eng.profile_enable(True)

    def prof():
        launches, _, flop = eng.profile_query()
        return " prof_launches=%d prof_flop=%r" % (launches, flop)
    row("mid_bf16x3_profile", eng, "mid", extra=prof)


if __name__ == "__main__":
    main()
