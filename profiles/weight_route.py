#!/usr/bin/env python3
"""What a handle computes after HOST-set weights (lrp_set_weight), as SHA-256 digests, and what setting them costs.

  weight_route.py digests          one line per output: features, heat-maps (bf16x3 and fp32), decoder LRP, decoder
                                   gradient and the fine-tune step's first gradients of the VGG handle with both decoders;
                                   features / heat-maps / decoder outputs of a ResNet handle at widths % 32 == 0 and != 0;
                                   lrp_op_conv (fp32 and split-bf16, the N == 64 nine-tap backward conv among them),
                                   lrp_op_conv_pool_sparse and lrp_op_epsilon_dense.  Fixed seeds: two builds of the
                                   library pack the weights identically iff every line is equal.
  weight_route.py startup vgg      wall time of set_weights() for the full-size VGG16 + adaptive decoder bundle
  weight_route.py startup resnet   ... for the ResNet-101 + grid-TD bundle (run each in fresh processes)

Listings of the commit that retired the host packers and of its parent: weight_route.txt."""
import hashlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def vgg_digests(kind):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, gridtd_weights, vgg_weights
    cfg = [("c1", 3, 64, False), ("c2", 64, 64, True), ("c3", 64, 128, True), ("c4", 128, 32, False)]   # c2, c3: cin <= 64 (fragment-major copies)
    hw, L, D, H, V = 16, 16, 32, 32, 40
    rs = np.random.RandomState(12)
    w = vgg_weights(rs, cfg, bias_std=0.3)
    w.update((adaptive_weights if kind == "adaptive" else gridtd_weights)(rs, L, D, H, H, V))
    kw = dict(decoder=kind, cnn_cfg=cfg, img_hw=(hw, hw), L=L, D=D, H=H, E=H, V=V, max_images=2, max_tokens=6, max_caption_len=5)
    X = rs.uniform(-120, 130, size=(2, hw, hw, 3)).astype(np.float32)
    caps = [[5, 9, 17, 1], [8, 3, 1]]
    idx, tpos = [0, 0, 0, 1, 1], [1, 2, 3, 1, 2]
    eng = LRPEngine(**kw)
    eng.set_weights(w)
    for prec in ("bf16x3", "fp32"):
        eng.set_precision(prec)
        eng.encode_images(X)
        eng.decoder_forward(caps)
        out, R, att, rw = eng.explain_tokens(idx, tpos, want_R_feat=True, want_attention=True, want_r_words=True)
        print("vgg_%s features_%s %s" % (kind, prec, sha(eng.get_features())))
        print("vgg_%s heatmaps_%s %s" % (kind, prec, sha(out)))
        print("vgg_%s decoder_lrp_%s %s" % (kind, prec, sha(R, att, rw)))
    d, drw = eng.decoder_gradient(idx, tpos)
    print("vgg_%s decoder_gradient %s" % (kind, sha(d, drw)))
    print("vgg_%s cnn_gradient_walk %s" % (kind, sha(eng.cnn_walk(idx, d, "gradient"))))
    fresh = LRPEngine(**kw)
    fresh.set_weights(w)
    cap_in = np.array([[1, 4, 8, 16], [1, 7, 2, 0]], dtype=np.int32)
    y = np.array([[4, 8, 16, 0], [7, 2, 0, -1]], dtype=np.int32)
    lw = (1 + rs.uniform(0, 1, size=(2, 4, V))).astype(np.float32)
    fresh.train_begin(lr=1e-3)
    fresh.encode_images(X)
    g, l = fresh.train_step(cap_in, y, lw)
    g, l = g.clone(), l.clone()
    fresh.train_apply(g)
    fresh.encode_images(X)
    g2, l2 = fresh.train_step(cap_in, y, lw)
    print("vgg_%s train_first_gradients %s" % (kind, sha(g, l)))
    print("vgg_%s train_second_gradients %s" % (kind, sha(g2, l2)))


def resnet_digests(tag, stacks, stem, hw):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import gridtd_weights, resnet_weights
    rs = np.random.RandomState(8)
    w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
    H, V = 32, 50
    side = hw // 4 // (2 ** (len(stacks) - 1))
    L, D = side * side, 4 * stacks[-1][0]
    w.update(gridtd_weights(rs, L, D, H, H, V))
    X = rs.uniform(-120, 130, size=(2, hw, hw, 3)).astype(np.float32)
    eng = LRPEngine(decoder="gridtd", img_hw=(hw, hw), L=L, D=D, H=H, E=H, V=V, max_images=2, max_tokens=6, max_caption_len=6,
                    resnet={"stem": stem, "stacks": stacks})
    eng.set_weights(w)
    caps = [[7, 19, 33, 1], [8, 3, 1]]
    idx, tpos = [0, 0, 0, 1, 1], [1, 2, 3, 1, 2]
    for prec in ("bf16x3", "fp32"):
        eng.set_precision(prec)
        eng.encode_images(X)
        eng.decoder_forward(caps)
        out, R, att, rw = eng.explain_tokens(idx, tpos, want_R_feat=True, want_attention=True, want_r_words=True)
        print("resnet_%s features_%s %s" % (tag, prec, sha(eng.get_features())))
        print("resnet_%s heatmaps_%s %s" % (tag, prec, sha(out)))
        print("resnet_%s decoder_lrp_%s %s" % (tag, prec, sha(R, att, rw)))
    d, drw = eng.decoder_gradient(idx, tpos)
    print("resnet_%s decoder_gradient %s" % (tag, sha(d, drw)))


def op_digests():
    import torch
    from lrp_imagecaptioning_amd.engine import op_conv, op_conv_pool_sparse, op_epsilon_dense
    rs = np.random.RandomState(5)
    for name, NB, Hh, Ww, Cin, Cout, taps in [("9tap_64_to_128", 2, 12, 10, 64, 128, 9), ("9tap_40_to_24", 2, 9, 7, 40, 24, 9),
                                              ("1tap_96_to_72", 3, 6, 5, 96, 72, 1)]:
        w = (rs.standard_normal((3 if taps == 9 else 1,) * 2 + (Cin, Cout)) / np.sqrt(taps * Cin)).astype(np.float32)
        b = rs.standard_normal(Cout).astype(np.float32)
        x = torch.as_tensor(rs.standard_normal((NB, Hh, Ww, Cin)).astype(np.float32)).cuda()
        s = torch.as_tensor(rs.standard_normal((NB, Hh, Ww, Cout)).astype(np.float32)).cuda()
        gate = torch.as_tensor(rs.uniform(0, 1, size=(NB, Hh, Ww, Cin)).astype(np.float32)).cuda()
        gate_up = torch.as_tensor(rs.uniform(0, 1, size=(NB, 2 * Hh, 2 * Ww, Cin)).astype(np.float32)).cuda()
        for split in (False, True):
            p = "bf16x3" if split else "fp32"
            if not split:
                print("op_conv %s relu_%s %s" % (name, p, sha(op_conv(x, w, b, None, 0, taps))))
            print("op_conv %s forward_%s %s" % (name, p, sha(op_conv(x, w, b, None, 1, taps, split_bf16=split))))
            # (Cin == 64, nine taps, split: the weights-in-registers backward conv and its fragment-major operand)
            print("op_conv %s backward_%s %s" % (name, p, sha(op_conv(s, w, None, gate, 2, taps, split_bf16=split))))
            if taps == 9:
                print("op_conv %s backward_up2_%s %s" % (name, p, sha(op_conv(s, w, None, gate_up, 3, taps, split_bf16=split))))
    NB, Hp, Wp, Cin, Cout = 2, 7, 5, 256, 32
    sc = torch.as_tensor(rs.standard_normal((NB, Hp, Wp, Cout)).astype(np.float32)).cuda()
    pos = torch.as_tensor(rs.randint(0, 4, size=(NB, Hp, Wp, Cout)).astype(np.uint8)).cuda()
    w = np.abs(rs.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cout)).astype(np.float32)
    gate = torch.as_tensor(rs.uniform(0, 1, size=(NB, 2 * Hp, 2 * Wp, Cin)).astype(np.float32)).cuda()
    print("op_conv_pool_sparse 256x32 %s" % sha(op_conv_pool_sparse(sc, pos, w, gate)))
    N, Din, Dout = 6, 40, 28
    xd = torch.as_tensor(rs.standard_normal((N, Din)).astype(np.float32)).cuda()
    W = rs.standard_normal((Din, Dout)).astype(np.float32)
    R = torch.as_tensor(rs.standard_normal((N, Dout)).astype(np.float32)).cuda()
    print("op_epsilon_dense 40x28 %s" % sha(op_epsilon_dense(xd, W, R, 1e-3)))


def startup(which):
    import torch
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import RESNET101_STACKS, adaptive_weights, gridtd_weights, resnet_weights, vgg_weights
    V = 10000
    rs = np.random.RandomState(0)
    if which == "vgg":
        w = vgg_weights(rs)
        w.update(adaptive_weights(rs, 196, 512, 512, 512, V))
        eng = LRPEngine(decoder="adaptive", V=V, max_images=1, max_tokens=4, max_caption_len=11)
    else:
        w = resnet_weights(rs)
        w.update(gridtd_weights(rs, 49, 2048, 512, 512, V))
        eng = LRPEngine(decoder="gridtd", img_hw=(224, 224), L=49, D=2048, H=512, E=512, V=V, max_images=1, max_tokens=4,
                        max_caption_len=11, resnet={"stem": 64, "stacks": RESNET101_STACKS})
    torch.cuda.synchronize()
    t = time.perf_counter()
    eng.set_weights(w)
    torch.cuda.synchronize()
    print("startup %s set_weights_ms %.1f workspace_bytes %d" % (which, (time.perf_counter() - t) * 1e3, eng.workspace_bytes))


if __name__ == "__main__":
    if sys.argv[1:2] == ["startup"]:
        startup(sys.argv[2])
    else:
        for kind in ("adaptive", "gridtd"):
            vgg_digests(kind)
        resnet_digests("w32", ((32, 2), (64, 2)), 32, 64)
        resnet_digests("w8", ((8, 2), (16, 3), (32, 2)), 16, 64)
        op_digests()
