#!/usr/bin/env python3
"""Does a build compute what another computes under the conv rules of the VGG walk?  What profiles/rule_merge_bitexact.txt records.

One row per case: SHA-256 (first 24 hex digits) of the heat-maps, taken over `out + 0.0` so that the sign of a zero does not count,
and the lrp_launch_count delta of the encode (the first one after the rule was set: it packs the rule's matrices) and of the
cnn_explain.  Run it on two builds and diff the tables:

  python profiles/rule_merge_bitexact.py [--lib PATH/liblrp_hip.so] > table.txt

Cases, on the TINY (16 x 16, B = 3) and MID (32 x 32, B = 2) nets of tests/rule_table_cases.py, two maps per image:
  rules (2, 1) and (1.5, 0.5) in fp32, bf16x3 and bf16x3_fast; (2, 1) under LRP_IMG_FUSED=0, LRP_FWD_EMIT=0, LRP_FWD_IL=0 and
  LRP_POOL_FUSED=0 (weights uploaded under the switch); (2, 1) after a fine-tune step (train_step, train_apply, encode; the handle
  gets a decoder's weights for it); the default rule in bf16x3; the tables mixed_ab, presetBflat and a2b1_bounded in bf16x3;
  lrp_op_conv_ab on the 3 x 14 x 14, 128 -> 128 shape of tests/conv_rule_cases.py, with and without pool and split."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def digest(t):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy() + 0.0).tobytes()).hexdigest()[:24]


def main():
    from lrp_imagecaptioning_amd import _capi
    if "--lib" in sys.argv:
        _capi.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    import numpy as np
    import torch
    import rule_table_cases as K
    from lrp_imagecaptioning_amd.engine import LRPEngine, op_conv_ab, switches
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights
    lib = _capi.load()

    def engine(net, prec, w):
        cfg, hw, B = K.NETS[net]
        side = hw
        for _, _, _, p in cfg:
            side = side // 2 if p else side
        eng = LRPEngine(decoder="adaptive", cnn_cfg=cfg, img_hw=(hw, hw), L=side * side, D=cfg[-1][2], H=32, E=32, V=50, max_images=B,
                        max_tokens=2 * B, max_caption_len=6)
        eng.set_weights(w)
        eng.set_precision(prec)
        return eng

    def counted(fn):
        n0 = int(lib.lrp_launch_count())
        out = fn()
        torch.cuda.synchronize()
        return out, int(lib.lrp_launch_count()) - n0

    def row(name, eng, X, idx, R):
        _, n_enc = counted(lambda: eng.encode_images(X))
        out, n_exp = counted(lambda: eng.cnn_explain(list(idx), R))
        assert bool(torch.isfinite(out).all()), name
        print("%-44s %s %3d %3d" % (name, digest(out), n_enc, n_exp), flush=True)

    print("# case                                       sha256(heat-maps)[:24] encode_launches explain_launches")
    for net in ("tiny", "mid"):
        w, X, idx, R, _ = K.net(net)
        for rule in ((2, 1), (1.5, 0.5)):
            for prec in ("fp32", "bf16x3", "bf16x3_fast"):
                eng = engine(net, prec, w)
                eng.set_cnn_rule(*rule)
                row("%s_%s_rule_%g_%g" % (net, prec, rule[0], rule[1]), eng, X, idx, R)
        for sw in ("LRP_IMG_FUSED", "LRP_FWD_EMIT", "LRP_FWD_IL", "LRP_POOL_FUSED"):
            with switches(**{sw: 0}):
                eng = engine(net, "bf16x3", w)
                eng.set_cnn_rule(2, 1)
                row("%s_bf16x3_rule_2_1_%s=0" % (net, sw), eng, X, idx, R)
        # (2, 1) after a fine-tune step: the rule's matrices come from the step's master buffer
        cfg, hw, B = K.NETS[net]
        L, D, H, V, Tn = R.shape[1] * R.shape[2], R.shape[3], 32, 50, 5
        rs = np.random.RandomState(3)
        wd = dict(w)
        wd.update(adaptive_weights(rs, L, D, H, H, V))
        y = rs.randint(2, V, size=(B, Tn)).astype(np.int32)
        cap_in = np.concatenate([np.ones((B, 1), np.int32), y[:, :-1]], axis=1)
        lw = np.ones((B, Tn, V), np.float32)
        eng = engine(net, "bf16x3", wd)
        eng.set_cnn_rule(2, 1)
        eng.train_begin(lr=1e-3, clipvalue=0.01)
        eng.encode_images(X)
        grads, _ = eng.train_step(cap_in, y, lw, None)
        eng.train_apply(grads)
        row("%s_bf16x3_rule_2_1_after_train_apply" % net, eng, X, idx, R)
        row("%s_bf16x3_default" % net, engine(net, "bf16x3", w), X, idx, R)
        for name in ("mixed_ab", "presetBflat", "a2b1_bounded"):
            eng = engine(net, "bf16x3", w)
            eng.set_cnn_rules(K.table(name))
            row("%s_bf16x3_table_%s" % (net, name), eng, X, idx, R)
    print("# lrp_op_conv_ab                             sha256(out+)[:24] sha256(out-)[:24] launches")
    NB, H, W, Cin, Cout = 3, 14, 14, 128, 128
    for pool in (False, True):
        for split in (False, True):
            rs = np.random.RandomState(11)
            u = 2 if pool else 1
            sp, sn = (torch.as_tensor(rs.standard_normal((NB, H, W, Cout)).astype(np.float32)).cuda() for _ in range(2))
            wk = (rs.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32)
            gp, gn = (torch.as_tensor((s * rs.uniform(size=(NB, u * H, u * W, Cin)) * (rs.uniform(size=(NB, u * H, u * W, Cin)) >= 0.125))
                                      .astype(np.float32)).cuda() for s in (1.0, -2.0))
            (op, on), n = counted(lambda: op_conv_ab(sp, sn, wk, 2.0, 1.0, gp, gn, pool=pool, split_bf16=split))
            print("%-44s %s %s %3d" % ("op_conv_ab_%s_%s" % ("up2" if pool else "mul", "split" if split else "fp32"), digest(op), digest(on), n),
                  flush=True)


if __name__ == "__main__":
    main()
