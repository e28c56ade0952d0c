"""-m gpu: the alpha-beta conv rule with beta > 0 (lrp_set_cnn_rule; LRPAlphaBeta / LRPAlpha2Beta1 / LRPSequentialPresetB) —
the two-chain launch at operator level (lrp_op_conv_ab, every case of tests/conv_ab_cases.py), the walk against the float64
restatement of RR:274-322 (tests/alphabeta_ref.py), beta = 0 as the unchanged alpha1beta0 path, batch invariance, properties
that need no oracle, and the Python surface.

Bounds.  Operator: gpu_util.elem_ratio under gpu_util.elem_bar of torch's float32 evaluation (the project's derived operator
bar).  Walk: relative L1 per map < 1e-4 (BASELINE.json's bar; the float32 evaluation of the restatement itself is 1.2e-7 ...
6.3e-7 per map from its float64 evaluation on the TINY / MID draws used here and 1.3e-7 ... 4.9e-7 on WIDE, seed 7,
profiles/alphabeta.txt; the smallest |Z_act|, |Z_inh| of these draws is 2.3e-2, on WIDE) and the worst row / column band under
gpu_util.band_bar of that float32 evaluation."""
import functools

import numpy as np
import pytest
import torch

import alphabeta_ref as AB
import conv_ab_cases as T
from conftest import rel_l1
from gpu_util import NONSQUARE_RESNETS, band_bar, band_rel_l1, elem_bar, elem_ratio, report
from lrp_imagecaptioning_amd.synthetic import adaptive_weights, vgg_weights
from oracle import cnn_lrp_ref as C

pytestmark = pytest.mark.gpu

TINY_CFG = [("c1", 3, 8, False), ("c2", 8, 8, True), ("c3", 8, 16, False), ("c4", 16, 16, True), ("c5", 16, 16, False)]
MID_CFG = [("c1", 3, 64, False), ("c2", 64, 64, True), ("c3", 64, 128, True), ("c4", 128, 256, False), ("c5", 256, 128, False)]
WIDE_CFG = [("c1", 3, 64, False), ("c2", 64, 64, True), ("c3", 64, 128, False), ("c4", 128, 128, True), ("c5", 128, 256, False),
            ("c6", 256, 512, True), ("c7", 512, 512, False)]
NETS = {"tiny": (TINY_CFG, 16, 3), "mid": (MID_CFG, 32, 2), "wide": (WIDE_CFG, 32, 2)}
RULES = ((2, 1), (1.5, 0.5))
RESIDENT_SET = {"LRP_CONV_SMALL": 0, "LRP_CONV_MID": 0, "LRP_CONV_HALO": 2}


# ---------------------------------------------------------------- operator
@pytest.mark.parametrize("pool", (False, True), ids=("mul", "up2"))
@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_op_conv_ab_against_float64(case, pool):
    from lrp_imagecaptioning_amd.engine import op_conv_ab, switches
    c = case
    alpha, beta = (1.5, 0.5) if pool else (2, 1)
    rs = np.random.RandomState(sum(c[:5]) + int(pool))
    u = 2 if pool else 1
    sp = torch.as_tensor(rs.standard_normal((c.NB, c.H, c.W, c.Cout)).astype(np.float32)).cuda()
    sn = torch.as_tensor(rs.standard_normal((c.NB, c.H, c.W, c.Cout)).astype(np.float32)).cuda()
    w = (rs.standard_normal((3, 3, c.Cin, c.Cout)) / np.sqrt(9 * c.Cin)).astype(np.float32)
    g = torch.Generator(device="cuda").manual_seed(int(rs.randint(1 << 30)))
    shape = (c.NB, u * c.H, u * c.W, c.Cin)
    gp = torch.rand(shape, device="cuda", generator=g) * (torch.rand(shape, device="cuda", generator=g) >= 0.125)
    gn = -2.0 * torch.rand(shape, device="cuda", generator=g) * (torch.rand(shape, device="cuda", generator=g) >= 0.125)
    with switches(**c.switches):
        p = T.op_plan(c, pool)
        assert p["ok"] == 1 and (T.FORM_NAMES[p["form"]], (p["BM"], p["BN"])) == (c.form, tuple(c.tile)), (T.plan_name(p), c)
        outs = op_conv_ab(sp, sn, w, alpha, beta, gp, gn, pool=pool, split_bf16=c.split)
    refs = AB.op_conv_ab_ref(sp, sn, w, alpha, beta, gp, gn, pool, torch.float64)
    # the mass each element was summed from: |gate| x (|S+| convT alpha |w+| + |S-| convT beta |w-|)
    w64 = torch.as_tensor(w).double().cuda().permute(3, 2, 0, 1)
    cm = (torch.nn.functional.conv_transpose2d(sp.double().abs().permute(0, 3, 1, 2), alpha * w64.clamp(min=0), padding=1)
          + torch.nn.functional.conv_transpose2d(sn.double().abs().permute(0, 3, 1, 2), beta * (-w64).clamp(min=0), padding=1))
    if pool:
        cm = torch.nn.functional.interpolate(cm, scale_factor=2, mode="nearest")
    cm = cm.permute(0, 2, 3, 1)
    mags = (cm * gp.double().abs(), cm * gn.double().abs())
    r32s = AB.op_conv_ab_ref(sp.cpu(), sn.cpu(), w, alpha, beta, gp.cpu(), gn.cpu(), pool, torch.float32)
    for name, out, ref, mag, r32t, gate in zip(("out+", "out-"), outs, refs, mags, r32s, (gp, gn)):
        assert out.shape == ref.shape and bool(torch.isfinite(out).all())
        r32 = elem_ratio(r32t.cuda(), ref, mag)
        bar = elem_bar(r32, c.split)
        ratio = elem_ratio(out, ref, mag)
        err = float((out.double() - ref).abs().sum() / ref.abs().sum())
        report("conv_ab", case=T.case_id(c), pool=pool, which=name, plan=T.plan_name(p), ratio=ratio, r32=r32, bar=bar, rel_l1=err)
        print("%s %s %s: ratio %.3e r32 %.3e bar %.3e rel_l1 %.3e" % (T.case_id(c), "up2" if pool else "mul", name, ratio, r32, bar, err))
        assert bool((out[gate == 0] == 0).all())                       # a zero gate gives an exact zero
        assert ratio < bar, (name, ratio, r32, bar)


# ---------------------------------------------------------------- walk parity
@functools.lru_cache(maxsize=None)
def _net(name, bias_std=0.3, seed=7):
    """weights, images, interleaved token -> image map, relevance maps, layers: computed once per net"""
    cfg, hw, B = NETS[name]
    rs = np.random.RandomState(seed)
    w = vgg_weights(rs, cfg, bias_std=bias_std)
    layers = C.vgg_layers(w, cfg)
    X = rs.uniform(-120, 130, size=(B, hw, hw, 3)).astype(np.float32)
    feat = C.forward(layers, X)
    idx = [b for b in range(B)] + [B - 1 - b for b in range(B)]
    R = (rs.standard_normal((2 * B,) + feat.shape[1:]) * feat[idx]).astype(np.float32)
    return w, X, tuple(idx), R, layers


@functools.lru_cache(maxsize=None)
def _refs(name, rule):
    """(float64, float32) restatement for the net's tokens under `rule`: computed once, never written to"""
    w, X, idx, R, layers = _net(name)
    Xi = X[list(idx)]
    r64, r32 = AB.analyze(layers, Xi, R, *rule), AB.analyze(layers, Xi, R, *rule, dtype=torch.float32)
    r64.setflags(write=False); r32.setflags(write=False)
    return r64, r32


def _engine(cfg, hw, B, ntok, w, prec="bf16x3", rule=None):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    side = hw
    for _, _, _, p in cfg:
        side = side // 2 if p else side
    eng = LRPEngine(decoder="adaptive", cnn_cfg=cfg, img_hw=(hw, hw), L=side * side, D=cfg[-1][2], H=32, E=32, V=50,
                    max_images=B, max_tokens=ntok, max_caption_len=4)
    eng.set_weights(w)
    eng.set_precision(prec)
    if rule is not None:
        eng.set_cnn_rule(*rule)
    return eng


def _walk_parity(name, prec, rule, tag):
    cfg, hw, B = NETS[name]
    w, X, idx, R, layers = _net(name)
    eng = _engine(cfg, hw, B, 2 * B, w, prec, rule)
    eng.encode_images(X)
    out = eng.cnn_explain(list(idx), R).cpu().numpy()
    ref, ref32 = _refs(name, rule)
    errs = [rel_l1(out[i], ref[i]) for i in range(2 * B)]
    own = max(rel_l1(ref32[i], ref[i]) for i in range(2 * B))
    bar, band32 = band_bar(ref32, ref)
    band = max(band_rel_l1(out[i], ref[i], where=True) for i in range(2 * B))
    report("alphabeta_%s_%s_%g_%g%s" % (name, prec, rule[0], rule[1], tag), max_rel_l1=max(errs), f32_restatement_rel_l1=own,
           worst_band=band[0], worst_band_at=band[1], f32_restatement_band=band32, band_bar=bar)
    print("%s %s %s%s: rel_l1 %.3e (float32 restatement %.3e) band %.3e at %s bar %.3e" % (name, prec, rule, tag, max(errs), own, band[0],
                                                                                           band[1], bar))
    assert np.isfinite(out).all()
    assert max(errs) < 1e-4, errs
    assert band[0] < bar, (band, bar)


@pytest.mark.parametrize("rule", RULES, ids=("a2b1", "a1.5b0.5"))
@pytest.mark.parametrize("prec", ("fp32", "bf16x3"))
@pytest.mark.parametrize("name", ("tiny", "mid", "wide"))
def test_walk_matches_restatement(name, prec, rule):
    _walk_parity(name, prec, rule, "")


@pytest.mark.parametrize("name", ("tiny", "mid", "wide"))
def test_walk_matches_restatement_on_the_resident_image_tile(name):
    from lrp_imagecaptioning_amd.engine import switches
    with switches(**RESIDENT_SET):
        _walk_parity(name, "bf16x3", (2, 1), "_resident")


@pytest.mark.parametrize("env,prec", [({"LRP_IMG_FUSED": 0}, "bf16x3"), ({"LRP_IMG_FUSED": 0}, "fp32"), ({"LRP_FWD_EMIT": 0}, "bf16x3"),
                                      ({"LRP_FWD_IL": 0}, "bf16x3"), ({"LRP_POOL_FUSED": 0}, "bf16x3"), ({}, "bf16x3_fast")],
                         ids=("img_unfused-bf16x3", "img_unfused-fp32", "fwd_emit0", "fwd_il0", "pool_fused0", "forward_fast"))
def test_walk_behind_the_other_forwards_and_the_unfused_image_layer(env, prec):
    # the inhibitor pass reads what each forward of Encoder::encode leaves (bf16x3_fast: the gates come from the side stream, the
    # pass waits for them); the image layer as GEMM + stencil kernel (K = 128)
    from lrp_imagecaptioning_amd.engine import switches
    with switches(**env):
        _walk_parity("mid", prec, (2, 1), "_" + "_".join("%s=%s" % kv for kv in env.items()))


def test_fine_tune_step_rebuilds_the_rule_matrices():
    # lrp_train_apply repacks every conv from the master buffer: under a beta > 0 rule the two-chain matrices follow
    import test_gpu_train as TT
    w, X, cap_in, y, lw, masks = TT._case(3)
    eng = TT._engine(w, len(X))
    eng.set_cnn_rule(2, 1)
    eng.train_begin(lr=1e-3, clipvalue=0.01)
    eng.encode_images(X)
    grads, _ = eng.train_step(cap_in, y, lw, masks)
    eng.train_apply(grads)
    new = eng.train_weights()
    wn = {k: new[k].reshape(np.shape(w[k])) for k in w}
    layers = C.vgg_layers(wn, TT.CFG)
    eng.encode_images(X)
    feat = C.forward(layers, X)
    R = (np.random.RandomState(0).standard_normal(feat[:2].shape) * feat[:2]).astype(np.float32)
    got = eng.cnn_explain([0, 1], R).cpu().numpy()
    want = AB.analyze(layers, X[:2], R, 2, 1)
    assert max(rel_l1(got[i], want[i]) for i in range(2)) < 1e-4
    moved = AB.analyze(C.vgg_layers(w, TT.CFG), X[:2], R, 2, 1)
    assert rel_l1(got[0], moved[0]) > 1e-3                    # (the update is visible at this bound)
    # a rule change after the step has released the layers' own HWIO copies: the matrices come from the step's master buffer
    eng.set_cnn_rule(1.5, 0.5)
    eng.encode_images(X)
    got = eng.cnn_explain([0, 1], R).cpu().numpy()
    want = AB.analyze(layers, X[:2], R, 1.5, 0.5)
    assert max(rel_l1(got[i], want[i]) for i in range(2)) < 1e-4


def test_rule_off_leaves_the_fine_tune_step_its_activations():
    # rule (2,1) -> train_begin -> rule (1,0): both asked for the kept layer inputs, and the rule giving them up must not take
    # them from the step — its gradients on a NEW batch equal those of a handle that never set the rule, bit for bit
    import test_gpu_train as TT
    w, X, cap_in, y, lw, masks = TT._case(3)
    _, X2, cap2, y2, lw2, masks2 = TT._case(4)
    ref = TT._engine(w, len(X))
    ref.train_begin(lr=1e-3, clipvalue=0.01)
    ref.encode_images(X)
    ref.train_step(cap_in, y, lw, masks)
    ref.encode_images(X2)
    g_ref, l_ref = ref.train_step(cap2, y2, lw2, masks2)
    g_ref, l_ref = g_ref.clone(), l_ref.clone()
    eng = TT._engine(w, len(X))
    eng.set_cnn_rule(2, 1)
    eng.train_begin(lr=1e-3, clipvalue=0.01)
    eng.encode_images(X)
    eng.train_step(cap_in, y, lw, masks)
    eng.set_cnn_rule(1, 0)
    eng.encode_images(X2)
    g, l = eng.train_step(cap2, y2, lw2, masks2)
    assert float(g_ref.abs().sum()) > 0
    assert torch.equal(g, g_ref) and torch.equal(l, l_ref)
    # ... and the other order: the step first, then the rule on and off
    eng.set_cnn_rule(2, 1)
    eng.encode_images(X)
    eng.set_cnn_rule(1, 0)
    eng.encode_images(X2)
    g, l = eng.train_step(cap2, y2, lw2, masks2)
    assert torch.equal(g, g_ref) and torch.equal(l, l_ref)


# ---------------------------------------------------------------- beta = 0 is the old path
def test_beta_zero_is_preset_a_bit_for_bit():
    from lrp_imagecaptioning_amd.analyzer import ImageModelSpec, LRPAlpha1Beta0, LRPAlphaBeta, LRPSequentialPresetA
    w, X, idx, R, _ = _net("mid")
    Xi, spec = X[list(idx)], ImageModelSpec(w, MID_CFG, (32, 32))
    base = LRPSequentialPresetA(spec, max_batch=4).analyze([Xi, R])
    assert np.array_equal(LRPAlphaBeta(spec, alpha=1, beta=0, max_batch=4).analyze([Xi, R]), base)
    assert np.array_equal(LRPAlpha1Beta0(spec, max_batch=4).analyze([Xi, R]), base)
    assert np.array_equal(LRPAlphaBeta(spec, beta=0, max_batch=4).analyze([Xi, R]), base)


def test_rule_round_trip_state_and_workspace():
    w, X, idx, R, _ = _net("mid")
    fresh = _engine(MID_CFG, 32, 2, 4, w)
    fresh.encode_images(X)
    base = fresh.cnn_explain(list(idx), R).cpu().numpy()
    eng = _engine(MID_CFG, 32, 2, 4, w)
    ws0 = eng.workspace_bytes
    assert ws0 == fresh.workspace_bytes
    eng.set_cnn_rule(1, 0)                                   # the default again: nothing allocated, nothing dropped
    assert eng.workspace_bytes == ws0
    eng.encode_images(X)
    eng.set_cnn_rule(1, 0)
    assert np.array_equal(eng.cnn_explain(list(idx), R).cpu().numpy(), base)
    eng.set_cnn_rule(2, 1)
    assert eng.workspace_bytes > ws0
    with pytest.raises(RuntimeError):
        eng.cnn_explain(list(idx), R)                         # LRP_ERR_STATE until the next encode
    eng.encode_images(X)
    out21 = eng.cnn_explain(list(idx), R).cpu().numpy()
    assert not np.array_equal(out21, base)
    ws1 = eng.workspace_bytes
    eng.set_cnn_rule(1, 0)
    with pytest.raises(RuntimeError):
        eng.cnn_explain(list(idx), R)
    eng.encode_images(X)
    assert np.array_equal(eng.cnn_explain(list(idx), R).cpu().numpy(), base)
    eng.set_cnn_rule(2, 1)                                    # the buffers are there already
    assert eng.workspace_bytes == ws1
    eng.encode_images(X)
    assert np.array_equal(eng.cnn_explain(list(idx), R).cpu().numpy(), out21)
    # the gradient walks ignore the rule
    g21 = eng.cnn_walk(list(idx), R, "gradient").cpu().numpy()
    assert np.array_equal(g21, fresh.cnn_walk(list(idx), R, "gradient").cpu().numpy())


# ---------------------------------------------------------------- batch invariance
@pytest.mark.parametrize("prec", ("fp32", "bf16x3"))
def test_batch_invariance(prec):
    w, X, idx, R, _ = _net("mid")
    one = _engine(MID_CFG, 32, 1, 1, w, prec, (2, 1))
    one.encode_images(X[1:2])
    alone = one.cnn_explain([0], R[0:1] * 0 + R[1:2]).cpu().numpy()
    many = _engine(MID_CFG, 32, 2, 5, w, prec, (2, 1))
    many.encode_images(X)
    Rs = np.stack([R[0], R[2], R[3], R[1], R[0]])
    out = many.cnn_explain([0, 1, 0, 1, 0], Rs).cpu().numpy()
    assert np.array_equal(out[3], alone[0])


# ---------------------------------------------------------------- properties that need no oracle
@pytest.mark.parametrize("prec", ("fp32", "bf16x3"))
def test_linearity_in_R(prec):
    w, X, idx, R, _ = _net("mid")
    eng = _engine(MID_CFG, 32, 2, 4, w, prec, (2, 1))
    eng.encode_images(X)
    out = eng.cnn_explain([0, 0], R[[0, 3]]).cpu().numpy()              # tokens 0 and 3 both belong to image 0
    out2 = eng.cnn_explain([0], (2.5 * R[0] + R[3])[None]).cpu().numpy()
    assert rel_l1(out2[0], 2.5 * out[0] + out[1]) < (1e-5 if prec == "fp32" else 5e-5)


@pytest.mark.parametrize("rule", RULES, ids=("a2b1", "a1.5b0.5"))
def test_conservation_without_biases(rule):
    w, X, idx, R, _ = _net("mid")
    w = {k: (np.zeros_like(v) if k.endswith("_b") else v) for k, v in w.items()}
    eng = _engine(MID_CFG, 32, 2, 4, w, "fp32", rule)
    eng.encode_images(X)
    out = eng.cnn_explain(list(idx), R).cpu().numpy().astype(np.float64)
    for i in range(len(R)):
        assert abs(out[i].sum() - R[i].astype(np.float64).sum()) <= 1e-4 * np.abs(out[i]).sum()


@pytest.mark.parametrize("prec", ("fp32", "bf16x3"))
def test_no_inhibitor_where_z_inh_is_zero(prec):
    # nonnegative weights, zero biases, nonnegative image: Z_inh == 0, S- = R / 1e-7 everywhere, and it must meet only zero weights
    w, X, idx, R, _ = _net("mid")
    w = {k: (np.abs(v) if k.endswith("_W") else np.zeros_like(v)) for k, v in w.items()}
    X = np.abs(X)
    a = _engine(MID_CFG, 32, 2, 4, w, prec)
    a.encode_images(X)
    base = a.cnn_explain(list(idx), R).cpu().numpy()
    b = _engine(MID_CFG, 32, 2, 4, w, prec, (2, 1))
    b.encode_images(X)
    out = b.cnn_explain(list(idx), R).cpu().numpy()
    assert np.isfinite(out).all()
    for i in range(len(R)):
        assert rel_l1(out[i], 2.0 ** len(MID_CFG) * base[i]) < 1e-6


# ---------------------------------------------------------------- surface
def test_preset_b_is_alpha2beta1():
    from lrp_imagecaptioning_amd.analyzer import ImageModelSpec, LRPAlpha2Beta1, LRPSequentialPresetB
    w, X, idx, R, _ = _net("tiny")
    Xi, spec = X[list(idx)], ImageModelSpec(w, TINY_CFG, (16, 16))
    b = LRPSequentialPresetB(spec, epsilon=0.01, max_batch=4).analyze([Xi, R])      # 6 maps, max_batch 4: two chunks
    assert np.array_equal(b, LRPAlpha2Beta1(spec, max_batch=4).analyze([Xi, R]))
    ref, _ = _refs("tiny", (2, 1))
    assert max(rel_l1(b[i], ref[i]) for i in range(len(R))) < 1e-4
    with pytest.raises(ValueError):
        LRPSequentialPresetB(spec, epsilon=0)


def test_explainer_follows_the_spec_rule():
    from lrp_imagecaptioning_amd.explainers import CaptionModelSpec, ExplainImgCaptioningAdaptiveAttention
    CFG = [("c1", 3, 8, False), ("c2", 8, 8, True), ("c3", 8, 16, True), ("c4", 16, 16, False)]
    HW, L, D, H, V = 16, 16, 16, 32, 40
    rs = np.random.RandomState(0)
    w = vgg_weights(rs, CFG, bias_std=0.3)
    w.update(adaptive_weights(rs, L, D, H, H, V))
    X = rs.uniform(-120, 130, size=(1, HW, HW, 3)).astype(np.float32)
    cap = [7, 12, 33, 5, 1]
    kw = dict(img_encoder="vgg16", hidden_dim=H, embedding_dim=H, L=L, D=D, vocab_size=V, cnn_cfg=CFG, img_hw=(HW, HW))
    ex = ExplainImgCaptioningAdaptiveAttention(CaptionModelSpec(w, cnn_rule="alpha2beta1", **kw), None, None, max_caption_length=8)
    ex0 = ExplainImgCaptioningAdaptiveAttention(CaptionModelSpec(w, **kw), None, None, max_caption_length=8)
    assert ex._engine.cnn_rule == (2, 1) and ex0._engine.cnn_rule == (1, 0)
    from lrp_imagecaptioning_amd.explainers import ExplainImgCaptioningAdaptiveAttentionGradient
    exg = ExplainImgCaptioningAdaptiveAttentionGradient(CaptionModelSpec(w, cnn_rule="alpha2beta1", **kw), None, None, max_caption_length=8)
    assert exg._engine.cnn_rule == (1, 0) and exg._engine.workspace_bytes == ex0._engine.workspace_bytes    # gradient walks ignore the rule
    del exg
    ex._forward_beam_search((None, X), cap)
    ex0._forward_beam_search((None, X), cap)
    rel, _ = ex._explain_sentence()
    layers = C.vgg_layers(w, CFG)
    for i, R in enumerate(rel):
        R1, a1 = ex._explain_lstm_single_word_sequence(i + 1)
        R0, a0 = ex0._explain_lstm_single_word_sequence(i + 1)
        assert np.array_equal(R1, R0) and np.array_equal(a1, a0)          # the decoder half does not see the rule
        img = ex._explain_CNN(X, R)
        direct = ex._engine.cnn_explain([0], R.reshape(1, L, D)).cpu().numpy()
        assert np.array_equal(img, direct.reshape(img.shape))
        assert rel_l1(img, AB.analyze(layers, X, R, 2, 1)) < 1e-4
        assert not np.array_equal(img, ex0._explain_CNN(X, R))


def test_unsupported_and_invalid():
    from lrp_imagecaptioning_amd.engine import LRPEngine
    w, X, idx, R, _ = _net("tiny")
    eng = _engine(TINY_CFG, 16, 3, 6, w)
    for bad in ((0.5, None), (None, -1), (2, 0.5), (None, None)):
        with pytest.raises(ValueError):
            eng.set_cnn_rule(*bad)
    lib = eng._lib                                            # ... and the library's own validation behind the binding's
    assert lib.lrp_set_cnn_rule(eng._h, 2.0, 0.5) == -1 and lib.lrp_set_cnn_rule(eng._h, 0.5, -0.5) == -1
    assert lib.lrp_set_cnn_rule(eng._h, float("nan"), 1.0) == -1
    assert eng.cnn_rule == (1, 0)
    # a pair that is exact in double but not in float32 (1.3f - 0.3f = 1 - 2^-24) is the caller's (1.3, 0.3): accepted
    eng.set_cnn_rule(1.3, None)
    eng.set_cnn_rule(None, 0.3)
    assert lib.lrp_set_cnn_rule(eng._h, 1.3, 0.3) == 0 and lib.lrp_set_cnn_rule(eng._h, 1.3, 0.3001) == -1
    eng.set_cnn_rule(1, 0)
    eng.set_precision("f16x2")
    eng.set_cnn_rule(2, 1)
    eng.encode_images(X)
    with pytest.raises(NotImplementedError):
        eng.cnn_explain(list(idx), R)
    stacks, stem, (h, wd) = NONSQUARE_RESNETS["tiny"]
    rn = LRPEngine(decoder="adaptive", img_hw=(h, wd), L=(h // 8) * (wd // 8), D=4 * stacks[-1][0], H=32, E=32, V=50, max_images=1,
                   max_tokens=1, max_caption_len=4, resnet={"stem": stem, "stacks": stacks})
    rn.set_cnn_rule(1, 0)
    with pytest.raises(NotImplementedError):
        rn.set_cnn_rule(2, 1)
