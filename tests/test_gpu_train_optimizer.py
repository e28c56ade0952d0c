"""What turns the fine-tune step's gradients into new weights, and what it reports besides the loss: Adam past its first
step (tr_adam_kernel + the host's lr_t), the two accuracy heads, train_step at weights Adam produced, and the loop
classes with dropout on.  Inputs, oracle runs and the derived bound live in tests/train_util.py; the CPU side of the
argument (fp32 stays inside the bound, wrong optimizers leave it) is tests/test_oracle_train.py."""
import numpy as np
import pytest
import torch

import train_util as U
from gpu_util import report
from test_gpu_train import CFG, D, H, HW, L, V, _case, _engine, _gridtd_case, rel_l1

pytestmark = pytest.mark.gpu


def _make_engine(w, kind="adaptive", big=False):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    if big:
        g = U.BIG
        eng = LRPEngine(decoder="adaptive", cnn_cfg=U.BIG_CFG, img_hw=(g["hw"], g["hw"]), L=g["L"], D=g["D"], H=g["H"], E=g["H"],
                        V=g["V"], max_images=1, max_tokens=2, max_caption_len=2)
    elif kind == "adaptive":
        return _engine(w, 4)
    else:
        eng = LRPEngine(decoder="gridtd", cnn_cfg=CFG, img_hw=(HW, HW), L=L, D=D, H=H, E=H, V=V, max_images=4, max_tokens=8,
                        max_caption_len=6)
    eng.set_weights(w)
    return eng


def _flat(eng):
    """The master weights as one flat float32 array in the trainer's layout (padding reads as zero)."""
    out = np.zeros(eng.train_flat_size, np.float32)
    for nm, v in eng.train_weights_device().items():
        off, n = eng.train_layout[nm]
        out[off:off + n] = v.cpu().numpy()
    return out


def _ratio(got, ref, k, lr):
    return np.abs(got.astype(np.float64) - ref) / U.adam_bound(k, ref, U.f32c(lr))


@pytest.mark.parametrize("name", list(U.ADAM_CONFIGS))
def test_adam_steps_match_float64_oracle(name):
    """train_apply(G[k]) for k = 1 ... K on synthetic gradients against oracle/train_ref.adam_clipvalue_step in float64 with
    the device's constants, the masters read back after EVERY step:  |p_gpu - p_ref| <= k 2^-22 |p_ref| + k^2 lr 2^-16
    (train_util.adam_bound; derived, and proven on the CPU for fp32 / against wrong optimizers on these gradients)."""
    kind, size, steps, lr, clip, b1, b2, eps = U.ADAM_CONFIGS[name]
    w, cfg, kind = U.adam_weights(name)
    eng = _make_engine(w, kind, big=size == "big")
    layout = eng.train_begin(lr=lr, clipvalue=clip, beta1=b1, beta2=b2, eps=eps)
    want_layout, total = U.flat_layout(w, cfg, kind)
    assert layout == want_layout and eng.train_flat_size == total
    if size == "big":
        assert eng.train_flat_size > U.GRID_LIMIT          # the kernel's grid-stride loop takes a second pass
    p0 = _flat(eng)
    assert np.array_equal(p0, U.flatten(w, layout, total))
    G = U.adam_gradients(layout, total, steps)
    ref = U.adam_reference(p0, G, lr, clip, b1, b2, eps)
    worst = 0.0
    for k in range(1, steps + 1):
        eng.train_apply(torch.as_tensor(G[k - 1]).to(eng.device))
        got = _flat(eng)
        r = _ratio(got, ref[k - 1], k, lr)
        worst = max(worst, float(r.max()))
        assert r.max() <= 1.0, (name, k, int(r.argmax()), float(r.max()))
        if size == "big":                                  # by name, so that a dropped tail cannot hide in a maximum
            off, n = layout["output_b"]
            assert off + n == total and r[off:off + n].max() <= 1.0
            assert np.count_nonzero(got[off:off + n] != p0[off:off + n]) > n // 2
            for i in (U.GRID_LIMIT - 1, U.GRID_LIMIT, U.GRID_LIMIT + 1):
                assert r[i] <= 1.0 and got[i] != p0[i], (k, i, float(r[i]))
    print("adam %s: max(err / bound) = %.3f over %d steps, %d elements" % (name, worst, steps, total))
    report("train_adam_" + name, max_err_over_bound=worst, steps=steps, elements=total)
    if name != "default":
        return
    # eight rebuilds of the operand copies later the explanation path still runs on the masters
    from oracle import cnn_lrp_ref as Cn
    X = _case(3)[1]
    new = eng.train_weights()
    wn = {k: new[k].reshape(np.shape(w[k])) for k in w}
    eng.encode_images(X[:1])
    feat = eng.get_features().cpu().numpy().reshape(1, -1, D)
    ref_feat = Cn.forward(Cn.vgg_layers(wn, CFG), X[:1]).reshape(1, -1, D)
    assert np.abs(ref_feat).sum() > 0 and rel_l1(feat, ref_feat) < 1e-5
    R = np.abs(np.random.RandomState(0).standard_normal((1, L, D))).astype(np.float32) * feat
    got = eng.cnn_explain([0], R).cpu().numpy()
    want = Cn.analyze(Cn.vgg_layers(wn, CFG), X[:1], R.reshape(1, 4, 4, D))
    assert rel_l1(got, want) < 1e-4


@pytest.mark.parametrize("kind", ["adaptive", "gridtd"])
@pytest.mark.parametrize("with_masks", [False, True])
def test_accuracy_heads_match_oracle(kind, with_masks):
    """losses[3], losses[4] == float32(hits / rows) of oracle/train_ref.two_head_accuracy on labels chosen so that both
    values are informative (train_util.accuracy_case; its conditions are asserted in tests/test_oracle_train.py)."""
    from oracle import train_ref as T
    w, X, cap_in, y, lw, masks, _, (h1, h2, n) = U.accuracy_case(kind, with_masks)
    eng = _make_engine(w, kind)
    eng.train_begin()
    eng.encode_images(X)
    _, losses = eng.train_step(cap_in, y, lw, masks)
    total, l1, l2, _, logits = T.loss_and_grads(w, CFG, X, cap_in, y, lw, masks, kind=kind)
    assert T.two_head_accuracy(logits, lw, y, counts=True) == (h1, h2, n)
    got = losses.cpu().numpy()
    print("accuracy %s masks=%s: expected %d/%d %d/%d, obtained %.7f %.7f" % (kind, with_masks, h1, n, h2, n, got[3], got[4]))
    report("train_accuracy_%s_%s" % (kind, "masks" if with_masks else "nomasks"), expected=[h1 / n, h2 / n],
           obtained=[float(got[3]), float(got[4])])
    np.testing.assert_allclose(got[:3], [total, l1, l2], rtol=2e-5)
    assert abs(float(got[3]) - float(np.float32(h1 / n))) <= 1e-6
    assert abs(float(got[4]) - float(np.float32(h2 / n))) <= 1e-6


def test_accuracy_is_zero_without_a_labelled_row():
    w, X, cap_in, y, lw, _ = _case(5, B=3, Tn=5)
    eng = _engine(w, 3)
    eng.train_begin()
    eng.encode_images(X)
    _, l0 = eng.train_step(cap_in, np.full_like(y, -1), lw)
    assert float(l0[3]) == 0.0 and float(l0[4]) == 0.0


@pytest.mark.parametrize("kind,precision", [("adaptive", "fp32"), ("gridtd", "fp32"), ("adaptive", "bf16")])
def test_three_steps_teacher_forced(kind, precision):
    """train_step at weights Adam produced (rebuilt operand copies, the training path's own buffers, carried moments):
    at every step the gradient against the oracle evaluated at the engine's CURRENT masters, then the update against the
    float64 Adam fed the engine's own gradient.  A fresh mask draw per step."""
    from oracle import train_ref as T
    w, X, cap_in, y, lw, masks = _case() if kind == "adaptive" else _gridtd_case()
    lr, clip = (1e-3, 0.01) if kind == "adaptive" else (1e-3, 0.1)
    eng = _make_engine(w, kind)
    layout = eng.train_begin(lr=lr, clipvalue=clip)
    if precision == "bf16":
        eng.train_set_precision("bf16")
    conv_w = {nm + "_W" for nm, _, _, _ in CFG[1:]} if precision == "bf16" else set()
    rs = np.random.RandomState(17)
    p64, m64, v64 = _flat(eng).astype(np.float64), 0.0, 0.0
    c = [U.f32c(x) for x in (lr, clip, 0.9, 0.999, 1e-7)]
    worst_update, worst_grad = 0.0, 0.0
    for k in (1, 2, 3):
        mk = {name: ((rs.uniform(size=v.shape) >= 0.5) * 2.0).astype(np.float32) for name, v in masks.items()}
        cur = eng.train_weights()
        wk = {name: cur[name].reshape(np.shape(w[name])) for name in layout}
        eng.encode_images(X)
        grads, losses = eng.train_step(cap_in, y, lw, mk)
        total, l1, l2, g, _ = T.loss_and_grads(wk, CFG, X, cap_in, y, lw, mk, kind=kind)
        np.testing.assert_allclose(losses.cpu().numpy()[:3], [total, l1, l2], rtol=2e-5)
        gf = grads.cpu().numpy()
        errs = {name: rel_l1(gf[off:off + n], g[name]) for name, (off, n) in layout.items()}
        bad = {name: e for name, e in errs.items() if not e < (2e-2 if name in conv_w else 2e-4)}
        assert not bad, (k, bad)
        worst_grad = max(worst_grad, max(e for name, e in errs.items() if name not in conv_w))
        eng.train_apply(grads)
        p64, m64, v64 = T.adam_clipvalue_step(p64, gf.astype(np.float64), m64, v64, k, *c)
        r = _ratio(_flat(eng), p64, k, lr)
        worst_update = max(worst_update, float(r.max()))
        assert r.max() <= 1.0, (k, int(r.argmax()), float(r.max()))
    print("three steps %s %s: max(err / bound) = %.3f, worst gradient rel L1 = %.2e" % (kind, precision, worst_update, worst_grad))
    report("train_three_steps_%s_%s" % (kind, precision), max_err_over_bound=worst_update, worst_grad_rel_l1=worst_grad)


def _loop_case(kind):
    from lrp_imagecaptioning_amd.explainers import (CaptionModelSpec, ExplainImgCaptioningAdaptiveAttention,
                                                    ExplainImgCaptioningGridTDModel)
    from lrp_imagecaptioning_amd.training import TrainingLRPInferenceAdaptive, TrainingLRPInferenceGridTD
    w, X, cap_in, y, lw, _ = _case(7, B=4, Tn=5) if kind == "adaptive" else _gridtd_case(23, B=4)
    X = X * 64

    def make(seed=3):
        spec = CaptionModelSpec(w, img_encoder="vgg16", hidden_dim=H, embedding_dim=H, L=L, D=D, vocab_size=V, cnn_cfg=CFG,
                                img_hw=(HW, HW))
        if kind == "adaptive":
            ex = ExplainImgCaptioningAdaptiveAttention(spec, None, None, max_caption_length=5, max_images=4)
            return TrainingLRPInferenceAdaptive(ex, learning_rate=1e-3, drop_rate=0.5, seed=seed)
        ex = ExplainImgCaptioningGridTDModel(spec, None, None, max_caption_length=5, max_images=4)
        return TrainingLRPInferenceGridTD(ex, learning_rate=1e-3, drop_rate=0.5, seed=seed)
    return make, w, X, cap_in, y, lw


def _masters_equal(a, b):
    wa, wb = a._engine.train_weights_device(), b._engine.train_weights_device()
    return all(torch.equal(wa[k], wb[k]) for k in wa)


@pytest.mark.parametrize("kind", ["adaptive", "gridtd"])
def test_loop_class_with_dropout(kind):
    """TrainingLRPInference* at drop_rate = 0.5: the masks `_masks` draws (keys, documented layout, scale, kept share),
    their way through train_on_batch against the oracle, the early-forward path with masks, and the seeded generator."""
    from oracle import train_ref as T
    make, w, X, cap_in, y, lw = _loop_case(kind)
    B, Tn = cap_in.shape
    M, A = make(), make()
    # -- mask bookkeeping: M draws what A's first and second train_on_batch will draw
    drawn = [M._masks(B, Tn), M._masks(B, Tn)]
    shapes = {"image_features": (B, L, H), "global": (B, H), "output": (B, Tn, H), "lstm_in": (Tn, 4, B, 2 * H),
              "lstm_rec": (Tn, 4, B, H)}
    if kind == "gridtd":
        shapes["logits"] = (B, Tn, V)
    # kept share: a mask of n independent draws at p = 0.5 has a share of standard deviation 0.5 / sqrt(n), so 0.5 +- 0.05
    # is a test of the generator's rate only where it is many deviations wide.  "Larger" is n >= 2500, where it is five or
    # more (a fair generator leaves it about once in 2e6 masks); at n = 1024 it would be 3.2 and fail once in 700.  The
    # masks below that size are held to the same band pooled per draw (n >= 5000 in both decoders).
    for j, masks in enumerate(drawn):
        assert set(masks) == set(shapes)
        kept = total = 0
        for k, m in masks.items():
            assert tuple(m.shape) == shapes[k] and m.dtype == torch.float32
            assert set(np.unique(m.cpu().numpy()).tolist()) <= {0.0, 2.0}             # {0, 1 / (1 - p)}
            share = float((m != 0).float().mean())
            print("mask share %s draw %d %s[%d] = %.4f" % (kind, j, k, m.numel(), share))
            kept, total = kept + int((m != 0).sum()), total + m.numel()
            if m.numel() >= 2500:
                assert abs(share - 0.5) <= 0.05, (k, share)
        assert total >= 5000 and abs(kept / total - 0.5) <= 0.05, (j, kept, total)
    assert any(m.numel() >= 2500 for m in drawn[0].values())
    assert not torch.equal(drawn[0]["output"], drawn[1]["output"])
    # -- explicit lrp_weight: the five numbers of call j == the oracle at A's weights before call j with M's j-th masks
    for j in range(2):
        wj = A.get_weights()
        got = A.train_on_batch([cap_in, X], y, lrp_weight=lw)
        mk = {k: v.cpu().numpy() for k, v in drawn[j].items()}
        total, l1, l2, _, logits = T.loss_and_grads(wj, CFG, X, cap_in, y, lw, mk, kind=kind)
        a1, a2 = T.two_head_accuracy(logits, lw, y)
        assert len(got) == 5
        np.testing.assert_allclose(got[:3], [total, l1, l2], rtol=2e-5)
        assert abs(got[3] - float(np.float32(a1))) <= 1e-6 and abs(got[4] - float(np.float32(a2))) <= 1e-6
    # -- seeding: the same seed and calls give bit-identical masters, another seed does not
    A2, C = make(), make(seed=4)
    for tr in (A2, C):
        for j in range(2):
            tr.train_on_batch([cap_in, X], y, lrp_weight=lw)
    assert _masters_equal(A, A2)
    assert not _masters_equal(A, C)
    # -- the early-forward path (lrp_weight computed inside, train_forward with masks on the side stream) against the
    #    same lrp_weight handed in explicitly: equal losses, bit-identical masters
    Bq, Dq = make(), make()
    got_b = Bq.train_on_batch([cap_in, X], y)
    lw_d = Dq._lrp_layer.call_device(X, Dq.predict_on_batch([cap_in, X]))
    assert bool((lw_d != 1).any())
    got_d = Dq.train_on_batch([cap_in, X], y, lrp_weight=lw_d)
    assert got_b == got_d
    assert _masters_equal(Bq, Dq)
