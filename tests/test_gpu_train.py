"""Fine-tune step against oracle/train_ref.py (torch float64 autograd) through the C ABI."""
import numpy as np
import pytest
import torch

from lrp_imagecaptioning_amd.synthetic import adaptive_weights, vgg_weights

pytestmark = pytest.mark.gpu

CFG = [("c1", 3, 8, True), ("c2", 8, 16, True), ("c3", 16, 16, False), ("c4", 16, 16, False)]
HW, L, D, H, V = 16, 16, 16, 16, 40


def rel_l1(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64).reshape(b.shape) - b).sum() / max(np.abs(b).sum(), 1e-30))


def _case(seed=0, B=3, Tn=5):
    rs = np.random.RandomState(seed)
    w = vgg_weights(rs, CFG, bias_std=0.3)
    w.update(adaptive_weights(rs, L, D, H, H, V))
    X = (rs.uniform(0, 255, size=(B, HW, HW, 3)) - 110).astype(np.float32) / 64
    caps = [[int(c) for c in rs.randint(3, V + 1, size=Tn - 1)] + [1] for _ in range(B)]
    cap_in = np.array([[2 - 1] + [c - 1 for c in cap[:-1]] for cap in caps], dtype=np.int32)
    y = np.array([[c - 1 for c in cap] for cap in caps], dtype=np.int32)
    y[1, -2:] = -1
    cap_in[2, 3] = cap_in[0, 1]                                       # a repeated embedding row
    lw = (1 + rs.uniform(0, 1, size=(B, Tn, V)) * (rs.uniform(size=(B, Tn, V)) < 0.2)).astype(np.float32)
    p = 0.5
    mk = lambda *s: ((rs.uniform(size=s) >= p) / (1 - p)).astype(np.float32)
    masks = {"image_features": mk(B, L, H), "global": mk(B, H), "output": mk(B, Tn, H), "lstm_in": mk(Tn, 4, B, 2 * H),
             "lstm_rec": mk(Tn, 4, B, H)}
    return w, X, cap_in, y, lw, masks


def _engine(w, B):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    eng = LRPEngine(decoder="adaptive", cnn_cfg=CFG, img_hw=(HW, HW), L=L, D=D, H=H, E=H, V=V, max_images=4, max_tokens=8,
                    max_caption_len=6)
    eng.set_weights(w)
    return eng


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
@pytest.mark.parametrize("with_masks", [False, True])
def test_gradients_match_oracle(with_masks, precision):
    """(precision = the engine's arithmetic mode: 'fp32' also takes the encoder's not-overlapped forward)"""
    from oracle import train_ref as T
    w, X, cap_in, y, lw, masks = _case()
    if not with_masks:
        masks = None
    eng = _engine(w, len(X))
    eng.set_precision(precision)
    layout = eng.train_begin(lr=1e-3, clipvalue=0.01)
    assert set(layout) == set(T.param_names(CFG))
    eng.encode_images(X)
    grads, losses = eng.train_step(cap_in, y, lw, masks)
    total, l1, l2, g, _ = T.loss_and_grads(w, CFG, X, cap_in, y, lw, masks)
    np.testing.assert_allclose(losses.cpu().numpy()[:3], [total, l1, l2], rtol=2e-5)
    assert 0 <= losses[3] <= 1 and 0 <= losses[4] <= 1
    gf = grads.cpu().numpy()
    worst = {}
    for name, (off, n) in layout.items():
        worst[name] = rel_l1(gf[off:off + n], g[name])
    bad = {k: v for k, v in worst.items() if not v < 2e-4}
    assert not bad, bad


def test_adam_step_matches_oracle_and_engine_follows():
    """Adam's first step and the engine following the masters; steps beyond the first: tests/test_gpu_train_optimizer.py."""
    from oracle import train_ref as T
    w, X, cap_in, y, lw, masks = _case(3)
    eng = _engine(w, len(X))
    layout = eng.train_begin(lr=1e-3, clipvalue=0.01)
    eng.encode_images(X)
    grads, _ = eng.train_step(cap_in, y, lw, masks)
    eng.train_apply(grads)
    new = eng.train_weights()
    _, _, _, g, _ = T.loss_and_grads(w, CFG, X, cap_in, y, lw, masks)
    for name in layout:
        p1, _, _ = T.adam_clipvalue_step(np.asarray(w[name], np.float64).ravel(), g[name].ravel(), 0.0, 0.0, 1, 1e-3, 0.01)
        # Adam's first step is lr * sign(g) wherever |g| >> eps: compare where the oracle gradient is not tiny
        big = np.abs(g[name].ravel()) > 1e-5
        np.testing.assert_allclose(new[name][big], p1[big], rtol=0, atol=2e-6)
    # the explanation path now runs on the updated weights
    from oracle import cnn_lrp_ref as Cn
    eng.encode_images(X)
    feat = eng.get_features().cpu().numpy().reshape(len(X), -1, D)
    ref = Cn.forward(Cn.vgg_layers({k: new[k].reshape(np.shape(w[k])) for k in w}, CFG), X).reshape(len(X), -1, D)
    assert rel_l1(feat, ref) < 1e-5
    # ... including the LRP operand copies rebuilt on the device (split / fragment-major forms)
    wn = {k: new[k].reshape(np.shape(w[k])) for k in w}
    R = np.abs(np.random.RandomState(0).standard_normal((1, L, D))).astype(np.float32) * feat[:1]
    got = eng.cnn_explain([0], R).cpu().numpy()
    want = Cn.analyze(Cn.vgg_layers(wn, CFG), X[:1], R.reshape(1, 4, 4, D))
    assert rel_l1(got, want) < 1e-4
    # ... and the decoder's derived matrices (concatenated LSTM kernel, transposed gate block, scan operand)
    from oracle.decoder_ref import AdaptiveOracle
    from oracle.decoder_grad_ref import AdaptiveGradOracle
    cap = [5, 9, 17, 1]
    for rounds in range(2):                              # second round: after another update (everything rebuilt in place)
        eng.decoder_forward([cap])
        o = AdaptiveOracle(wn, L, D, H, H)
        o.forward(ref[:1].reshape(1, 4, 4, D).astype(np.float32), cap)
        Rf, att, rw = eng.decoder_explain([0, 0], [1, 3])
        for k, t in enumerate((1, 3)):
            Ro, _ = o.explain(t)
            assert rel_l1(Rf[k].cpu().numpy(), Ro.reshape(L, D)) < 1e-4
        d, _ = eng.decoder_gradient([0], [3])
        og = AdaptiveGradOracle(wn, L, D, H, H)
        og.forward(ref[:1].reshape(1, 4, 4, D).astype(np.float32), cap)
        assert rel_l1(d[0].cpu().numpy(), np.asarray(og.backward(3)[0]).reshape(L, D)) < 1e-4
        if rounds == 0:
            eng.encode_images(X)
            g2, _ = eng.train_step(cap_in, y, lw, masks)
            eng.train_apply(g2)
            new = eng.train_weights()
            wn = {k: new[k].reshape(np.shape(w[k])) for k in w}
            eng.encode_images(X)
            ref = Cn.forward(Cn.vgg_layers(wn, CFG), X).reshape(len(X), -1, D)
    with pytest.raises(RuntimeError):
        eng.set_weights({"Wv": w["Wv"]})                 # the trainer owns the weights now
    with pytest.raises(ValueError):
        eng.train_step(cap_in[:, :1], y[:, :1], lw[:, :1])           # T < 2
    bad = cap_in.copy(); bad[0, 0] = V
    with pytest.raises(ValueError):
        eng.train_step(bad, y, lw)                                   # embedding row out of range
    bad = y.copy(); bad[0, 0] = V
    with pytest.raises(ValueError):
        eng.train_step(cap_in, bad, lw)                              # label out of range


def test_training_loop_class():
    """`TrainingLRPInferenceAdaptive`: predict -> lrp_weight -> train_on_batch on one handle (train.py:571-580)."""
    from lrp_imagecaptioning_amd.explainers import CaptionModelSpec, ExplainImgCaptioningAdaptiveAttention
    from lrp_imagecaptioning_amd.training import TrainingLRPInferenceAdaptive
    from oracle import train_ref as T
    w, X, cap_in, y, lw, _ = _case(7, B=4, Tn=5)
    X = X * 64
    spec = CaptionModelSpec(w, img_encoder="vgg16", hidden_dim=H, embedding_dim=H, L=L, D=D, vocab_size=V, cnn_cfg=CFG,
                            img_hw=(HW, HW))
    ex = ExplainImgCaptioningAdaptiveAttention(spec, None, None, max_caption_length=5, max_images=4)
    tr = TrainingLRPInferenceAdaptive(ex, learning_rate=2e-3, clipvalue=0.01, drop_rate=0.0)
    y_pred = tr.predict_on_batch([cap_in, X]).cpu().numpy()
    _, _, _, _, logits = T.loss_and_grads(w, CFG, X, cap_in, y, np.ones_like(lw))
    assert rel_l1(y_pred, logits) < 1e-5                                   # predict == the oracle's inference forward
    y_dev = tr.predict_on_batch([cap_in, X])
    lw_host = tr._lrp_layer.call([cap_in, X, y_dev.cpu().numpy()])
    lw_dev = tr._lrp_layer.call_device(X, y_dev).cpu().numpy()
    assert (lw_host != 1).sum() > 0
    np.testing.assert_allclose(lw_dev, lw_host, rtol=1e-6)               # device-side assembly == the reference-shaped call
    onehot = np.zeros(y.shape + (V,), np.float32)
    for b in range(y.shape[0]):
        for t in range(y.shape[1]):
            if y[b, t] >= 0:
                onehot[b, t, y[b, t]] = 1
    first = tr.train_on_batch([cap_in, X], onehot)
    assert len(first) == 5 and np.isfinite(first).all()
    # the first call's loss is the oracle's loss for the lrp_weight the layer produced
    w1 = tr.get_weights()
    assert any(np.abs(w1[k] - np.asarray(w[k])).max() > 0 for k in ("c1_W", "lstm_Wi", "output_W"))
    losses = [first[0]] + [tr.train_on_batch([cap_in, X], y)[0] for _ in range(12)]
    assert losses[-1] < losses[0], losses                                  # same batch over and over: the loss goes down
    # checkpoint round trip (train.py:585-587 save_weights -> E:27 load_weights): a fresh explainer on the bundle
    import os, tempfile
    with tempfile.TemporaryDirectory() as d:
        path = tr.save_weights(os.path.join(d, "keras_model_00.npz"))
        after = tr.predict_on_batch([cap_in, X]).cpu().numpy()
        spec2 = CaptionModelSpec(w, img_encoder="vgg16", hidden_dim=H, embedding_dim=H, L=L, D=D, vocab_size=V, cnn_cfg=CFG,
                                 img_hw=(HW, HW))
        ex2 = ExplainImgCaptioningAdaptiveAttention(spec2, path, None, max_caption_length=5, max_images=4)
        ex2._engine.encode_images(X)
        ex2._engine.decoder_forward([[int(c) + 1 for c in cap_in[b, 1:]] + [1] for b in range(len(X))])
        again = ex2._engine.read_state("caption_preds")[:, :cap_in.shape[1]].cpu().numpy()
    np.testing.assert_allclose(again, after, rtol=1e-5, atol=1e-6)


def test_gradients_match_oracle_midsize():
    """Widths that are not multiples of the 64 / 128 GEMM tiles, enough rows for the K split, a vocabulary wider than a tile."""
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from oracle import train_ref as T
    cfg = [("c1", 3, 24, False), ("c2", 24, 72, True), ("c3", 72, 136, True), ("c4", 136, 136, False)]
    hw, Lm, Dm, Hm, Vm, B, Tn = 28, 49, 136, 136, 300, 5, 6
    rs = np.random.RandomState(11)
    w = vgg_weights(rs, cfg, bias_std=0.2)
    w.update(adaptive_weights(rs, Lm, Dm, Hm, Hm, Vm))
    X = (rs.uniform(0, 255, size=(B, hw, hw, 3)) - 110).astype(np.float32) / 64
    cap_in = np.concatenate([np.full((B, 1), 1), rs.randint(2, Vm, size=(B, Tn - 1))], axis=1).astype(np.int32)
    y = rs.randint(0, Vm, size=(B, Tn)).astype(np.int32)
    y[0, 3:] = -1
    lw = (1 + rs.uniform(0, 1, size=(B, Tn, Vm)) * (rs.uniform(size=(B, Tn, Vm)) < 0.1)).astype(np.float32)
    mk = lambda *s: ((rs.uniform(size=s) >= 0.5) * 2.0).astype(np.float32)
    masks = {"image_features": mk(B, Lm, Hm), "global": mk(B, Hm), "output": mk(B, Tn, Hm), "lstm_in": mk(Tn, 4, B, 2 * Hm),
             "lstm_rec": mk(Tn, 4, B, Hm)}
    eng = LRPEngine(decoder="adaptive", cnn_cfg=cfg, img_hw=(hw, hw), L=Lm, D=Dm, H=Hm, E=Hm, V=Vm, max_images=B, max_tokens=8,
                    max_caption_len=Tn)
    eng.set_weights(w)
    layout = eng.train_begin()
    eng.encode_images(X)
    grads, losses = eng.train_step(cap_in, y, lw, masks)
    total, l1, l2, g, _ = T.loss_and_grads(w, cfg, X, cap_in, y, lw, masks)
    np.testing.assert_allclose(losses.cpu().numpy()[:3], [total, l1, l2], rtol=5e-5)
    gf = grads.cpu().numpy()
    bad = {}
    for name, (off, n) in layout.items():
        e = rel_l1(gf[off:off + n], g[name])
        if not e < 3e-4:
            bad[name] = e
    assert not bad, bad
    g2, _ = eng.train_step(cap_in, y, lw, masks)
    assert torch.equal(grads, g2)                       # no atomics anywhere: run-to-run identical


SGEMM_CASES = [  # (M, N, K, transA, transB): the three forms at shapes of the step (tile edges, K split, strided views)
    (512, 10000, 672, True, False), (672, 512, 10000, False, True), (672, 2048, 1024, False, False),
    (32, 2048, 512, False, False), (32, 512, 2048, False, True), (136, 72, 5000, True, False), (64, 64, 100000, True, False),
    (3, 64, 70000, True, False), (1, 1, 1, False, False), (129, 257, 33, False, True),
]


@pytest.mark.parametrize("M,N,K,ta,tb", SGEMM_CASES)
def test_sgemm_matches_torch(M, N, K, ta, tb):
    """csrc/train_gemm.h against a float64 torch product (the MFMA accumulates fp32: tolerance ~ sqrt(K) ulp)."""
    from lrp_imagecaptioning_amd.engine import op_sgemm
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N)
    pad = 8                                                # operands are views into wider buffers: lda / ldb != width
    A = torch.randn((K, M + pad) if ta else (M, K + pad), device="cuda", generator=g)[:, :(M if ta else K)]
    B = torch.randn((N, K + pad) if tb else (K, N + pad), device="cuda", generator=g)[:, :(K if tb else N)]
    want = (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
    got = op_sgemm(A, B, ta, tb)
    scale = want.abs().mean()
    assert float((got.double() - want).abs().max() / scale) < 2e-5
    C0 = torch.randn((M, N), device="cuda", generator=g)
    got2 = op_sgemm(A, B, ta, tb, C_init=C0.clone())
    assert float((got2.double() - (want + C0.double())).abs().max() / scale) < 2e-5
    assert torch.equal(op_sgemm(A, B, ta, tb), got)       # deterministic K split


@pytest.mark.parametrize("NB,HW,Cin,Cout", [(2, 224, 3, 64), (2, 112, 64, 128), (4, 28, 512, 512), (3, 14, 136, 72), (1, 5, 8, 8)])
def test_conv_wgrad_matches_torch(NB, HW, Cin, Cout):
    """lrp_op_conv_wgrad at VGG16 layer shapes against torch's conv weight gradient in float64 on the CPU."""
    import torch.nn.functional as F
    from lrp_imagecaptioning_amd.engine import op_conv_wgrad
    g = torch.Generator().manual_seed(NB + HW)
    x = torch.randn((NB, HW, HW, Cin), generator=g)
    dz = torch.randn((NB, HW, HW, Cout), generator=g) * (torch.rand((NB, HW, HW, Cout), generator=g) > 0.5)
    w = torch.zeros((Cout, Cin, 3, 3), dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w, b, padding=1)
    y.backward(dz.double().permute(0, 3, 1, 2))
    dw, db = op_conv_wgrad(x.cuda(), dz.cuda())
    want = w.grad.permute(2, 3, 1, 0)                                   # OIHW -> HWIO
    assert rel_l1(dw.cpu().numpy(), want.numpy()) < 1e-5
    assert rel_l1(db.cpu().numpy(), b.grad.numpy()) < 1e-5


def _gridtd_case(seed=21, B=3, Tn=5):
    from lrp_imagecaptioning_amd.synthetic import gridtd_weights
    rs = np.random.RandomState(seed)
    w = vgg_weights(rs, CFG, bias_std=0.3)
    w.update(gridtd_weights(rs, L, D, H, H, V))
    X = (rs.uniform(0, 255, size=(B, HW, HW, 3)) - 110).astype(np.float32) / 64
    cap_in = np.concatenate([np.full((B, 1), 1), rs.randint(2, V, size=(B, Tn - 1))], axis=1).astype(np.int32)
    y = rs.randint(0, V, size=(B, Tn)).astype(np.int32)
    y[1, -2:] = -1
    lw = (1 + rs.uniform(0, 1, size=(B, Tn, V)) * (rs.uniform(size=(B, Tn, V)) < 0.2)).astype(np.float32)
    mk = lambda *s: ((rs.uniform(size=s) >= 0.5) * 2.0).astype(np.float32)
    masks = {"image_features": mk(B, L, H), "global": mk(B, H), "output": mk(B, Tn, H), "lstm_in": mk(Tn, 4, B, 2 * H),
             "lstm_rec": mk(Tn, 4, B, H), "logits": mk(B, Tn, V)}
    return w, X, cap_in, y, lw, masks


@pytest.mark.parametrize("with_masks", [False, True])
def test_gridtd_gradients_match_oracle(with_masks):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from oracle import train_ref as T
    w, X, cap_in, y, lw, masks = _gridtd_case()
    if not with_masks:
        masks = None
    eng = LRPEngine(decoder="gridtd", cnn_cfg=CFG, img_hw=(HW, HW), L=L, D=D, H=H, E=H, V=V, max_images=4, max_tokens=8,
                    max_caption_len=6)
    eng.set_weights(w)
    layout = eng.train_begin(lr=1e-3, clipvalue=0.1)
    assert set(layout) == set(T.param_names(CFG, "gridtd"))
    eng.encode_images(X)
    grads, losses = eng.train_step(cap_in, y, lw, masks)
    total, l1, l2, g, _ = T.loss_and_grads(w, CFG, X, cap_in, y, lw, masks, kind="gridtd")
    np.testing.assert_allclose(losses.cpu().numpy()[:3], [total, l1, l2], rtol=2e-5)
    gf = grads.cpu().numpy()
    bad = {}
    for name, (off, n) in layout.items():
        e = rel_l1(gf[off:off + n], g[name])
        if not e < 2e-4:
            bad[name] = e
    assert not bad, bad


def test_gridtd_training_loop_and_operand_rebuild():
    from lrp_imagecaptioning_amd.explainers import CaptionModelSpec, ExplainImgCaptioningGridTDModel
    from lrp_imagecaptioning_amd.training import TrainingLRPInferenceGridTD
    from oracle import cnn_lrp_ref as Cn
    from oracle import train_ref as T
    from oracle.decoder_ref import GridTDOracle
    w, X, cap_in, y, lw, _ = _gridtd_case(23, B=4)
    X = X * 64
    spec = CaptionModelSpec(w, img_encoder="vgg16", hidden_dim=H, embedding_dim=H, L=L, D=D, vocab_size=V, cnn_cfg=CFG,
                            img_hw=(HW, HW))
    ex = ExplainImgCaptioningGridTDModel(spec, None, None, max_caption_length=5, max_images=4)
    tr = TrainingLRPInferenceGridTD(ex, learning_rate=2e-3, drop_rate=0.0)
    y_pred = tr.predict_on_batch([cap_in, X]).cpu().numpy()
    _, _, _, _, logits = T.loss_and_grads(w, CFG, X, cap_in, y, np.ones_like(lw), kind="gridtd")
    assert rel_l1(y_pred, logits) < 1e-5                                   # the Keras model's logits (h2 + c_hat)
    losses = [tr.train_on_batch([cap_in, X], y)[0] for _ in range(10)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    # after ten updates (operands rebuilt in place nine times) the explanation follows the master weights
    new = tr.get_weights()
    wn = {k: new[k].reshape(np.shape(w[k])) for k in w}
    eng = ex._engine
    eng.encode_images(X[:1])
    feat = Cn.forward(Cn.vgg_layers(wn, CFG), X[:1]).astype(np.float32)
    cap = [5, 9, 17, 1]
    eng.decoder_forward([cap])
    o = GridTDOracle(wn, L, D, H, H)
    o.forward(feat, cap)
    Rf, _, _ = eng.decoder_explain([0, 0], [1, 3])
    for k, t in enumerate((1, 3)):
        Ro, _ = o.explain(t)
        assert rel_l1(Rf[k].cpu().numpy(), Ro.reshape(L, D)) < 1e-4


def test_train_step_edge_cases():
    """Smallest shapes and degenerate labels: B = 1 / T = 2; no labelled row at all (zero loss, zero gradient);
    lrp_weight == 1 everywhere (both heads see the same logits)."""
    from oracle import train_ref as T
    w, X, cap_in, y, lw, _ = _case(5, B=3, Tn=5)
    eng = _engine(w, 3)
    layout = eng.train_begin()
    eng.encode_images(X[:1])
    g1, l1 = eng.train_step(cap_in[:1, :2], y[:1, :2], lw[:1, :2])
    tot, a, b, g, _ = T.loss_and_grads(w, CFG, X[:1], cap_in[:1, :2], y[:1, :2], lw[:1, :2])
    np.testing.assert_allclose(l1.cpu().numpy()[:3], [tot, a, b], rtol=2e-5)
    gf = g1.cpu().numpy()
    assert all(rel_l1(gf[o:o + n], g[k]) < 2e-4 for k, (o, n) in layout.items() if np.abs(g[k]).sum() > 0)
    eng.encode_images(X)
    g0, l0 = eng.train_step(cap_in, np.full_like(y, -1), lw)
    assert float(l0[0]) == 0.0 and float(g0.abs().max()) == 0.0
    _, l2 = eng.train_step(cap_in, y, np.ones_like(lw))
    assert float(l2[1]) == float(l2[2]) and float(l2[3]) == float(l2[4])


def test_gradients_match_oracle_vgg16_full_size():
    """The real encoder (VGG16, 224 x 224, L = 196, D = H = 512) for one image: every kernel configuration the
    BASELINE-size step uses (256 x 128 gradient tiles, K = 1.6 M-pixel splits, the 224^2 gather, the im2col image layer)."""
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import VGG16_CFG, images
    from oracle import train_ref as T
    Lf, Df, Hf, Vf_, B, Tn = 196, 512, 512, 300, 1, 3
    rs = np.random.RandomState(31)
    w = vgg_weights(rs)
    w.update(adaptive_weights(rs, Lf, Df, Hf, Hf, Vf_))
    X = images(rs, B)
    cap_in = np.array([[1, 17, 230]], dtype=np.int32)
    y = np.array([[16, 229, 0]], dtype=np.int32)
    lw = (1 + rs.uniform(0, 1, size=(B, Tn, Vf_)) * (rs.uniform(size=(B, Tn, Vf_)) < 0.1)).astype(np.float32)
    eng = LRPEngine(decoder="adaptive", cnn_cfg=VGG16_CFG, img_hw=(224, 224), L=Lf, D=Df, H=Hf, E=Hf, V=Vf_, max_images=1,
                    max_tokens=4, max_caption_len=4)
    eng.set_weights(w)
    layout = eng.train_begin()
    eng.encode_images(X)
    grads, losses = eng.train_step(cap_in, y, lw)
    import time
    t0 = time.perf_counter()
    total, l1, l2, g, _ = T.loss_and_grads(w, VGG16_CFG, X, cap_in, y, lw)
    from gpu_util import report
    report("train_full_size", cpu_oracle_seconds_per_image=round(time.perf_counter() - t0, 2), cpu_threads=torch.get_num_threads())
    np.testing.assert_allclose(losses.cpu().numpy()[:3], [total, l1, l2], rtol=1e-4)
    gf = grads.cpu().numpy()
    errs = {name: rel_l1(gf[off:off + n], g[name]) for name, (off, n) in layout.items()}
    # The decoder's gradients and the features' are smooth functions of the forward: fp32-level agreement.  Below the
    # features the gradient of a ReLU / max-pool net is only piecewise continuous: a forward that differs from float64
    # in the 7th digit flips a handful of near-tie ReLU / arg-max decisions per image, and one flip in block 5 moves
    # every gradient below it by ~1e-3 (plain torch float32 on the CPU is 1e-3 ... 4e-3 from float64 on this very case,
    # scratch-measured; the same walk is 7e-7 from float64 on an image without such a tie, tests/test_gpu_gradient.py).
    dec = [k for k in errs if not k.startswith("block")]
    assert all(errs[k] < 1e-4 for k in dec), {k: errs[k] for k in dec}
    assert errs["block5_conv3_W"] < 1e-4 and errs["block5_conv3_b"] < 1e-4          # (its dZ is the masked head itself)
    assert all(v < 2e-2 for v in errs.values()), errs


def test_early_forward_gives_identical_gradients():
    """lrp_train_forward on a side stream + lrp_train_step == lrp_train_step alone, bit for bit; a forward for another
    (B, T) is ignored."""
    w, X, cap_in, y, lw, masks = _case(9)
    eng = _engine(w, len(X))
    eng.train_begin()
    eng.encode_images(X)
    g_ref, l_ref = eng.train_step(cap_in, y, lw, masks)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.train_forward(cap_in, masks)
    g1, l1 = eng.train_step(cap_in, y, lw, masks)
    assert torch.equal(g1, g_ref) and torch.equal(l1, l_ref)
    with torch.cuda.stream(side):
        eng.train_forward(cap_in[:, :3], {k: (v[:, :3] if k == "output" else v[:3] if k.startswith("lstm") else v) for k, v in masks.items()})
    side.synchronize()
    g2, _ = eng.train_step(cap_in, y, lw, masks)              # different T: the early forward does not apply
    assert torch.equal(g2, g_ref)


def test_step_refuses_masks_other_than_the_early_forwards():
    """lrp_train_forward reads the caller's mask buffers and lrp_train_step's backward scan reads them again (nothing is
    staged, include/lrp_hip.h): a step handed OTHER mask pointers than its pending early forward ran with must be refused
    (LRP_ERR_INVALID -> ValueError), not back-propagated through masks the forward never applied; the same objects pass."""
    w, X, cap_in, y, lw, masks = _case(13)
    eng = _engine(w, len(X))
    eng.train_begin()
    eng.encode_images(X)
    g_ref = eng.train_step(cap_in, y, lw, masks)[0].clone()
    eng.train_forward(cap_in, masks)
    other = {k: np.array(v) for k, v in masks.items()}    # equal values, other objects -> other device buffers
    with pytest.raises(ValueError):
        eng.train_step(cap_in, y, lw, other)
    eng.encode_images(X)                                   # drops the pending forward
    eng.train_forward(cap_in, masks)
    g = eng.train_step(cap_in, y, lw, masks)[0]
    assert torch.equal(g, g_ref)


def test_refused_step_then_retry_with_fresh_masks_equals_a_plain_step():
    """refuse, then RETRY.  After a refused step the early forward's device tensors lose their
    keep-alive; torch's caching allocator hands the same addresses to the retry's fresh masks, and a library that still
    held the early forward's pointers would accept them and back-propagate through masks that forward never applied.
    The refusal (and any failed step) now drops the pending forward — lrp_train_step on a mismatch, lrp_train_drop_forward
    (ABI v6) from engine.train_step's error path — so the retry runs its own forward: gradients equal to a plain step with
    the NEW masks, bit for bit, both when the library refuses (other pointers) and when the host side does (bad labels)."""
    w, X, cap_in, y, lw, masks = _case(13)
    eng = _engine(w, len(X))
    eng.train_begin()
    eng.encode_images(X)
    rs = np.random.RandomState(99)
    fresh = lambda: {k: ((rs.uniform(size=v.shape) < 0.5) * 2.0).astype(np.float32) for k, v in masks.items()}
    for how in ("library_refuses", "host_refuses"):
        eng.train_forward(cap_in, masks)
        with pytest.raises(ValueError):
            if how == "library_refuses":
                eng.train_step(cap_in, y, lw, {k: np.array(v) for k, v in masks.items()})
            else:
                eng.train_step(cap_in, np.full_like(np.asarray(y), 10 ** 6), lw, masks)
        new = fresh()                                          # same shapes: the allocator reuses the released blocks
        g = eng.train_step(cap_in, y, lw, new)[0].clone()
        g_ref = eng.train_step(cap_in, y, lw, new)[0]          # a plain step (no early forward pending)
        assert torch.equal(g, g_ref), how
        g_old = eng.train_step(cap_in, y, lw, masks)[0]
        assert not torch.equal(g, g_old)                       # (the masks do matter)


def test_early_forward_is_dropped_by_a_new_encode_or_weight():
    """lrp_train_forward(batch 0) followed by lrp_encode_images(batch 1) — e.g. a loop whose explanation raised between
    the two — must NOT let lrp_train_step(batch 1) back-propagate through batch 0's activations: same (B, T), new
    images, the result has to be the fresh step's, bit for bit.  The same for lrp_set_features and lrp_set_weight."""
    w, X, cap_in, y, lw, masks = _case(9)
    rs = np.random.RandomState(77)
    X1 = (rs.uniform(0, 255, size=X.shape) - 110).astype(np.float32) / 64
    eng = _engine(w, len(X))
    eng.train_begin()
    eng.encode_images(X1)
    g_ref, l_ref = eng.train_step(cap_in, y, lw, masks)
    g_ref, l_ref = g_ref.clone(), l_ref.clone()
    side = torch.cuda.Stream()
    for how in ("encode", "features", "weight"):
        eng.encode_images(X)                                   # the OLD batch ...
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.train_forward(cap_in, masks)                   # ... gets an early forward on the side stream
        if how == "encode":
            eng.encode_images(X1)                              # new batch, same (B, T)
        elif how == "features":
            eng.set_features(eng.get_features().clone())       # drops the forward (the step itself needs a full encode)
            eng.encode_images(X1)
        else:
            eng.set_weights({"c4_b": w["c4_b"]})               # same values: only the invalidation is under test
            eng.encode_images(X1)
        g, l = eng.train_step(cap_in, y, lw, masks)
        assert torch.equal(g, g_ref) and torch.equal(l, l_ref), how


@pytest.mark.parametrize("NB,HW,Cin,Cout", [(2, 112, 64, 128), (4, 28, 512, 512), (2, 56, 128, 256), (3, 14, 136, 72), (1, 5, 8, 8),
                                            (2, 224, 64, 64)])
def test_conv_wgrad_bf16_matches_torch(NB, HW, Cin, Cout):
    """lrp_op_conv_wgrad_bf16 (csrc/train_gemm_bf16.h: operands rounded to bf16, transposed LDS reads, bf16 MFMA, fp32
    accumulate).  Two bars: (a) against the float64 gradient of the SAME bf16-rounded operands only the fp32
    accumulation differs -> 2e-5; (b) against the float64 gradient of the unrounded operands the rounding shows: the
    stated tolerance of the bf16 training mode, 1e-2 relative L1 (2^-9 per operand, random sign, averaged over K)."""
    import torch.nn.functional as F
    from lrp_imagecaptioning_amd.engine import op_conv_wgrad
    g = torch.Generator().manual_seed(NB + HW)
    x = torch.randn((NB, HW, HW, Cin), generator=g)
    dz = torch.randn((NB, HW, HW, Cout), generator=g) * (torch.rand((NB, HW, HW, Cout), generator=g) > 0.5)

    def grad(xx, dd):
        w = torch.zeros((Cout, Cin, 3, 3), dtype=torch.float64, requires_grad=True)
        y = F.conv2d(xx.double().permute(0, 3, 1, 2), w, None, padding=1)
        y.backward(dd.double().permute(0, 3, 1, 2))
        return w.grad.permute(2, 3, 1, 0).numpy()                      # OIHW -> HWIO
    dw, db = op_conv_wgrad(x.cuda(), dz.cuda(), bf16=True)
    dw = dw.cpu().numpy()
    assert np.isfinite(dw).all()
    assert rel_l1(dw, grad(x.bfloat16().float(), dz.bfloat16().float())) < 2e-5
    assert rel_l1(dw, grad(x, dz)) < 1e-2
    assert rel_l1(db.cpu().numpy(), dz.double().sum((0, 1, 2)).numpy()) < 1e-5      # (the bias gradient stays fp32)
    dw2, _ = op_conv_wgrad(x.cuda(), dz.cuda(), bf16=True)
    assert np.array_equal(dw2.cpu().numpy(), dw)                       # deterministic K split


def test_gradients_in_bf16_training_mode():
    """lrp_train_set_precision(LRP_TRAIN_BF16) — BASELINE config 5's arithmetic: the encoder's weight gradients on the
    bf16 MFMA (operands rounded to bf16), everything else as in the fp32 mode.  Stated tolerance vs the float64 oracle:
    conv kernels 2e-2 relative L1, every other tensor (decoder, biases) the fp32 mode's 2e-4."""
    from oracle import train_ref as T
    w, X, cap_in, y, lw, masks = _case()
    eng = _engine(w, len(X))
    layout = eng.train_begin(lr=1e-3, clipvalue=0.01)
    with pytest.raises(ValueError):
        eng.train_set_precision("fp8")
    eng.train_set_precision("bf16")
    eng.encode_images(X)
    grads, losses = eng.train_step(cap_in, y, lw, masks)
    total, l1, l2, g, _ = T.loss_and_grads(w, CFG, X, cap_in, y, lw, masks)
    np.testing.assert_allclose(losses.cpu().numpy()[:3], [total, l1, l2], rtol=2e-5)
    gf = grads.cpu().numpy()
    conv_w = {name + "_W" for name, _, _, _ in CFG[1:]}                # (the image layer's product stays on the fp32 MFMA)
    worst = {name: rel_l1(gf[off:off + n], g[name]) for name, (off, n) in layout.items()}
    bad = {k: v for k, v in worst.items() if not v < (2e-2 if k in conv_w else 2e-4)}
    assert not bad, bad
    assert max(worst[k] for k in conv_w) > 1e-5                        # the mode really took the bf16 path
    eng.train_set_precision("fp32")
    g32, _ = eng.train_step(cap_in, y, lw, masks)
    worst32 = {name: rel_l1(g32.cpu().numpy()[off:off + n], g[name]) for name, (off, n) in layout.items()}
    assert all(v < 2e-4 for v in worst32.values()), worst32
