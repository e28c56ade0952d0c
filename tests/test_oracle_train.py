"""oracle/train_ref.py: pinned against the decoder oracle (itself pinned by reference outputs) and by finite differences."""
import numpy as np
import pytest
import torch

from lrp_imagecaptioning_amd.synthetic import adaptive_weights, vgg_weights
from oracle import cnn_lrp_ref as C
from oracle import train_ref as T
from oracle.decoder_ref import AdaptiveOracle

import train_util as U

CFG = [("c1", 3, 8, True), ("c2", 8, 16, True), ("c3", 16, 16, False)]
HW, L, D, H, V = 16, 16, 16, 16, 24


def _case(seed=0, B=2, Tn=4):
    rs = np.random.RandomState(seed)
    w = vgg_weights(rs, CFG, bias_std=0.3)
    w.update(adaptive_weights(rs, L, D, H, H, V))
    X = rs.uniform(-120, 130, size=(B, HW, HW, 3)).astype(np.float32) / 64
    caps = [[int(c) for c in rs.randint(3, V + 1, size=Tn - 1)] + [1] for _ in range(B)]
    cap_in = np.array([[2 - 1] + [c - 1 for c in cap[:-1]] for cap in caps])        # SOS then the shifted caption
    y = np.array([[c - 1 for c in cap] for cap in caps])
    y[1, -2:] = -1                                                                  # a padded tail
    lw = 1 + rs.uniform(0, 1, size=(B, Tn, V)) * (rs.uniform(size=(B, Tn, V)) < 0.2)
    return rs, w, X, caps, cap_in, y, lw


def test_logits_match_decoder_oracle():
    rs, w, X, caps, cap_in, y, lw = _case()
    _, _, _, _, logits = T.loss_and_grads(w, CFG, X, cap_in, y, lw)
    layers = C.vgg_layers(w, CFG)
    for b in range(len(caps)):
        o = AdaptiveOracle(w, L, D, H, H)
        o.forward(C.forward(layers, X[b:b + 1]).astype(np.float32), caps[b])
        np.testing.assert_allclose(logits[b], o.caption_preds, rtol=2e-4, atol=2e-5)   # (the oracle's chain is float32)


def test_gradients_by_central_differences():
    rs, w, X, caps, cap_in, y, lw = _case(1)
    B, Tn = cap_in.shape
    p = 0.5
    mk = lambda *s: (rs.uniform(size=s) >= p) / (1 - p)
    masks = {"image_features": mk(B, L, H), "global": mk(B, H), "output": mk(B, Tn, H),
             "lstm_in": mk(Tn, 4, B, 2 * H), "lstm_rec": mk(Tn, 4, B, H)}
    total, l1, l2, g, _ = T.loss_and_grads(w, CFG, X, cap_in, y, lw, masks)
    assert np.isclose(total, 0.5 * l1 + 0.5 * l2)
    w64 = {k: np.asarray(v, np.float64) for k, v in w.items()}
    for name in ("c1_W", "c2_b", "c3_W", "image_features_W", "global_b", "embedding", "lstm_Wi", "lstm_Wh", "lstm_b", "Wv",
                 "Wg", "V", "Wx", "Wh", "Ws", "output_W", "output_b"):
        flat = np.abs(g[name]).ravel()
        idx = np.unravel_index(int(np.argmax(flat)), g[name].shape)
        eps = 1e-5
        vals = []
        for sgn in (+1, -1):
            wp = dict(w64)
            wp[name] = w64[name].copy()
            wp[name][idx] += sgn * eps
            vals.append(T.loss_and_grads(wp, CFG, X, cap_in, y, lw, masks)[0])
        fd = (vals[0] - vals[1]) / (2 * eps)
        assert abs(fd - g[name][idx]) <= 1e-5 * max(1.0, abs(fd)) + 1e-8, (name, fd, g[name][idx])


def test_adam_clipvalue_step():
    rs = np.random.RandomState(0)
    p, g = rs.standard_normal(6), np.array([0.5, -0.5, 0.001, -0.002, 0.0, 0.02])
    m = v = np.zeros(6)
    p1, m1, v1 = T.adam_clipvalue_step(p, g, m, v, 1, lr=1e-3, clipvalue=0.01)
    gc = np.clip(g, -0.01, 0.01)
    np.testing.assert_allclose(m1, 0.1 * gc)
    np.testing.assert_allclose(v1, 0.001 * gc * gc)
    # first step of Adam moves every touched parameter by ~lr against the sign of its gradient
    lr_t = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
    np.testing.assert_allclose(p1, p - lr_t * m1 / (np.sqrt(v1) + 1e-7))
    assert np.all(np.sign(p - p1)[g != 0] == np.sign(g)[g != 0]) and p1[4] == p[4]


def test_gridtd_hidden_states_match_decoder_oracle():
    """The grid-TD training graph against oracle/decoder_ref.GridTDOracle (pinned by reference outputs).  The explainer's
    replay takes its logits from h2 alone (E:1154) while the Keras model uses h2 + c_hat (M:816): compare h2 + c_hat."""
    from lrp_imagecaptioning_amd.synthetic import gridtd_weights
    from oracle.decoder_ref import GridTDOracle
    rs = np.random.RandomState(2)
    w = vgg_weights(rs, CFG, bias_std=0.3)
    w.update(gridtd_weights(rs, L, D, H, H, V))
    X = rs.uniform(-2, 2, size=(1, HW, HW, 3)).astype(np.float32)
    cap = [5, 9, 14, 1]
    cap_in = np.array([[1] + [c - 1 for c in cap[:-1]]])
    y = np.array([[c - 1 for c in cap]])
    _, _, _, g, logits = T.loss_and_grads(w, CFG, X, cap_in, y, np.ones((1, 4, V)), kind="gridtd")
    o = GridTDOracle(w, L, D, H, H)
    o.forward(C.forward(C.vgg_layers(w, CFG), X).astype(np.float32), cap)
    want = (o.h2t[1:] + o.context_hat[1:]) @ w["output_W"] + w["output_b"]
    np.testing.assert_allclose(logits[0], want, rtol=2e-4, atol=2e-5)
    assert set(g) == set(T.param_names(CFG, "gridtd")) and all(np.isfinite(v).all() for v in g.values())


def test_two_head_accuracy_hand_example():
    """B = 2, T = 3, V = 4; the last step is dropped, so rows (b, t) with t in {0, 1} count.
      (0, 0) logits [1, 3, 2, 0], lw [1, 1, 2, 1] -> head 2 sees [1, 3, 4, 0]; label 1: head 1 hit, head 2 miss
      (0, 1) logits [2, 2, 1, 0] (tie: the FIRST index, 0), lw 1;               label 1: miss, miss
      (1, 0) logits [-1, -2, -3, -4], lw [2, 1, 1, 1] -> [-2, -2, -3, -4] (tie -> 0); label 0: hit, hit
      (1, 1) no label (-1): dropped although its arg-max is defined
      (0, 2), (1, 2): last step, dropped although (0, 2) would be a hit for both heads
    -> 3 rows; head 1: 2 hits = 2/3; head 2: 1 hit = 1/3."""
    logits = np.array([[[1, 3, 2, 0], [2, 2, 1, 0], [9, 0, 0, 0]],
                       [[-1, -2, -3, -4], [0, 5, 0, 0], [0, 0, 0, 0]]], np.float64)
    lw = np.ones((2, 3, 4))
    lw[0, 0, 2] = 2
    lw[1, 0, 0] = 2
    y = np.array([[1, 1, 0], [0, -1, 2]])
    assert T.two_head_accuracy(logits, lw, y, counts=True) == (2, 1, 3)
    a1, a2 = T.two_head_accuracy(logits, lw, y)
    assert a1 == 2 / 3 and a2 == 1 / 3
    assert T.two_head_accuracy(logits, lw, np.full_like(y, -1)) == (0.0, 0.0)          # no labelled row
    y2 = y.copy()
    y2[0, 1] = 0                                                                       # the first index of the tie: a hit
    assert T.two_head_accuracy(logits, lw, y2, counts=True) == (3, 2, 3)


ADAM_WRONG = ("no_clip", "step_minus_1", "step_plus_1", "no_bias_correction", "eps_in_root", "eps_on_vhat")


@pytest.mark.parametrize("name", list(U.ADAM_CONFIGS))
def test_adam_bound_holds_for_fp32_and_excludes_wrong_optimizers(name):
    """The bound tests/test_gpu_train_optimizer.py applies to the device, on the very gradients it uses: (a) tr_adam_kernel's
    operation order in np.float32 stays within HALF of it at every step, so fp32 rounding cannot fail the device test;
    (b) every wrong variant of the float64 oracle leaves it by more than 100x on at least 5 % of the elements at the last
    step, so each of those mistakes in the kernel or in the host's lr_t would."""
    kind, size, steps, lr, clip, b1, b2, eps = U.ADAM_CONFIGS[name]
    w, cfg, kind = U.adam_weights(name)
    layout, total = U.flat_layout(w, cfg, kind)
    if size == "big":
        assert total > U.GRID_LIMIT + 1
    p0 = U.flatten(w, layout, total)
    G = U.adam_gradients(layout, total, steps)
    assert G.dtype == np.float32 and G.shape == (steps, total)
    real = np.zeros(total, bool)
    for off, n in layout.values():
        real[off:off + n] = True
    assert not G[:, ~real].any()                                                        # padding gets zeros
    assert 0.05 < (G[:, real] == 0).mean() and (np.abs(G) > 0.1).any() and ((np.abs(G) < 1e-8) & (G != 0)).any()
    ref = U.adam_reference(p0, G, lr, clip, b1, b2, eps)
    emu = U.adam_fp32_emulation(p0, G, lr, clip, b1, b2, eps)
    for k in range(steps):
        ratio = np.abs(emu[k] - ref[k]) / U.adam_bound(k + 1, ref[k], U.f32c(lr))
        assert ratio.max() <= 0.5, (name, k + 1, float(ratio.max()))
    bound = U.adam_bound(steps, ref[-1], U.f32c(lr))
    for variant in ADAM_WRONG:
        if variant == "no_clip" and not clip:
            continue
        wrong = U.adam_reference(p0, G, lr, clip, b1, b2, eps, variant=variant)[-1]
        outside = ~(np.abs(wrong - ref[-1]) <= 100 * bound)                             # (a NaN is outside)
        assert outside.mean() >= 0.05, (name, variant, float(outside.mean()))
    if size == "big":                                 # the elements the device test names have moved far more than the bound
        for i in (U.GRID_LIMIT - 1, U.GRID_LIMIT, U.GRID_LIMIT + 1):
            assert real[i] and abs(ref[-1][i] - p0[i]) > 100 * bound[i]
        off, n = layout["output_b"]
        assert off + n == total and (np.abs(ref[-1] - p0)[off:off + n] > 100 * bound[off:off + n]).mean() > 0.5


def test_device_constants_are_not_the_decimal_ones():
    """float32(0.999): 1 - b2 differs from 1e-3 by 1.3e-5 relative — the oracle must get the constants the device has."""
    assert abs((1 - U.f32c(0.999)) / 1e-3 - 1) > 1e-5


@pytest.mark.parametrize("kind", ["adaptive", "gridtd"])
@pytest.mark.parametrize("with_masks", [False, True])
def test_accuracy_case_conditions(kind, with_masks):
    """The inputs of the device's accuracy test decide something: the two expected accuracies differ from each other and
    from 0 and 1, and in every labelled row both heads' top-1 to top-2 margin exceeds 1e-3 max|logit| (a hundred times the
    forward's fp32 error: no decision depends on rounding, no exact tie at the maximum)."""
    w, X, cap_in, y, lw, masks, logits, (h1, h2, n) = U.accuracy_case(kind, with_masks)
    assert cap_in.shape == (4, 6) and (masks is not None) == with_masks
    assert (y[1, -2:] == -1).all() and n == 19                                          # the padded tail of _case is kept
    assert 0 < h1 < n and 0 < h2 < n and h1 != h2
    if kind == "gridtd" and with_masks:
        assert (logits == 0).mean() > 0.3                                               # the logits carry their Dropout mask
    keep = y[:, :-1] >= 0
    for z in (logits[:, :-1], logits[:, :-1] * lw[:, :-1].astype(np.float64)):
        s = np.sort(z, axis=-1)
        assert ((s[..., -1] - s[..., -2])[keep]).min() > 1e-3 * np.abs(z).max()
