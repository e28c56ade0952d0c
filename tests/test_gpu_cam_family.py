"""-m gpu: the CAM family on the device (lrp_op_cam / _cam_weighted / _scorecam_apply / _feature_ablate, csrc/cam_kernels.h, the
three drivers of saliency.py and their explainer classes) against the numpy restatement (tests/cam_ref.py) and the by-hand path
through the same engine.

Measured shares of the derived bar |got - ref| <= 4 L D 2^-52 mass / (max + 1e-6) (MI355X; profiles/cam_family.txt), the largest
over units, words and launches: lrp_op_cam gradcam 0.0058, gradcam++ 0.0078, xgradcam 0.0091, layercam 0.0156, hirescam 0.0085;
lrp_op_cam_weighted softmax 0.0156, linear 0.0155, ablation 0.0078.  By geometry (g, upscale, D): (2, 3, 8) 0.0156 (two units in
the last place of a bar of 128 of them), (3, 4, 24) 0.0023, (16, 2, 8) 0.0006, (14, 2, 72) 7e-5, (7, 4, 264) 6e-5.  The constant
4 was not widened."""
import numpy as np
import pytest
import torch

import cam_ref as ref
import perturbation_ref as pref
from gpu_util import report
from lrp_imagecaptioning_amd import engine as E
from lrp_imagecaptioning_amd import perturbation as PB
from lrp_imagecaptioning_amd import saliency as SAL
from test_gpu_eval_bbox import CAPS, _explainer
from test_gpu_saliency import KINDS, _log_softmax, _saliency_explainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL3 = [-3.5, 10.25, 0.0]
# (g, upscale, D): a non-power-of-two upscale; a D tail inside a wave; D > 256; L over the four waves; the largest g
GEOMETRIES = [(2, 3, 8), (3, 4, 24), (7, 4, 264), (14, 2, 72), (16, 2, 8)]
# the draw of each geometry: the first seed at which unit 3 (the one launched alone) and at least one more unit have a cam that
# is somewhere positive in every form (with sigma = 20 a zero-mean gradient often blurs to a map of one sign), found on
# cam_ref alone and asserted by test_inputs_meet_their_conditions
SEED = {(2, 3, 8): 1, (3, 4, 24): 0, (7, 4, 264): 1, (14, 2, 72): 0, (16, 2, 8): 1}
B, NMAX, C = 3, 5, 3
_CACHE = {}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------- op_cam
def case(geom):
    """F = max(N(0, 1), 0) (post-ReLU, as in practice); G[l][c] = u[l][c] / (1 + S_c), u uniform in (-1, 1), S_c the channel sum
    of the unit's image: |S_c G| < 1, so Grad-CAM++'s 2 + S_c G lies in (1, 3).  Inputs and every reference, computed once."""
    if geom not in _CACHE:
        g, up, D = geom
        rs = np.random.RandomState(SEED[geom])
        L, S = g * g, g * up
        feat = np.maximum(rs.randn(B, L, D), 0).astype(np.float32)
        idx = np.array([1, 1, 2, 0, 2])                                # units crossing images
        Sc = feat.astype(np.float64).sum(axis=1)                        # (B, D)
        grads = (rs.uniform(-1, 1, size=(NMAX, L, D)) / (1.0 + Sc[idx][:, None, :])).astype(np.float32)
        gb = rs.randn(NMAX, S, S, C).astype(np.float32)
        want = {m: [ref.cam(feat[idx[u]], grads[u], m, g, up) for u in range(NMAX)] for m in ref.MODES}
        for a in (feat, idx, grads, gb):
            a.setflags(write=False)
        _CACHE[geom] = (feat, idx, grads, gb, want)
    return _CACHE[geom]


def launch(geom, units, mode, gate, idx=None, grads=None):
    g, up, _ = geom
    feat, idx0, grads0, gb, _ = case(geom)
    idx = idx0 if idx is None else idx
    grads = grads0 if grads is None else grads
    r = E.op_cam(_t(feat), idx[units], _t(grads[units]), g, up, mode, gb=_t(gb[units]) if gate else None)
    return (r[1].cpu().numpy(), r[0].cpu().numpy()) if gate else (r.cpu().numpy(), None)


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_inputs_meet_their_conditions(geom):
    """on the CPU arrays alone: the Grad-CAM++ denominator 2 G^2 + S_c G^3 = G^2 (2 + S_c G) is well conditioned"""
    feat, idx, grads, _, want = case(geom)
    Sc = feat.astype(np.float64).sum(axis=1)
    t = 2.0 + Sc[idx][:, None, :] * grads.astype(np.float64)
    assert (np.abs(t) > 1.0).all() and (feat >= 0).all() and np.abs(grads).max() < 1.0
    for m in ref.MODES:
        live = [bool(c.any()) for c, _ in want[m]]                      # a form whose every cam were zero would test nothing
        assert live[3] and sum(live) >= 2, (m, live)


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_cam_matches_float64(geom, mode, n, gate):
    g, up, D = geom
    _, _, _, gb, want = case(geom)
    units = [3] if n == 1 else list(range(n))
    cam, out = launch(geom, units, mode, gate)
    assert cam.shape == (n, g * up, g * up) and cam.dtype == np.float64
    share = 0.0
    for j, u in enumerate(units):
        w, bar = want[mode][u]
        err = np.abs(cam[j] - w)
        share = max(share, float((err / np.maximum(bar, 1e-300)).max()))
        assert (err <= bar).all(), (mode, u, share)
    print("op_cam", geom, mode, n, "share of the bar %.3e" % share)
    report("op_cam", g=g, upscale=up, D=D, mode=mode, n=n, share_of_bar=share)
    if gate:                                                            # one IEEE multiply of numpy's float32 -> float64 promotion
        assert _same_bits(out, gb[units].astype(np.float64) * cam[..., None])


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_gradcam_mode_equals_op_gradcam_bit_for_bit(geom):
    g, up, _ = geom
    feat, idx, grads, gb, _ = case(geom)
    units = list(range(NMAX))
    cam, out = launch(geom, units, "gradcam", True)
    o0, c0 = E.op_gradcam(_t(feat), idx, _t(grads), g, up, gb=_t(gb))
    assert _same_bits(cam, c0.cpu().numpy()) and _same_bits(out, o0.cpu().numpy())
    assert _same_bits(launch(geom, units, "gradcam", False)[0], E.op_gradcam(_t(feat), idx, _t(grads), g, up).cpu().numpy())


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_unit_does_not_depend_on_the_launch_and_a_bad_index_is_nan(geom, mode):
    feat, idx, _, _, _ = case(geom)
    units = list(range(NMAX))
    cam, out = launch(geom, units, mode, True)
    alone_cam, alone_out = launch(geom, [3], mode, True)
    assert _same_bits(alone_cam[0], cam[3]) and _same_bits(alone_out[0], out[3])
    back_cam, _ = launch(geom, units[::-1], mode, False)
    assert _same_bits(back_cam[::-1], cam)
    for bad in (B, -1):                                                 # unit 2 points outside the batch: NaN there, nowhere else
        idx2 = np.array(idx)
        idx2[2] = bad
        c2, o2 = launch(geom, units, mode, True, idx=idx2)
        assert np.isnan(c2[2]).all() and np.isnan(o2[2]).all()
        keep = [0, 1, 3, 4]
        assert _same_bits(c2[keep], cam[keep]) and _same_bits(o2[keep], out[keep])


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_a_nowhere_positive_cam_is_exact_zeros(geom):
    _, _, grads, _, _ = case(geom)
    neg = -np.abs(grads)
    cam, out = launch(geom, list(range(NMAX)), "layercam", True, grads=neg)
    assert not cam.any() and not out.any() and not np.isnan(cam).any()
    cam, _ = launch(geom, [1], "gradcam", False, grads=neg)             # F >= 0 and every weight <= 0
    assert not cam.any()


# ---------------------------------------------------------------------------------------------------- op_cam_weighted
def _weighted_scores(rs, n_img, D, T, mode, quantum=None):
    R = 1 + D + (mode == "linear")
    s = rs.randn(n_img, R, T) * rs.choice([1e-2, 1.0, 6.0], size=(n_img, 1, T))
    if quantum is not None:
        s = np.round(s / quantum) * quantum
    return s


def _check_weighted(got, scores, feat, idx, mode, g, up, what):
    share = 0.0
    for i in range(scores.shape[0]):
        want, bar = ref.cam_weighted(scores[i], feat[idx[i]], mode, g, up)
        err = np.abs(got[i] - want)
        share = max(share, float((err / np.maximum(bar, 1e-300)).max()))
        assert (err <= bar).all(), (what, i, share)
    return share


@pytest.mark.parametrize("T", [1, 8, 11])
@pytest.mark.parametrize("mode", ref.WEIGHTS)
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_cam_weighted_matches_float64(geom, mode, T):
    g, up, D = geom
    feat = case(geom)[0]
    rs = np.random.RandomState(T + D)
    idx = np.array([2, 0])
    scores = _weighted_scores(rs, 2, D, T, mode)
    maps, cam = E.op_cam_weighted(_t(scores), _t(feat), idx, g, up, mode, want_cam=True)
    assert maps.shape == (2, T, g * up, g * up) and maps.dtype == torch.float32 and cam.dtype == torch.float64
    cam, maps = cam.cpu().numpy(), maps.cpu().numpy()
    share = _check_weighted(cam, scores, feat, idx, mode, g, up, "cam_weighted %s %s" % (geom, mode))
    print("op_cam_weighted", geom, mode, T, "share of the bar %.3e" % share)
    report("op_cam_weighted", g=g, upscale=up, D=D, mode=mode, T=T, share_of_bar=share)
    assert cam.any()
    assert _same_bits(maps, cam.astype(np.float32))                     # the float32 map is the cam rounded once
    only = E.op_cam_weighted(_t(scores), _t(feat), idx, g, up, mode).cpu().numpy()      # without the float64 output: the same bits
    assert _same_bits(only, maps)
    # an image alone, and a word alone, equal their place among the others
    one = E.op_cam_weighted(_t(scores[1:]), _t(feat), idx[1:], g, up, mode).cpu().numpy()
    assert _same_bits(one[0], maps[1])
    word = E.op_cam_weighted(_t(scores[:1, :, T - 1:]), _t(feat), idx[:1], g, up, mode).cpu().numpy()
    assert _same_bits(word[0, 0], maps[0, T - 1])


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_softmax_is_shift_invariant(geom):
    """Add 1000 to a column (one word, every row): the map stays within the bar of the unshifted reference.  The scores are
    multiples of 2^-30 below 2^5, so the shifted column is exactly representable: what is tested is the kernel's max subtraction
    and not the rounding of the test's own input (a random double + 1000 moves by up to 2^-44, 6e-14, more than the whole bar
    4 L D 2^-52 = 3e-14 of the smallest geometry).  A kernel without the subtraction overflows exp(1000) to inf and fails."""
    g, up, D = geom
    feat = case(geom)[0]
    rs = np.random.RandomState(D)
    idx = np.array([1, 2])
    scores = _weighted_scores(rs, 2, D, 8, "softmax", quantum=2.0 ** -30)
    assert np.abs(scores).max() < 32.0
    shifted = np.array(scores)
    shifted[:, :, 3] += 1000.0
    assert np.array_equal(shifted[:, :, 3] - 1000.0, scores[:, :, 3])
    _, cam = E.op_cam_weighted(_t(shifted), _t(feat), idx, g, up, "softmax", want_cam=True)
    share = _check_weighted(cam.cpu().numpy(), scores, feat, idx, "softmax", g, up, "softmax shift %s" % (geom,))
    report("op_cam_weighted_shift", g=g, upscale=up, D=D, share_of_bar=share)


@pytest.mark.parametrize("mode", ref.WEIGHTS)
def test_weighted_zero_base_score_nan_score_and_bad_index(mode):
    g, up, D = GEOMETRIES[1]
    feat = case(GEOMETRIES[1])[0]
    rs = np.random.RandomState(9)
    idx = np.array([0, 2])
    scores = _weighted_scores(rs, 2, D, 8, mode)
    clean = E.op_cam_weighted(_t(scores), _t(feat), idx, g, up, mode).cpu().numpy()
    s = np.array(scores)
    s[1, 1 + 5, 2] = np.nan                                             # one NaN score: its own word only
    got = E.op_cam_weighted(_t(s), _t(feat), idx, g, up, mode).cpu().numpy()
    assert np.isnan(got[1, 2]).all()
    got[1, 2] = clean[1, 2]
    assert _same_bits(got, clean)
    if mode == "ablation":
        s = np.array(scores)
        s[0, 0, 4] = 0.0                                                # s_0 == 0: every weight 0, the map exact zeros
        got = E.op_cam_weighted(_t(s), _t(feat), idx, g, up, mode).cpu().numpy()
        assert not got[0, 4].any() and not np.isnan(got).any()
        got[0, 4] = clean[0, 4]
        assert _same_bits(got, clean)
    bad = E.op_cam_weighted(_t(scores), _t(feat), np.array([0, B]), g, up, mode).cpu().numpy()
    assert np.isnan(bad[1]).all() and _same_bits(bad[0], clean[0])


# ---------------------------------------------------------------------------------------------------- apply and ablate
# (g, upscale, D): sides 6, 12, 35 (35 * 35 * 3 values: no multiple of four, the scalar path with a tail group) and 28
APPLY_CASES = [(2, 3, 8), (3, 4, 24), (7, 5, 264), (14, 2, 72)]


def _apply_rows(rs, D, hi, n=37):
    """n rows over B images, k from [-1, hi], every special k at least once and one k outside"""
    idx = rs.randint(0, B, size=n)
    ks = rs.randint(-1, hi + 1, size=n)
    ks[:4] = [-1, hi, 0, hi + 1]                                        # the copy, the last valid k, channel 0, an invalid k
    idx[4], ks[4] = 0, 1                                                # the dead channel of image 0 (below)
    idx[5], ks[5] = 1, 2                                                # the constant channel of image 1
    return idx, ks


@pytest.mark.parametrize("geom", APPLY_CASES)
def test_scorecam_apply_equals_the_restatement_bit_for_bit(geom):
    g, up, D = geom
    S = g * up
    rs = np.random.RandomState(S)
    x = rs.uniform(-120, 130, size=(B, S, S, C)).astype(np.float32)
    feat = np.maximum(rs.randn(B, g * g, D), 0).astype(np.float32)
    feat[0, :, 1] = 0.0                                                 # a dead channel
    feat[1, :, 2] = 0.625                                               # a constant one
    idx, ks = _apply_rows(rs, D, D)
    got = E.op_scorecam_apply(_t(x), _t(feat), idx, ks, g, up, FILL3).cpu().numpy()
    want = ref.scorecam_apply(x, feat, idx, ks, g, up, FILL3)
    nan = np.isnan(want).all(axis=(1, 2, 3))
    assert nan.sum() == 1 and nan[3] and np.isnan(got[nan]).all() and not np.isnan(got[~nan]).any()
    assert _same_bits(got[~nan], want[~nan])
    fill = np.broadcast_to(np.asarray(FILL3, dtype=np.float32), (S, S, C))
    assert _same_bits(got[0], x[idx[0]]) and _same_bits(got[1], fill)   # k = -1 the image, k = D the fill image
    assert _same_bits(got[4], fill) and _same_bits(got[5], fill)        # dead and constant channels: the mask is zeros
    bad = E.op_scorecam_apply(_t(x), _t(feat), [B, -1], [0, 0], g, up, FILL3).cpu().numpy()
    assert np.isnan(bad).all()
    # any cut of the rows into calls, and any slot, gives the same bits
    parts = np.concatenate([E.op_scorecam_apply(_t(x), _t(feat), idx[:13], ks[:13], g, up, FILL3).cpu().numpy(),
                            E.op_scorecam_apply(_t(x), _t(feat), idx[13:], ks[13:], g, up, FILL3).cpu().numpy()])
    assert _same_bits(parts[~nan], got[~nan])
    back = E.op_scorecam_apply(_t(x), _t(feat), idx[::-1].copy(), ks[::-1].copy(), g, up, FILL3).cpu().numpy()[::-1]
    assert _same_bits(back[~nan], got[~nan])


def test_scorecam_apply_over_more_than_one_slice():
    """224 x 224 x 3 values per row: 19 slices of a row, the last one short"""
    g, up, D = 14, 16, 16
    rs = np.random.RandomState(5)
    x = rs.uniform(-120, 130, size=(1, 224, 224, C)).astype(np.float32)
    feat = np.maximum(rs.randn(1, g * g, D), 0).astype(np.float32)
    ks = [3, -1, D, 15]
    got = E.op_scorecam_apply(_t(x), _t(feat), [0] * 4, ks, g, up, FILL3).cpu().numpy()
    assert _same_bits(got, ref.scorecam_apply(x, feat, [0] * 4, ks, g, up, FILL3))


@pytest.mark.parametrize("L,D", [(4, 8), (9, 24), (49, 264)])
def test_feature_ablate_is_bit_exact(L, D):
    rs = np.random.RandomState(L)
    feat = rs.randn(B, L, D).astype(np.float32)
    idx, ks = _apply_rows(rs, D, D - 1)
    got = E.op_feature_ablate(_t(feat), idx, ks).cpu().numpy()
    want = ref.feature_ablate(feat, idx, ks)
    nan = np.isnan(want).all(axis=(1, 2))
    assert nan.sum() == 1 and nan[3] and np.isnan(got[nan]).all()
    assert _same_bits(got[~nan], want[~nan])
    assert _same_bits(got[0], feat[idx[0]])                             # k = -1
    parts = np.concatenate([E.op_feature_ablate(_t(feat), idx[:13], ks[:13]).cpu().numpy(),
                            E.op_feature_ablate(_t(feat), idx[13:], ks[13:]).cpu().numpy()])
    assert _same_bits(parts[~nan], got[~nan])
    assert np.isnan(E.op_feature_ablate(_t(feat), [B, 0], [0, -2]).cpu().numpy()).all()
    odd = rs.randn(2, 3, 7).astype(np.float32)                          # 21 values per row: the scalar path
    assert _same_bits(E.op_feature_ablate(_t(odd), [1, 0, 1], [6, -1, 0]).cpu().numpy(), ref.feature_ablate(odd, [1, 0, 1], [6, -1, 0]))


# ---------------------------------------------------------------------------------------------------- the drivers
# the small VGG net of test_gpu_saliency: 32 x 32 images, L = 64 (g = 8, upscale 4), D = 64
G8, UP4 = 8, 4
X_SEED = 11


def _images(n=2):
    return np.random.RandomState(X_SEED).uniform(-120, 130, size=(n, 32, 32, 3)).astype(np.float32)


def _units(caps):
    return [(b, t) for b in range(len(caps)) for t in range(1, len(caps[b]))]


@pytest.mark.parametrize("method,guided", [("gradcam", True), ("gradcam++", False), ("xgradcam", False), ("layercam", True),
                                           ("hirescam", False)])
@pytest.mark.parametrize("kind,cls", KINDS)
def test_gradient_driver_matches_the_by_hand_path(kind, cls, method, guided):
    ex, _ = _explainer(cls, kind, max_images=2)
    eng = ex._engine
    X, caps = _images(), CAPS[:2]                                       # captions of 7 and 5 words: chunks of 2 units cross the images
    res = SAL.GradientCAMSaliency(ex, method, guided=guided).explain(X, caps)
    assert ex.caption is None and eng.precision == "fp32"
    units = _units(caps)
    assert res["units"] == units and res["maps"].shape == (len(units), 32, 32) and res["maps"].dtype == torch.float32
    assert ("guided" in res) == guided
    for j, (b, t) in enumerate(units):                                  # by hand: one unit at a time, straight through the operators
        eng.encode_images(X[b:b + 1])
        eng.decoder_forward([caps[b]])
        d, _ = eng.decoder_gradient([0], [t], want_r_words=False)
        cam = E.op_cam(eng.get_features(), [0], d, G8, UP4, method)
        assert torch.equal(res["maps"][j], cam[0].to(torch.float32)), (j, b, t)
        logit, _ = E.perturb_word_scores(eng, [0], [t], [caps[b][t - 1] - 1])
        assert torch.equal(res["scores0"][j:j + 1], logit)
        if guided:
            if method == "gradcam":                                     # the engine's own chain, bit for bit
                out = eng.guided_gradcam([0], [t])
            else:
                out, _ = E.op_cam(eng.get_features(), [0], d, G8, UP4, method, gb=eng.cnn_walk([0], d, "guided_backprop"))
            assert torch.equal(res["guided"][j], out[0]) and res["guided"].dtype == torch.float64
    assert bool(res["maps"].any()) and bool(torch.isfinite(res["maps"]).all())
    assert [tuple(s.shape) for s in res["scores"]] == [(1, 7), (1, 5)]


def _forward_scores_by_hand(ex, caps, n_img, n_rows, rows_of, enter, score):
    """the (1 + n_rows, T) score matrix of every image: the jobs (image, k = -1 .. n_rows - 1) in chunks of max_images through
    `enter`, decoder_forward and lrp_perturb_word_scores"""
    eng = ex._engine
    jobs = [(b, k) for b in range(n_img) for k in range(-1, n_rows)]
    S = [torch.zeros((1 + n_rows, len(caps[b]) - 1), dtype=torch.float64, device=DEV) for b in range(n_img)]
    for c0 in range(0, len(jobs), eng.max_images):
        part = jobs[c0:c0 + eng.max_images]
        enter(rows_of([b for b, _ in part], [k for _, k in part]))
        eng.decoder_forward([caps[b] for b, _ in part])
        for j, (b, k) in enumerate(part):
            ts = list(range(1, len(caps[b])))
            logit, logp = E.perturb_word_scores(eng, [j] * len(ts), ts, [caps[b][t - 1] - 1 for t in ts])
            S[b][1 + k] = logit if score == "logit" else logp
    return S


def _features_by_hand(eng, X):
    out = []
    for b in range(len(X)):
        eng.encode_images(X[b:b + 1])
        out.append(eng.get_features())
    return torch.cat(out)


@pytest.mark.parametrize("weights,score", [("softmax", "logit"), ("linear", "logp")])
@pytest.mark.parametrize("kind,cls", KINDS)
def test_scorecam_driver_matches_the_by_hand_path(kind, cls, weights, score):
    ex, _ = _explainer(cls, kind, max_images=2)
    eng = ex._engine
    X, caps = _images(), CAPS[:2]
    res = SAL.ScoreCAMSaliency(ex, weights, fill=FILL3, score=score).explain(X, caps)
    assert ex.caption is None and res["units"] == _units(caps)
    D = eng.D
    rows = D + (weights == "linear")
    feat, xd = _features_by_hand(eng, X), _t(X)
    S = _forward_scores_by_hand(ex, caps, 2, rows, lambda bs, ks: E.op_scorecam_apply(xd, feat, bs, ks, G8, UP4, FILL3),
                                eng.encode_images, score)
    u0 = 0
    for b in range(2):
        T = len(caps[b]) - 1
        assert torch.equal(res["scores"][b], S[b]) and torch.equal(res["scores0"][u0:u0 + T], S[b][0])
        maps = E.op_cam_weighted(S[b][None], feat, [b], G8, UP4, weights)
        assert torch.equal(res["maps"][u0:u0 + T], maps[0])
        assert bool((S[b][1:] != S[b][0]).any())                        # the masks move the scores
        u0 += T
    # softmax weights are positive and the features non-negative: that cam cannot vanish.  Linear weights can all be negative
    # (every mask scores below the fill image): the cam is then exact zeros, which the bit comparison above covers
    assert bool(torch.isfinite(res["maps"]).all()) and (weights != "softmax" or bool(res["maps"].any()))


@pytest.mark.parametrize("kind,cls", KINDS)
def test_ablationcam_driver_matches_the_by_hand_path(kind, cls):
    ex, _ = _explainer(cls, kind, max_images=2)
    eng = ex._engine
    X, caps = _images(), CAPS[:2]
    res = SAL.AblationCAMSaliency(ex).explain(X, caps)
    assert ex.caption is None and res["units"] == _units(caps)
    feat = _features_by_hand(eng, X)
    S = _forward_scores_by_hand(ex, caps, 2, eng.D, lambda bs, ks: E.op_feature_ablate(feat, bs, ks), eng.set_features, "logit")
    u0 = 0
    for b in range(2):
        T = len(caps[b]) - 1
        assert torch.equal(res["scores"][b], S[b])
        assert torch.equal(res["maps"][u0:u0 + T], E.op_cam_weighted(S[b][None], feat, [b], G8, UP4, "ablation")[0])
        assert bool((S[b][1:] != S[b][0]).any())                        # ablating a channel moves the scores
        u0 += T
    assert bool(torch.isfinite(res["maps"]).all())
    # the unablated row of the features equals the image's own forward
    eng.encode_images(X[:1])
    eng.decoder_forward([caps[0]])
    logit, _ = E.perturb_word_scores(eng, [0], [1], [caps[0][0] - 1])
    assert torch.equal(res["scores0"][:1], logit)


def test_drivers_do_not_depend_on_batch_order_or_chunk_size():
    ex2, _ = _explainer("ExplainImgCaptioningAdaptiveAttention", "adaptive", max_images=2, seed=3)
    ex5, _ = _explainer("ExplainImgCaptioningAdaptiveAttention", "adaptive", max_images=5, seed=3)
    X = _images(3)
    caps = [CAPS[0], CAPS[1], CAPS[3]]
    words = [[2, 1], [1, 3, 5], []]                                     # an image without a word, words out of order
    order = [2, 1, 0]
    for make in (lambda ex: SAL.GradientCAMSaliency(ex, "gradcam++", guided=True), lambda ex: SAL.ScoreCAMSaliency(ex),
                 lambda ex: SAL.AblationCAMSaliency(ex, score="logp")):
        a, b = make(ex2).explain(X, caps, words), make(ex5).explain(X, caps, words)
        assert a["units"] == [(0, 2), (0, 1), (1, 1), (1, 3), (1, 5)] == b["units"]
        assert torch.equal(a["maps"], b["maps"]) and torch.equal(a["scores0"], b["scores0"])
        assert a["scores"][2] is None and bool(torch.isfinite(a["maps"]).all())
        c = make(ex5).explain(X[order], [caps[i] for i in order], [words[i] for i in order])
        assert c["units"] == [(1, 1), (1, 3), (1, 5), (2, 2), (2, 1)]
        assert torch.equal(c["maps"], a["maps"][[2, 3, 4, 0, 1]])
        if "guided" in a:
            assert torch.equal(a["guided"], b["guided"]) and torch.equal(c["guided"], a["guided"][[2, 3, 4, 0, 1]])
    with pytest.raises(ValueError):                                     # the CAM family takes no label map
        SAL.ScoreCAMSaliency(ex2).explain(X, caps, words, segments=np.zeros((3, 32, 32), dtype=np.int32))
    with pytest.raises(ValueError):                                     # ... and no image that is not the model's square
        SAL.AblationCAMSaliency(ex2).explain(np.zeros((1, 32, 48, 3), dtype=np.float32), caps[:1])


# ---------------------------------------------------------------------------------------------------- the classes
@pytest.mark.parametrize("cls,kind,kw", [
    ("ExplainImgCaptioningAdaptiveAttentionCAM", "adaptive", {"method": "xgradcam"}),
    ("ExplainImgCaptioningGridTDCAM", "gridtd", {"method": "layercam", "guided": True}),
    ("ExplainImgCaptioningAdaptiveAttentionScoreCAM", "adaptive", {"weights": "linear", "score": "logp"}),
    ("ExplainImgCaptioningGridTDScoreCAM", "gridtd", {}),
    ("ExplainImgCaptioningAdaptiveAttentionAblationCAM", "adaptive", {}),
    ("ExplainImgCaptioningGridTDAblationCAM", "gridtd", {"score": "logp"})])
def test_classes_return_maps_that_move_with_the_image(cls, kind, kw):
    ex, rs = _saliency_explainer(cls, kind, **kw)
    X = rs.uniform(-120, 130, size=(2, 32, 32, 3)).astype(np.float32)
    res = ex.explain_images(X[:1], [CAPS[1]])
    n_words = len(CAPS[1]) - 1
    assert res["maps"].shape == (n_words, 32, 32) and bool(torch.isfinite(res["maps"]).all())
    assert float(res["maps"].min()) >= 0.0 and float(res["maps"].max()) <= 1.0
    other = ex.explain_images(X[1:], [CAPS[1]])
    assert not torch.equal(other["scores0"], res["scores0"])
    if cls.endswith("ScoreCAM") and kw.get("weights", "softmax") == "softmax":     # positive weights: the cam cannot vanish
        assert bool(res["maps"].any()) and not torch.equal(other["maps"], res["maps"])
    assert torch.equal(ex.explain_images(X[:1], [CAPS[1]])["maps"], res["maps"])
    assert ("guided" in res) == bool(kw.get("guided"))
    with pytest.raises(NotImplementedError):
        ex._explain_sentence()


@pytest.mark.parametrize("cls,kw", [("ExplainImgCaptioningAdaptiveAttentionCAM", {"method": "hirescam", "guided": True}),
                                    ("ExplainImgCaptioningAdaptiveAttentionScoreCAM", {}),
                                    ("ExplainImgCaptioningAdaptiveAttentionAblationCAM", {})])
def test_classes_run_on_a_resnet_spec(cls, kw):
    rn = {"stem": 8, "stacks": ((8, 1), (8, 1), (8, 1), (8, 1))}       # L = 49 (g = 7, upscale 32), D = 32
    ex, rs = _saliency_explainer(cls, "adaptive", resnet=rn, hw=224, **kw)
    X = rs.uniform(-120, 130, size=(1, 224, 224, 3)).astype(np.float32)
    res = ex.explain_images(X, [CAPS[2]])
    assert res["maps"].shape == (3, 224, 224) and bool(torch.isfinite(res["maps"]).all())
    assert not cls.endswith("ScoreCAM") or bool(res["maps"].any())      # softmax weights: the cam cannot vanish
    if kw.get("guided"):
        assert res["guided"].shape == (3, 224, 224, 3) and bool(torch.isfinite(res["guided"]).all())


def test_perturbation_analysis_ranks_by_the_scorecam_maps_and_leaves_lrp_alone():
    lrp, rs = _explainer("ExplainImgCaptioningAdaptiveAttention", "adaptive", max_images=2)
    X = rs.uniform(-120, 130, size=(3, 32, 32, 3)).astype(np.float32)
    caps = CAPS[:3]
    pa_lrp = PB.CaptionPerturbationAnalysis(lrp, PB.Perturbation("zeros"), steps=2, regions_per_step=3)
    before = pa_lrp.compute_perturbation_analysis(X, caps)

    ex, _ = _saliency_explainer("ExplainImgCaptioningAdaptiveAttentionScoreCAM", "adaptive", score="logp")
    pa = PB.CaptionPerturbationAnalysis(ex, PB.Perturbation("zeros", channels="all"), steps=2, regions_per_step=3)
    res = pa.compute_perturbation_analysis(X, caps)
    units = _units(caps)
    assert res["units"] == units and ex.caption is None
    # by hand: ranks from the maps broadcast to three channels, restated perturbation, the same engine's forward
    eng, M = ex._engine, ex._engine.max_images
    ranks = []
    for lo in range(0, 3, M):
        maps = ex.explain_images(X[lo:lo + M], caps[lo:lo + M])["maps"].cpu().numpy()
        ranks.append(pref.region_ranks(np.repeat(maps[..., None], 3, axis=-1), (9, 9)))
    ranks = np.concatenate(ranks)
    want = np.empty((3, len(units)))
    for lo in range(0, 3, M):
        eng.encode_images(X[lo:lo + M])
        eng.decoder_forward(caps[lo:lo + M])
        preds = eng.read_state("caption_preds").cpu().numpy()
        for j, (b, t) in enumerate(units):
            if lo <= b < lo + M:
                want[0, j] = _log_softmax(preds[b - lo, t - 1])[caps[b][t - 1] - 1]
    for s, k in enumerate((1, 4)):
        for c0 in range(0, len(units), M):
            chunk = units[c0:c0 + M]
            eng.encode_images(pref.perturbate(X, ranks[c0:c0 + M], k, (9, 9), "zeros", img_idx=[b for b, _ in chunk], all_channels=True))
            eng.decoder_forward([caps[b] for b, _ in chunk])
            preds = eng.read_state("caption_preds").cpu().numpy()
            for j, (b, t) in enumerate(chunk):
                want[s + 1, c0 + j] = _log_softmax(preds[j, t - 1])[caps[b][t - 1] - 1]
    err = np.abs(res["logp"] - want).max()
    assert err <= 1e-12, err
    assert (res["logp"][1:] != res["logp"][0]).any()

    after = pa_lrp.compute_perturbation_analysis(X, caps)              # the new classes leave the others alone
    assert _same_bits(after["logp"], before["logp"]) and _same_bits(after["logit"], before["logit"])
    report("perturbation_with_scorecam", max_abs=float(err))
