"""-m gpu: the perturbation analysis on the device (lrp_perturb_*, perturbation.py) against the reference's own outputs
(tests/golden/perturbation_*.npz) and the numpy restatement (tests/perturbation_ref.py)."""
import numpy as np
import pytest
import torch

import perturbation_ref as ref
from gpu_util import report
from lrp_imagecaptioning_amd import engine as E
from lrp_imagecaptioning_amd import perturbation as PB
from test_gpu_eval_bbox import CAPS, _explainer, _relevance_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module", params=ref.GOLDENS)
def golden(request):
    return ref.load_golden(request.param)


# ---------------------------------------------------------------------------------------------------- against the goldens
def test_ranks_equal_the_reference(golden):
    region = tuple(golden["region"])
    for dtype in (np.float32, np.float64):
        ranks, scores = E.perturb_ranks(_t(golden["analysis"].astype(dtype)), region, want_scores=True)
        assert ranks.dtype == torch.int32 and scores.dtype == torch.float64
        assert np.array_equal(ranks.cpu().numpy(), golden["ranks"])
        want = ref.region_scores(golden["analysis"], region)
        assert np.abs(scores.cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max()


def test_apply_equals_the_reference_at_every_function_k_and_range(golden):
    region = tuple(golden["region"])
    x = _t(golden["x"])
    n = len(golden["x"])
    ranks = E.perturb_ranks(_t(golden["analysis"]), region)
    worst = 0.0
    for ri, rng in enumerate(ref.RANGES):
        for fn in ref.FUNCTIONS:
            for ki, k in enumerate(golden["ks"]):
                got = E.perturb_apply(x, list(range(n)), ranks, float(k), region, mode=fn, value_range=rng).cpu().numpy()
                worst = max(worst, ref.check_against_golden(golden, fn, ki, ri, got))
                # and bit-equal to the restatement, 'mean' included
                want = ref.perturbate(golden["x"], golden["ranks"], k, region, fn, value_range=rng)
                assert np.array_equal(_bits(got), _bits(want)), (fn, ki, ri)
    report("perturb_apply_golden", regions=int(ranks.shape[1]), mean_max_abs=worst)


def test_perturbation_class_matches_the_reference(golden):
    region = tuple(golden["region"])
    for fn, ki, ri in (("zeros", 3, 0), ("mean", 2, 1), ("invert", 4, 1)):
        k = golden["ks"][ki]
        p = PB.Perturbation(fn, num_perturbed_regions=int(k) if float(k).is_integer() else float(k), region_shape=region,
                            value_range=ref.RANGES[ri])
        got = p.perturbate_on_batch(golden["x"], golden["analysis"])
        assert isinstance(got, np.ndarray)
        ref.check_against_golden(golden, fn, ki, ri, got)
        dev = p.perturbate_on_batch(_t(golden["x"]), _t(golden["analysis"]))
        assert torch.is_tensor(dev) and dev.is_cuda and np.array_equal(_bits(dev.cpu().numpy()), _bits(got))
        assert np.array_equal(p.region_ranks(golden["analysis"]), golden["ranks"])


# ---------------------------------------------------------------------------------------------------- against the restatement
def _separated(rs, n, hw, dtype, region, reduce, aggregate):
    """Heat-maps whose restated fp64 region scores are no closer than 1e-9 relative (asserted, not assumed)."""
    R = (rs.randn(n, hw, hw, 3) * rs.choice([1e-3, 1.0, 50.0], size=(n, 1, 1, 1))).astype(dtype)
    s = ref.region_scores(R, region, reduce, aggregate)
    assert ref.min_relative_gap(s) > 1e-9
    return R, s


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("hw,n,seed", [(32, 7, 11), (224, 5, 12)])
@pytest.mark.parametrize("reduce,aggregate", [("mean", "mean"), ("max", "mean"), ("mean", "max")])
def test_ranks_and_scores_match_restatement(dtype, hw, n, seed, reduce, aggregate):
    rs = np.random.RandomState(seed)
    R, want = _separated(rs, n, hw, dtype, (9, 9), reduce, aggregate)
    ranks, scores = E.perturb_ranks(_t(R), (9, 9), reduce, aggregate, want_scores=True)
    assert ranks.shape == (n, 16 if hw == 32 else 625)
    got = scores.cpu().numpy()
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all()
    assert np.array_equal(ranks.cpu().numpy(), ref.ranks_from_scores(want))
    neg, nscores = E.perturb_ranks(_t(R), (9, 9), reduce, aggregate, want_scores=True, negate=True)
    assert np.array_equal(nscores.cpu().numpy(), -got)
    assert np.array_equal(neg.cpu().numpy(), ref.ranks_from_scores(-want))


@pytest.mark.parametrize("hw", [32, 224])
def test_ties_and_degenerate_maps_rank_in_the_stable_order(hw):
    rs = np.random.RandomState(3)
    for dtype in (np.float32, np.float64):
        R = _relevance_batch(rs, 6, hw, hw, dtype)
        R[5, 0, 0, 0] = np.nan                                         # one NaN region: last
        for reduce, aggregate in (("mean", "mean"), ("max", "max")):
            got = E.perturb_ranks(_t(R), (9, 9), reduce, aggregate).cpu().numpy()
            want = ref.region_ranks(R, (9, 9), reduce, aggregate)
            assert np.array_equal(got, want), (dtype, reduce)
            assert np.array_equal(got[0], np.arange(got.shape[1]))     # all zero: raster order
            assert got[5, 0] == got.shape[1] - 1
    # the all-zero map perturbs in raster order
    x = rs.randn(1, hw, hw, 3).astype(np.float32)
    out = E.perturb_apply(_t(x), [0], _t(got[:1]), 2.0, (9, 9)).cpu().numpy()
    reg = ref._region_of_pixels(hw, hw, (9, 9))
    assert not out[0, ..., 0][reg < 2].any() and np.array_equal(out[0, ..., 0][reg >= 2], x[0, ..., 0][reg >= 2])
    assert np.array_equal(out[..., 1:], x[..., 1:])


@pytest.mark.parametrize("hw", [32, 224])
def test_apply_matches_restatement_with_options(hw):
    rs = np.random.RandomState(hw)
    B, n = 3, 6
    x = rs.uniform(-120, 130, size=(B, hw, hw, 3)).astype(np.float32)
    R, _ = _separated(rs, n, hw, np.float32, (9, 9), "mean", "mean")
    ranks = E.perturb_ranks(_t(R), (9, 9))
    rh = ranks.cpu().numpy()
    idx = [2, 0, 0, 1, 2, 2]                                            # any order, with repeats
    nreg = rh.shape[1]
    k = np.array([0, 1, 2.5, 7, nreg, nreg + 3], dtype=np.float64)
    noise = rs.normal(0, 0.3, size=(n, hw, hw, 3)).astype(np.float32)
    for mode in ("zeros", "mean", "invert", "noise"):
        for allc in (False, True):
            for rng in (None, (-100.0, 60.5)):
                got = E.perturb_apply(_t(x), idx, ranks, k, (9, 9), mode=mode, noise=_t(noise) if mode == "noise" else None,
                                      all_channels=allc, value_range=rng).cpu().numpy()
                want = ref.perturbate(x, rh, k, (9, 9), mode, img_idx=idx, noise=noise, all_channels=allc, value_range=rng)
                assert np.array_equal(_bits(got), _bits(want)), (mode, allc, rng)
    # noise: inside the perturbed regions the output is the noise, outside it is x
    got = E.perturb_apply(_t(x), idx, ranks, k, (9, 9), mode="noise", noise=_t(noise), all_channels=True).cpu().numpy()
    reg = ref._region_of_pixels(hw, hw, (9, 9))
    for u in range(n):
        inside = (rh[u] <= k[u] - 1)[reg]
        assert np.array_equal(got[u][inside], noise[u][inside]) and np.array_equal(got[u][~inside], x[idx[u]][~inside])
    assert np.array_equal(got[0], x[2]) and np.array_equal(got[4], noise[4])
    # channels='all' of the class is that switch
    p = PB.Perturbation("mean", num_perturbed_regions=3, channels="all")
    got = p.perturbate_on_batch(x, R[:B])
    assert np.array_equal(_bits(got), _bits(ref.perturbate(x, rh[:B], 3, (9, 9), "mean", all_channels=True)))
    assert (got[..., 1] != x[..., 1]).any()


def test_gaussian_draws_from_the_callers_generator():
    rs = np.random.RandomState(5)
    x = rs.randn(2, 32, 32, 3).astype(np.float32)
    R = rs.randn(2, 32, 32, 3).astype(np.float32)
    outs = []
    for _ in range(2):
        g = torch.Generator(device=DEV)
        g.manual_seed(7)
        outs.append(PB.Perturbation("gaussian", num_perturbed_regions=4, generator=g).perturbate_on_batch(x, R))
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    inside = (ref.region_ranks(R, (9, 9)) <= 3)[:, ref._region_of_pixels(32, 32, (9, 9))]
    assert np.array_equal(outs[0][..., 1:], x[..., 1:]) and np.array_equal(outs[0][..., 0][~inside], x[..., 0][~inside])
    v = outs[0][..., 0][inside]
    assert (v != x[..., 0][inside]).all() and abs(v.std() - 0.3) < 0.05 and abs(v.mean()) < 0.05


def test_a_unit_alone_and_in_a_batch_of_40_is_bit_identical():
    rs = np.random.RandomState(9)
    n, hw = 40, 224
    x = rs.uniform(-120, 130, size=(4, hw, hw, 3)).astype(np.float32)
    R = rs.randn(n, hw, hw, 3).astype(np.float32)
    idx = rs.randint(0, 4, size=n).astype(np.int32)
    k = rs.randint(0, 40, size=n).astype(np.float64)
    ranks, scores = E.perturb_ranks(_t(R), (9, 9), want_scores=True)
    out = E.perturb_apply(_t(x), idx, ranks, k, (9, 9), mode="mean", value_range=(-100.0, 100.0))
    for i in (0, 17, 39):
        r1, s1 = E.perturb_ranks(_t(R[i:i + 1]), (9, 9), want_scores=True)
        assert torch.equal(r1[0], ranks[i]) and np.array_equal(_bits(s1[0].cpu().numpy()), _bits(scores[i].cpu().numpy()))
        o1 = E.perturb_apply(_t(x), idx[i:i + 1], r1, k[i:i + 1], (9, 9), mode="mean", value_range=(-100.0, 100.0))
        assert np.array_equal(_bits(o1[0].cpu().numpy()), _bits(out[i].cpu().numpy()))


def test_an_index_outside_the_batch_comes_out_nan():
    rs = np.random.RandomState(2)
    x = rs.randn(2, 20, 29, 3).astype(np.float32)
    ranks = E.perturb_ranks(_t(rs.randn(4, 20, 29, 3).astype(np.float32)), (9, 9))
    out = E.perturb_apply(_t(x), [1, -1, 2, 0], ranks, 3.0, (9, 9), mode="mean").cpu().numpy()
    assert np.isnan(out[1]).all() and np.isnan(out[2]).all()
    assert not np.isnan(out[0]).any() and not np.isnan(out[3]).any()
    want = ref.perturbate(x, ranks.cpu().numpy(), 3.0, (9, 9), "mean", img_idx=[1, -1, 2, 0])
    assert np.array_equal(_bits(out[[0, 3]]), _bits(want[[0, 3]]))


# ---------------------------------------------------------------------------------------------------- the word's score
def _log_softmax(row):
    m = row.max()
    return row - (m + np.log(np.exp(row - m).sum()))


@pytest.mark.parametrize("kind,cls", [("adaptive", "ExplainImgCaptioningAdaptiveAttention"),
                                      ("gridtd", "ExplainImgCaptioningGridTDModel")])
def test_word_scores_match_numpy_on_the_cached_logits(kind, cls):
    ex, rs = _explainer(cls, kind, max_images=2)
    eng = ex._engine
    with pytest.raises(RuntimeError):
        E.perturb_word_scores(eng, [0], [1], [0])                       # no forward yet
    X = rs.uniform(-120, 130, size=(2, 32, 32, 3)).astype(np.float32)
    eng.encode_images(X)
    eng.decoder_forward(CAPS[:2])
    preds = eng.read_state("caption_preds").cpu().numpy()
    units = [(b, t) for b in range(2) for t in range(1, len(CAPS[b]) + 1)]
    cols = [CAPS[b][t - 1] - 1 for b, t in units]
    logit, logp = E.perturb_word_scores(eng, [u[0] for u in units], [u[1] for u in units], cols)
    logit, logp = logit.cpu().numpy(), logp.cpu().numpy()
    V = preds.shape[2]
    worst = 0.0
    for j, (b, t) in enumerate(units):
        row = preds[b, t - 1]
        assert logit[j] == row[cols[j]]
        worst = max(worst, abs(logp[j] - _log_softmax(row)[cols[j]]))
    assert worst <= V * 2.0 ** -52, worst
    bad_logit, bad_logp = E.perturb_word_scores(eng, [0, 2, 0, 0, -1], [1, 1, 0, eng.Tm + 1, 1], [0, 0, 0, 0, V])
    assert np.isnan(bad_logp.cpu().numpy()[1:]).all() and np.isnan(bad_logit.cpu().numpy()[1:]).all()
    assert abs(bad_logp.cpu().numpy()[0] - _log_softmax(preds[0, 0])[0]) <= V * 2.0 ** -52
    report("perturb_word_scores", kind=kind, max_abs=worst, bound=V * 2.0 ** -52)


# ---------------------------------------------------------------------------------------------------- the driver
def _heatmaps_by_hand(ex, ii, ts):
    from lrp_imagecaptioning_amd.explainers import _GradientMixin, _GuidedGradcamMixin
    eng = ex._engine
    if isinstance(ex, _GuidedGradcamMixin):
        return eng.guided_gradcam(ii, ts)
    if isinstance(ex, _GradientMixin):
        d, _ = eng.decoder_gradient(ii, ts, want_r_words=False)
        return eng.cnn_walk(ii, d, ex._walk)
    return eng.explain_tokens(ii, ts)[0]


def _by_hand(ex, X, caps, units, ks, region, mode="zeros", all_channels=False, negate=False):
    """(len(ks) + 1, n) log-probabilities: restatement on the host, encode_images, decoder_forward and numpy log-softmax on
    the same engine, in the chunks the driver uses (max_images images, then max_images units)."""
    eng = ex._engine
    M = eng.max_images
    n = len(units)
    out = np.empty((len(ks) + 1, n))
    ranks = np.empty((n, np.prod(ref.geometry(X.shape[1], X.shape[2], region)[:2])), dtype=np.int32)
    for lo in range(0, len(X), M):
        sel = [j for j, (b, _) in enumerate(units) if lo <= b < lo + M]
        if not sel:
            continue
        eng.encode_images(X[lo:lo + M])
        eng.decoder_forward(caps[lo:lo + M])
        preds = eng.read_state("caption_preds").cpu().numpy()
        for j in sel:
            b, t = units[j]
            out[0, j] = _log_softmax(preds[b - lo, t - 1])[caps[b][t - 1] - 1]
        R = _heatmaps_by_hand(ex, [units[j][0] - lo for j in sel], [units[j][1] for j in sel]).cpu().numpy()
        ranks[sel] = ref.region_ranks(R, region, negate=negate)
    for s, k in enumerate(ks):
        for c0 in range(0, n, M):
            chunk = units[c0:c0 + M]
            xp = ref.perturbate(X, ranks[c0:c0 + M], k, region, mode, img_idx=[b for b, _ in chunk], all_channels=all_channels)
            eng.encode_images(xp)
            eng.decoder_forward([caps[b] for b, _ in chunk])
            preds = eng.read_state("caption_preds").cpu().numpy()
            for j, (b, t) in enumerate(chunk):
                out[s + 1, c0 + j] = _log_softmax(preds[j, t - 1])[caps[b][t - 1] - 1]
    return out, ranks


DRIVER_CASES = [("adaptive", "ExplainImgCaptioningAdaptiveAttention"), ("gridtd", "ExplainImgCaptioningGridTDModel"),
                ("adaptive", "ExplainImgCaptioningAdaptiveAttentionGradient"), ("gridtd", "ExplainImgCaptioningGridTDGuidedGradcam")]


@pytest.mark.parametrize("kind,cls", DRIVER_CASES)
def test_driver_matches_the_by_hand_path(kind, cls):
    ex, rs = _explainer(cls, kind, max_images=2)
    X = rs.uniform(-120, 130, size=(4, 32, 32, 3)).astype(np.float32)
    pa = PB.CaptionPerturbationAnalysis(ex, PB.Perturbation("zeros"), steps=3, regions_per_step=2.5)
    res = pa.compute_perturbation_analysis(X, CAPS)
    units = [(b, t) for b in range(4) for t in range(1, len(CAPS[b]))]
    assert res["units"] == units and res["logp"].shape == res["logit"].shape == (4, len(units))
    assert res["logp"].dtype == np.float64
    want, _ = _by_hand(ex, X, CAPS, units, [1, 3.5, 6.0], (9, 9))
    err = np.abs(res["logp"] - want)
    assert err[0].max() <= 1e-12, err[0].max()                          # row 0: the unperturbed word log-probability
    assert err[1:].max() <= 1e-12, err[1:].max()
    assert (res["logp"] <= 0).all()
    p = np.exp(res["logp"])
    assert np.allclose(res["scores"], p.mean(axis=1), rtol=0, atol=1e-15) and len(res["scores"]) == 4
    assert np.allclose(res["aopc"], (p[0] - p[1:]).mean(axis=0), rtol=0, atol=1e-15) and res["aopc"].shape == (len(units),)
    assert (res["logp"][1:] != res["logp"][0]).any()                    # the perturbation reaches the word's score
    assert ex.caption is None
    report("perturb_driver", cls=cls, max_abs=float(err.max()))


def test_driver_words_orders_and_the_all_zero_image():
    ex, rs = _explainer("ExplainImgCaptioningAdaptiveAttention", "adaptive", max_images=2, seed=3)
    X = rs.uniform(-120, 130, size=(4, 32, 32, 3)).astype(np.float32)
    caps = [CAPS[0], CAPS[1], CAPS[0], CAPS[1]]
    words = [[1, 2], [1, 2], [1, 2], [1, 2]]
    units = [(b, t) for b in range(4) for t in words[b]]
    # channels='all', zeros, k = nreg = 16 at step 2: every image is all zero, units sharing a caption and t score the same
    pa = PB.CaptionPerturbationAnalysis(ex, PB.Perturbation("zeros", channels="all"), steps=2, regions_per_step=15)
    res = pa.compute_perturbation_analysis(X, caps, words)
    assert res["units"] == units
    lp = res["logp"]
    for j in range(4):
        assert abs(lp[2, j] - lp[2, j + 4]) <= 1e-12 and abs(res["logit"][2, j] - res["logit"][2, j + 4]) <= 1e-12
    assert (lp[0, :4] != lp[0, 4:]).any()                               # (different images before the perturbation)
    # least relevant first: the by-hand path with the negated scores
    pa = PB.CaptionPerturbationAnalysis(ex, PB.Perturbation("invert"), steps=1, order="least_relevant")
    got = pa.compute_perturbation_analysis(X, caps, words)["logp"]
    want, ranks = _by_hand(ex, X, caps, units, [1], (9, 9), mode="invert", negate=True)
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(_by_hand(ex, X, caps, units, [], (9, 9))[1], 15 - ranks)
    eng = ex._engine
    # random order: seeded, needs no explanation, and is another curve
    ra = PB.CaptionPerturbationAnalysis(ex, PB.Perturbation("zeros"), steps=2, regions_per_step=3, order="random", seed=5)
    a, b = ra.compute_perturbation_analysis(X, caps, words), ra.compute_perturbation_analysis(X, caps, words)
    assert np.array_equal(a["logp"], b["logp"])
    rr = PB.random_ranks(len(units), 16, 5)
    M = eng.max_images
    for c0 in range(0, len(units), M):
        chunk = units[c0:c0 + M]
        eng.encode_images(ref.perturbate(X, rr[c0:c0 + M], 4.0, (9, 9), "zeros", img_idx=[u[0] for u in chunk]))
        eng.decoder_forward([caps[u[0]] for u in chunk])
        preds = eng.read_state("caption_preds").cpu().numpy()
        for j, (bb, t) in enumerate(chunk):
            assert abs(a["logp"][2, c0 + j] - _log_softmax(preds[j, t - 1])[caps[bb][t - 1] - 1]) <= 1e-12
    with pytest.raises(NotImplementedError):
        ra.compute_perturbation_analysis(X, caps, [[1], [2], [99], [1]])


def test_driver_resnet_stem_path_625_regions():
    rn = {"stem": 8, "stacks": ((8, 1), (8, 1), (8, 1), (8, 1))}
    ex, rs = _explainer("ExplainImgCaptioningAdaptiveAttention", "adaptive", hw=224, resnet=rn, max_images=2, seed=6)
    X = rs.uniform(-120, 130, size=(2, 224, 224, 3)).astype(np.float32)
    words = [[1, 4], [2]]
    units = [(0, 1), (0, 4), (1, 2)]
    pa = PB.CaptionPerturbationAnalysis(ex, PB.Perturbation("zeros", channels="all"), steps=2, regions_per_step=200)
    res = pa.compute_perturbation_analysis(X, CAPS[:2], words)
    want, ranks = _by_hand(ex, X, CAPS[:2], units, [1, 201], (9, 9), all_channels=True)
    assert ranks.shape == (3, 625)
    err = np.abs(res["logp"] - want)
    assert err.max() <= 1e-12, err.max()
    assert (res["logp"][2] != res["logp"][0]).any()
    report("perturb_driver_resnet", max_abs=float(err.max()))
