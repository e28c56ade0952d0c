"""-m gpu: occlusion and RISE word saliency on the device (lrp_op_occlude / _occlusion_map / _rise_*, saliency.py, the four
explainer classes) against the numpy restatement (tests/saliency_ref.py) and the by-hand path through the same engine."""
import numpy as np
import pytest
import torch

import perturbation_ref as pref
import saliency_ref as ref
from gpu_util import report
from lrp_imagecaptioning_amd import engine as E
from lrp_imagecaptioning_amd import perturbation as PB
from lrp_imagecaptioning_amd import saliency as SAL
from test_gpu_eval_bbox import CAPS, CFG, WORDS, _explainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL3 = [-3.5, 10.25, 0.0]


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------- occlude
# (H, W, C), window, stride: one axis fits and the other clips (per image 1740 values: float4 path); window == stride; one
# window; 189 values per image (not a multiple of four: the scalar path with a tail group)
OCC_CASES = [((20, 29, 3), (5, 7), (3, 4)), ((16, 16, 1), (4, 4), None), ((16, 16, 3), (16, 16), None), ((7, 9, 3), (3, 2), (2, 1))]


def _occ_rows(rs, B, nwin):
    idx = [b for b in range(B) for _ in range(nwin + 1)] + [-1, B, 0, 1]
    ks = [k for _ in range(B) for k in range(-1, nwin)] + [0, 0, -2, nwin]
    order = rs.permutation(len(idx))
    return np.asarray(idx)[order], np.asarray(ks)[order], len(idx) - 4


@pytest.mark.parametrize("shape,window,stride", OCC_CASES)
def test_occlude_equals_the_restatement_bit_for_bit(shape, window, stride):
    rs = np.random.RandomState(sum(shape))
    H, W, C = shape
    B = 2
    x = rs.uniform(-120, 130, size=(B, H, W, C)).astype(np.float32)
    fill = FILL3[:C]
    Hn, Wn = ref.geometry(H, W, window, stride)
    idx, ks, good = _occ_rows(rs, B, Hn * Wn)
    got = E.op_occlude(_t(x), idx, ks, window, stride, fill).cpu().numpy()
    want = ref.occlude(x, idx, ks, window, stride, fill)
    nan = np.isnan(want).all(axis=(1, 2, 3))
    assert nan.sum() == 4 and np.isnan(got[nan]).all() and not np.isnan(got[~nan]).any()
    assert _same_bits(got[~nan], want[~nan])
    for r in np.nonzero(ks == -1)[0]:
        assert _same_bits(got[r], x[idx[r]])
    # any cut of the rows into calls, and any slot, gives the same bits
    n = len(idx)
    cut = min(13, n - 1)
    parts = np.concatenate([E.op_occlude(_t(x), idx[:cut], ks[:cut], window, stride, fill).cpu().numpy(),
                            E.op_occlude(_t(x), idx[cut:], ks[cut:], window, stride, fill).cpu().numpy()])
    assert _same_bits(parts[~nan], got[~nan])
    back = E.op_occlude(_t(x), idx[::-1].copy(), ks[::-1].copy(), window, stride, fill).cpu().numpy()[::-1]
    assert _same_bits(back[~nan], got[~nan])


# ---------------------------------------------------------------------------------------------------- RISE grids and apply
# (H, W, C), s, cell.  The first two hold 1740 and 256 values per image (multiples of four: the float4 path); the last two 189 and
# 63: the scalar path, rows that start at any alignment, a short last group, pixels that straddle a group (C = 3) and not (C = 1)
RISE_CASES = [((20, 29, 3), 3, (7, 10)), ((16, 16, 1), 8, (2, 2)), ((7, 9, 3), 3, (3, 3)), ((7, 9, 1), 3, (3, 3))]


def _rise_rows(rs, n=37):
    keys = rs.randint(0, 2 ** 32, size=n, dtype=np.int64)
    keys[:3] = [0, 2 ** 32 - 1, 2 ** 31]
    return keys, rs.randint(0, 5000, size=n).astype(np.int64)


@pytest.mark.parametrize("p", [0.25, 0.5])
@pytest.mark.parametrize("shape,s,cell", RISE_CASES)
def test_rise_grids_and_apply_match_the_restatement(shape, s, cell, p):
    H, W, C = shape
    assert ref.rise_cell(H, W, s) == cell
    rs = np.random.RandomState(H + s)
    B, n, seed = 3, 37, (7 << 32) + 12345
    x = rs.uniform(-120, 130, size=(B, H, W, C)).astype(np.float32)
    fill = FILL3[:C]
    keys, ks = _rise_rows(rs, n)
    idx = rs.randint(0, B, size=n)
    grid, shift = E.op_rise_grids(keys, ks, s, p, seed, H, W, device=torch.device(DEV))
    g_ref, s_ref = ref.rise_grids(keys, ks, s, p, seed, cell)
    assert grid.dtype == torch.uint8 and shift.dtype == torch.int32
    assert np.array_equal(grid.cpu().numpy(), g_ref) and np.array_equal(shift.cpu().numpy(), s_ref)
    got = E.op_rise_apply(_t(x), idx, grid, shift, s, fill).cpu().numpy()
    want = ref.rise_apply(x, idx, g_ref, s_ref, s, cell, fill)
    # the mask takes at most six float32 roundings, the blend two more
    bound = 8 * 2.0 ** -24 * (np.abs(x[idx].astype(np.float64)) + np.abs(np.asarray(fill, dtype=np.float64)))
    err = np.abs(got.astype(np.float64) - want)
    print("rise_apply", shape, s, p, "max err / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    # [0, 13) + [13, 37) equal one call
    ga, sa = E.op_rise_grids(keys[:13], ks[:13], s, p, seed, H, W, device=torch.device(DEV))
    gb, sb = E.op_rise_grids(keys[13:], ks[13:], s, p, seed, H, W, device=torch.device(DEV))
    assert torch.equal(torch.cat([ga, gb]), grid) and torch.equal(torch.cat([sa, sb]), shift)
    parts = torch.cat([E.op_rise_apply(_t(x), idx[:13], ga, sa, s, fill), E.op_rise_apply(_t(x), idx[13:], gb, sb, s, fill)])
    assert _same_bits(parts.cpu().numpy(), got)
    # the same (key, k) in another slot gives the same bits
    perm = rs.permutation(n)
    gp, sp = E.op_rise_grids(keys[perm], ks[perm], s, p, seed, H, W, device=torch.device(DEV))
    assert torch.equal(gp, grid[_t(perm)]) and torch.equal(sp, shift[_t(perm)])
    assert _same_bits(E.op_rise_apply(_t(x), idx[perm], gp, sp, s, fill).cpu().numpy(), got[perm])
    # rows that read nothing: an image index outside the batch, a shift outside the cell
    bad_shift = shift[:3].clone()
    bad_shift[1, 0] = cell[0]
    bad_shift[2, 1] = -1
    bad = E.op_rise_apply(_t(x), [B, 0, 1], grid[:3], bad_shift, s, fill).cpu().numpy()
    assert np.isnan(bad).all()
    report("rise_apply", shape=list(shape), s=s, p=p, worst_over_bound=float((err / np.maximum(bound, 1e-300)).max()))


def test_rise_p_one_is_the_identity_mask():
    rs = np.random.RandomState(4)
    x = rs.uniform(-120, 130, size=(2, 20, 29, 3)).astype(np.float32)
    grid, shift = E.op_rise_grids([1, 2, 3], [0, 1, 2], 3, 1.0, 5, 20, 29, device=torch.device(DEV))
    assert bool(grid.all())
    got = E.op_rise_apply(_t(x), [0, 1, 0], grid, shift, 3, 0.0).cpu().numpy()      # fill 0, m = 1: 0 + 1 (x - 0) = x exactly
    assert _same_bits(got, x[[0, 1, 0]])


# ---------------------------------------------------------------------------------------------------- the map operators
def _check_map(got, S, A, what):
    err = np.abs(got.astype(np.float64) - S)
    bar = ref.map_bar(S, A)
    worst = float((err / np.maximum(bar, 1e-300)).max())
    print(what, "max err / bar", worst)
    assert (err <= bar).all(), (what, worst)
    return worst


def _check_prob_maps(got, p0, S, A, what):
    """The default score='prob' maps of the driver, on the words whose probability a float32 map can hold: p0 >= 2^-100 leaves 26
    binary orders above float32's smallest normal number 2^-126 for the differences.  An element below 2^-126 is a float32
    subnormal, whose spacing 2^-149 is then the rounding the format allows on top of the map bar.  -> words checked"""
    words = np.nonzero(p0 >= 2.0 ** -100)[0]
    for w in words:
        err = np.abs(got[w].astype(np.float64) - S[w])
        assert (err <= ref.map_bar(S[w], A[w]) + 2.0 ** -149).all(), (what, int(w), float(p0[w]))
        assert got[w].any()
    return len(words)


@pytest.mark.parametrize("shape,window,stride", OCC_CASES + [((32, 32, 3), (12, 12), (8, 8))])
def test_occlusion_map_matches_the_restatement(shape, window, stride):
    H, W, _ = shape
    rs = np.random.RandomState(H * W)
    Hn, Wn = ref.geometry(H, W, window, stride)
    scores = rs.randn(2, 1 + Hn * Wn, 3) * rs.choice([1e-3, 1.0, 40.0], size=(2, 1, 3))
    got = E.op_occlusion_map(_t(scores), H, W, window, stride)
    assert got.shape == (2, 3, H, W) and got.dtype == torch.float32
    S, A = ref.occlusion_map(scores, H, W, window, stride)
    worst = _check_map(got.cpu().numpy(), S, A, "occlusion_map %s" % (shape,))
    for i in range(2):                                                  # an image alone equals its place among two
        assert torch.equal(E.op_occlusion_map(_t(scores[i:i + 1]), H, W, window, stride)[0], got[i])
    report("occlusion_map", shape=list(shape), worst_over_bar=worst)


def test_occlusion_map_known_answers():
    H, W, win, st = 20, 29, (5, 7), (3, 4)
    Hn, Wn = ref.geometry(H, W, win, st)
    c = ref.coverage(H, W, win, st)
    for k in (0, 9, Hn * Wn - 1):
        s = np.full((1, 1 + Hn * Wn, 2), 0.75)
        s[0, 1 + k, 1] -= 1.0
        got = E.op_occlusion_map(_t(s), H, W, win, st).cpu().numpy()
        y0, y1, x0, x1 = ref.window_box(k, H, W, win, st)
        ind = np.zeros((H, W))
        ind[y0:y1, x0:x1] = 1.0
        assert _same_bits(got[0, 1], (ind / c).astype(np.float32)) and not got[0, 0].any()
    # window == stride: c = 1, the map is the window's own difference
    rs = np.random.RandomState(1)
    s = rs.rand(1, 17, 2)
    got = E.op_occlusion_map(_t(s), 16, 16, 4).cpu().numpy()
    for k in range(16):
        y0, y1, x0, x1 = ref.window_box(k, 16, 16, 4)
        assert (_bits(got[0, :, y0:y1, x0:x1]) == _bits((s[0, 0] - s[0, 1 + k]).astype(np.float32))[:, None, None]).all()
    # one window covering the image
    got = E.op_occlusion_map(_t(np.array([[[0.9, 0.5], [0.25, 0.75]]])), 16, 16, 16).cpu().numpy()
    assert (got[0, 0] == np.float32(0.9 - 0.25)).all() and (got[0, 1] == np.float32(0.5 - 0.75)).all()


@pytest.mark.parametrize("p", [0.25, 0.5])
@pytest.mark.parametrize("shape,s,cell", RISE_CASES)
def test_rise_map_matches_the_restatement(shape, s, cell, p):
    H, W, _ = shape
    rs = np.random.RandomState(W + s)
    n_img, K, T = 2, 37, 3
    keys = np.repeat([11, 2 ** 32 - 5], K)
    ks = np.tile(np.arange(K), n_img)
    grid, shift = E.op_rise_grids(keys, ks, s, p, 99, H, W, device=torch.device(DEV))
    grid, shift = grid.view(n_img, K, -1), shift.view(n_img, K, 2)
    scores = rs.randn(n_img, K, T) * rs.choice([1e-3, 1.0, 40.0], size=(n_img, 1, T))
    got = E.op_rise_map(_t(scores), grid, shift, H, W, s, p)
    assert got.shape == (n_img, T, H, W) and got.dtype == torch.float32
    S, A = ref.rise_map(scores, grid.cpu().numpy(), shift.cpu().numpy(), H, W, s, p, cell)
    worst = _check_map(got.cpu().numpy(), S, A, "rise_map %s p=%g" % (shape, p))
    for i in range(n_img):
        assert torch.equal(E.op_rise_map(_t(scores[i:i + 1]), grid[i:i + 1], shift[i:i + 1], H, W, s, p)[0], got[i])
    # a constant score v gives v sum m / (K p)
    v = 0.375
    m = ref.rise_masks(grid[0].cpu().numpy(), shift[0].cpu().numpy(), H, W, s, cell)
    got_v = E.op_rise_map(_t(np.full((1, K, 9), v)), grid[:1], shift[:1], H, W, s, p).cpu().numpy()    # T = 9: two word tiles
    want = v * m.sum(axis=0) / (K * p)
    assert (np.abs(got_v[0] - want[None]) <= ref.map_bar(want, want)[None]).all()
    report("rise_map", shape=list(shape), s=s, p=p, worst_over_bar=worst)


def test_rise_map_with_p_one_returns_the_constant_score():
    grid, shift = E.op_rise_grids([4] * 6, range(6), 3, 1.0, 1, 20, 29, device=torch.device(DEV))
    got = E.op_rise_map(_t(np.full((1, 6, 2), 0.375)), grid.view(1, 6, -1), shift.view(1, 6, 2), 20, 29, 3, 1.0)
    assert bool((got == 0.375).all())                                   # m = 1: 6 x 0.375 / 6, exact


# ---------------------------------------------------------------------------------------------------- the driver
KINDS = [("adaptive", "ExplainImgCaptioningAdaptiveAttention"), ("gridtd", "ExplainImgCaptioningGridTDModel")]


def _log_softmax(row):
    m = row.max()
    return row - (m + np.log(np.exp(row - m).sum()))


def _scores_by_hand(ex, rows_of_job, caps_of_job, words_of_job):
    """log-probability of every word of every job: the rows through encode_images, decoder_forward and numpy, in chunks of max_images"""
    eng = ex._engine
    M = eng.max_images
    out = []
    for c0 in range(0, len(caps_of_job), M):
        eng.encode_images(rows_of_job(c0, min(len(caps_of_job), c0 + M)))
        eng.decoder_forward(caps_of_job[c0:c0 + M])
        preds = eng.read_state("caption_preds").cpu().numpy()
        for j, (cap, ts) in enumerate(zip(caps_of_job[c0:c0 + M], words_of_job[c0:c0 + M])):
            out.append(np.array([_log_softmax(preds[j, t - 1])[cap[t - 1] - 1] for t in ts]))
    return out


@pytest.mark.parametrize("window,stride", [((8, 8), None), ((12, 12), (8, 8))])
@pytest.mark.parametrize("kind,cls", KINDS)
def test_occlusion_driver_matches_the_by_hand_path(kind, cls, window, stride):
    ex, rs = _explainer(cls, kind, max_images=2)
    B = 3
    X = rs.uniform(-120, 130, size=(B, 32, 32, 3)).astype(np.float32)
    caps = CAPS[:B]
    # every map is checked on score='logp': the tiny random captioner gives some words probabilities near 1e-90, which a float32
    # map cannot hold (the map bar has no term for underflow).  The float64 'prob' scores are checked all the same, and the 'prob'
    # maps of the words a float32 map can hold (_check_prob_maps)
    res = SAL.OcclusionSaliency(ex, window, stride, fill=FILL3, score="logp").explain(X, caps)
    assert ex.caption is None
    prob = SAL.OcclusionSaliency(ex, window, stride, fill=FILL3).explain(X, caps)
    units = [(b, t) for b in range(B) for t in range(1, len(caps[b]))]
    assert res["units"] == units
    assert res["maps"].shape == (len(units), 32, 32) and res["maps"].dtype == torch.float32 and res["maps"].is_cuda
    Hn, Wn = ref.geometry(32, 32, window, stride)
    R = 1 + Hn * Wn
    jobs = [(b, k) for b in range(B) for k in range(-1, Hn * Wn)]
    rows = lambda c0, c1: ref.occlude(X, [b for b, _ in jobs[c0:c1]], [k for _, k in jobs[c0:c1]], window, stride, FILL3)
    hand = _scores_by_hand(ex, rows, [caps[b] for b, _ in jobs], [list(range(1, len(caps[b]))) for b, _ in jobs])
    got_maps, prob_maps = res["maps"].cpu().numpy(), prob["maps"].cpu().numpy()
    u0, worst_s, worst_m, n_prob = 0, 0.0, 0.0, 0
    for b in range(B):
        T = len(caps[b]) - 1
        sc = res["scores"][b].cpu().numpy()
        assert sc.shape == (R, T)
        ps = prob["scores"][b].cpu().numpy()
        Sp, Ap = ref.occlusion_map(ps[None], 32, 32, window, stride)
        n_prob += _check_prob_maps(prob_maps[u0:u0 + T], ps[0], Sp[0], Ap[0], "driver occlusion prob image %d" % b)
        worst_s = max(worst_s, np.abs(sc - np.stack(hand[b * R:(b + 1) * R])).max())
        worst_s = max(worst_s, np.abs(prob["scores"][b].cpu().numpy() - np.exp(np.stack(hand[b * R:(b + 1) * R]))).max())
        # the map against the restatement on the device's own scores (the by-hand scores are within 1e-12 of them, which a map
        # whose terms nearly cancel would not forgive; the scores are compared above)
        S, A = ref.occlusion_map(sc[None], 32, 32, window, stride)
        worst_m = max(worst_m, _check_map(got_maps[u0:u0 + T], S[0], A[0], "driver occlusion image %d" % b))
        assert np.array_equal(res["scores0"][u0:u0 + T].cpu().numpy(), sc[0])
        u0 += T
    assert worst_s <= 1e-12, worst_s
    assert np.abs(got_maps).max() > 0 and n_prob >= 1
    report("occlusion_driver", kind=kind, window=list(window), score_max_abs=float(worst_s), map_over_bar=worst_m)


@pytest.mark.parametrize("kind,cls", KINDS)
def test_rise_driver_matches_the_by_hand_path(kind, cls):
    ex, rs = _explainer(cls, kind, max_images=2)
    B, K, s, p, seed = 3, 24, 4, 0.5, 77
    X = rs.uniform(-120, 130, size=(B, 32, 32, 3)).astype(np.float32)
    caps = CAPS[:B]
    keys = [5, 2 ** 31 + 3, 9]
    res = SAL.RISESaliency(ex, K, s=s, p=p, seed=seed, fill=FILL3, keys=keys, score="logp").explain(X, caps)     # (logp: see above)
    assert ex.caption is None
    prob = SAL.RISESaliency(ex, K, s=s, p=p, seed=seed, fill=FILL3, keys=keys).explain(X, caps)
    units = [(b, t) for b in range(B) for t in range(1, len(caps[b]))]
    assert res["units"] == units and res["maps"].shape == (len(units), 32, 32)
    # the device-made masked rows (checked against the restatement above) through the same calls
    grid, shift = E.op_rise_grids(np.repeat(keys, K), np.tile(np.arange(K), B), s, p, seed, 32, 32, device=torch.device(DEV))
    jobs = [(b, k) for b in range(B) for k in range(-1, K)]
    xd = _t(X)

    def rows(c0, c1):
        out = []
        for b, k in jobs[c0:c1]:
            out.append(xd[b:b + 1] if k < 0 else E.op_rise_apply(xd, [b], grid[b * K + k:b * K + k + 1],
                                                                 shift[b * K + k:b * K + k + 1], s, FILL3))
        return torch.cat(out)
    hand = _scores_by_hand(ex, rows, [caps[b] for b, _ in jobs], [list(range(1, len(caps[b]))) for b, _ in jobs])
    g, sh = grid.view(B, K, -1).cpu().numpy(), shift.view(B, K, 2).cpu().numpy()
    got_maps, prob_maps = res["maps"].cpu().numpy(), prob["maps"].cpu().numpy()
    u0, worst_s, worst_m, n_prob = 0, 0.0, 0.0, 0
    for b in range(B):
        T = len(caps[b]) - 1
        sc = res["scores"][b].cpu().numpy()
        assert sc.shape == (1 + K, T)
        ps = prob["scores"][b].cpu().numpy()
        Sp, Ap = ref.rise_map(ps[None, 1:], g[b:b + 1], sh[b:b + 1], 32, 32, s, p, (8, 8))
        n_prob += _check_prob_maps(prob_maps[u0:u0 + T], ps[0], Sp[0], Ap[0], "driver RISE prob image %d" % b)
        worst_s = max(worst_s, np.abs(sc - np.stack(hand[b * (K + 1):(b + 1) * (K + 1)])).max())
        worst_s = max(worst_s, np.abs(prob["scores"][b].cpu().numpy() - np.exp(np.stack(hand[b * (K + 1):(b + 1) * (K + 1)]))).max())
        S, A = ref.rise_map(sc[None, 1:], g[b:b + 1], sh[b:b + 1], 32, 32, s, p, (8, 8))
        worst_m = max(worst_m, _check_map(got_maps[u0:u0 + T], S[0], A[0], "driver RISE image %d" % b))
        u0 += T
    assert worst_s <= 1e-12, worst_s
    assert n_prob >= 1
    report("rise_driver", kind=kind, score_max_abs=float(worst_s), map_over_bar=worst_m)


def test_driver_zero_image_words_and_chunking():
    ex2, rs = _explainer("ExplainImgCaptioningAdaptiveAttention", "adaptive", max_images=2, seed=3)
    ex5, _ = _explainer("ExplainImgCaptioningAdaptiveAttention", "adaptive", max_images=5, seed=3)
    X = rs.uniform(-120, 130, size=(3, 32, 32, 3)).astype(np.float32)
    X[1] = 0
    caps = [CAPS[0], CAPS[1], CAPS[3]]
    words = [[2, 1], [1, 3, 5], []]                                     # an image without a word, words out of order
    for make in (lambda ex: SAL.OcclusionSaliency(ex, (12, 12), (8, 8), score="logp"),
                 lambda ex: SAL.RISESaliency(ex, 12, s=4, seed=1, score="logp")):
        a, b = make(ex2).explain(X, caps, words), make(ex5).explain(X, caps, words)
        assert a["units"] == [(0, 2), (0, 1), (1, 1), (1, 3), (1, 5)] == b["units"]
        assert torch.equal(a["maps"], b["maps"]) and torch.equal(a["scores0"], b["scores0"])       # max_images 2 and 5
        assert bool(torch.isfinite(a["maps"]).all()) and bool((a["maps"][:2] != 0).any())
    occ = SAL.OcclusionSaliency(ex2, (12, 12), (8, 8)).explain(X, caps, words)
    # all-zero image, fill 0: every occluded copy is the image, every difference exactly 0 (on 'logp' too, where no score is
    # small enough to vanish in a float32 map whatever the kernel does)
    assert not bool(occ["maps"][2:].any())
    occ_lp = SAL.OcclusionSaliency(ex2, (12, 12), (8, 8), score="logp").explain(X, caps, words)
    assert not bool(occ_lp["maps"][2:].any()) and bool(occ_lp["maps"][:2].any())
    one = SAL.OcclusionSaliency(ex2, (12, 12), (8, 8)).explain(X[:1], caps[:1], [[1]])
    assert torch.equal(one["maps"][0], occ["maps"][1])                  # a word alone is the word among others
    for score in ("logp", "logit"):
        r = SAL.OcclusionSaliency(ex2, (16, 16), score=score).explain(X[:1], caps[:1], [[1, 2]])
        assert bool(torch.isfinite(r["maps"]).all()) and bool(torch.isfinite(r["scores0"]).all())
        assert score == "logit" or bool((r["scores0"] <= 0).all())
    with pytest.raises(NotImplementedError):
        SAL.OcclusionSaliency(ex2, (16, 16)).explain(X, caps, [[1], [99], []])
    with pytest.raises(ValueError):
        SAL.OcclusionSaliency(ex2, (16, 16)).explain(X, caps[:2])
    with pytest.raises(ValueError):
        SAL.OcclusionSaliency(ex2, (33, 4))                             # window beyond the model's image
    beam = SAL.OcclusionSaliency(ex2, (16, 16)).explain(X[:2])          # captions=None: beam search
    assert beam["maps"].shape[0] == len(beam["units"]) >= 1


# ---------------------------------------------------------------------------------------------------- the classes
def _saliency_explainer(cls_name, kind, max_images=2, seed=0, resnet=None, hw=32, **kw):
    """test_gpu_eval_bbox._explainer with the class's own keywords"""
    import lrp_imagecaptioning_amd.explainers as EX
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, gridtd_weights, resnet_weights, vgg_weights
    rs = np.random.RandomState(seed)
    V, H = 40, 32
    if resnet is None:
        w = vgg_weights(rs, CFG, bias_std=0.3)
        L, D = (hw // 4) ** 2, CFG[-1][2]
    else:
        w = resnet_weights(rs, resnet["stacks"], stem=resnet["stem"], bias_std=0.2)
        L, D = (hw // 32) ** 2, resnet["stacks"][-1][0] * 4
    w.update((adaptive_weights if kind == "adaptive" else gridtd_weights)(rs, L, D, H, H, V))
    spec = EX.CaptionModelSpec(w, img_encoder="vgg16" if resnet is None else "resnet101", hidden_dim=H, embedding_dim=H, L=L, D=D,
                               vocab_size=V, cnn_cfg=CFG, img_hw=(hw, hw), resnet=resnet)
    dp = EX.DatasetProviderStub(EX.CaptionPreprocessorStub(word_of={i: WORDS[i % len(WORDS)] for i in range(2, V + 1)}))
    return getattr(EX, cls_name)(spec, None, dp, max_caption_length=8, max_images=max_images, **kw), rs


@pytest.mark.parametrize("cls,kind,kw", [
    ("ExplainImgCaptioningAdaptiveAttentionOcclusion", "adaptive", {"window": (12, 12), "stride": 8, "score": "logp"}),
    ("ExplainImgCaptioningGridTDOcclusion", "gridtd", {"window": 16, "score": "logit"}),
    ("ExplainImgCaptioningAdaptiveAttentionRISE", "adaptive", {"n_masks": 8, "s": 4, "score": "logp"}),
    ("ExplainImgCaptioningGridTDRISE", "gridtd", {"n_masks": 8, "s": 4, "p": 0.25, "seed": 3, "score": "logit"})])
def test_classes_return_maps_that_move_with_the_image(cls, kind, kw):
    ex, rs = _saliency_explainer(cls, kind, **kw)
    X = rs.uniform(-120, 130, size=(2, 32, 32, 3)).astype(np.float32)
    res = ex.explain_images(X[:1], [CAPS[1]])
    n_words = len(CAPS[1]) - 1
    assert res["maps"].shape == (n_words, 32, 32) and bool(torch.isfinite(res["maps"]).all()) and bool(res["maps"].any())
    other = ex.explain_images(X[1:], [CAPS[1]])
    assert not torch.equal(other["maps"], res["maps"])
    assert torch.equal(ex.explain_images(X[:1], [CAPS[1]])["maps"], res["maps"])
    with pytest.raises(NotImplementedError):
        ex._explain_sentence()


def test_occlusion_class_runs_on_a_resnet_spec():
    rn = {"stem": 8, "stacks": ((8, 1), (8, 1), (8, 1), (8, 1))}
    ex, rs = _saliency_explainer("ExplainImgCaptioningAdaptiveAttentionOcclusion", "adaptive", resnet=rn, hw=224, window=112, score="logp")
    X = rs.uniform(-120, 130, size=(1, 224, 224, 3)).astype(np.float32)
    res = ex.explain_images(X, [CAPS[2]])
    assert res["maps"].shape == (3, 224, 224) and bool(torch.isfinite(res["maps"]).all()) and bool(res["maps"].any())


def test_perturbation_analysis_ranks_by_the_occlusion_maps_and_leaves_lrp_alone():
    lrp, rs = _explainer("ExplainImgCaptioningAdaptiveAttention", "adaptive", max_images=2)
    X = rs.uniform(-120, 130, size=(3, 32, 32, 3)).astype(np.float32)
    caps = CAPS[:3]
    pa_lrp = PB.CaptionPerturbationAnalysis(lrp, PB.Perturbation("zeros"), steps=2, regions_per_step=3)
    before = pa_lrp.compute_perturbation_analysis(X, caps)

    ex, _ = _saliency_explainer("ExplainImgCaptioningAdaptiveAttentionOcclusion", "adaptive", window=(12, 12), stride=(8, 8), score="logp")
    pa = PB.CaptionPerturbationAnalysis(ex, PB.Perturbation("zeros", channels="all"), steps=2, regions_per_step=3)
    res = pa.compute_perturbation_analysis(X, caps)
    units = [(b, t) for b in range(3) for t in range(1, len(caps[b]))]
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

    after = pa_lrp.compute_perturbation_analysis(X, caps)              # the new branch leaves the others alone
    assert _same_bits(after["logp"], before["logp"]) and _same_bits(after["logit"], before["logit"])
    report("perturbation_with_occlusion", max_abs=float(err))
