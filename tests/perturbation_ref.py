"""Numpy restatement of the perturbation analysis (innvestigate/tools/perturbate.py, cited PT:) with the project's own
rules where the reference has none: float64 scores added in one fixed order, ties to the lower region index, NaN last.
Written from the description of the algorithm, not from the reference's code; the goldens of
tests/golden/make_perturbation_golden.py pin it against the reference itself."""
import os

import numpy as np

FUNCTIONS = ("zeros", "mean", "invert")
RANGES = (None, (-0.5, 0.5))


def geometry(H, W, region):
    """-> (Hr, Wr, before_h, before_w).  PT:170: padding iff the region does not divide both axes; PT:106-111: each axis by
    r - dim % r, floor(pad / 2) before.  One divisible axis alone is the reference's assert (PT:107): ValueError."""
    rh, rw = int(region[0]), int(region[1])
    if rh < 1 or rw < 1:
        raise NotImplementedError("the region shape must be at least 1 x 1")
    dh, dw = H % rh == 0, W % rw == 0
    if dh != dw:
        raise ValueError("the region divides one axis and not the other")
    ph, pw = (0 if dh else rh - H % rh), (0 if dw else rw - W % rw)
    return (H + ph) // rh, (W + pw) // rw, ph // 2, pw // 2


def _mirror(i, n):
    """np.pad(mode='reflect') as an index map."""
    if n == 1:
        return np.zeros_like(i)
    per = 2 * (n - 1)
    i = np.mod(i, per)
    return np.where(i >= n, per - i, i)


def _padded_index(n, r, count, before):
    return _mirror(np.arange(count * r) - before, n)


def _region_of_pixels(H, W, region):
    """(H, W) region index of every pixel of the unpadded map."""
    Hr, Wr, bh, bw = geometry(H, W, region)
    return ((np.arange(H) + bh) // region[0])[:, None] * Wr + ((np.arange(W) + bw) // region[1])[None, :]


def _raster_sum(vp, region, op):
    """vp (n, Hp, Wp) float64 -> (n, Hr, Wr): the pixels of each region combined one at a time in raster order."""
    acc = None
    for dy in range(region[0]):
        for dx in range(region[1]):
            t = vp[:, dy::region[0], dx::region[1]]
            acc = t.copy() if acc is None else op(acc, t)
    return acc


def region_scores(analysis, region, reduce="mean", aggregate="mean", negate=False):
    """analysis (n, H, W, C) float32 / float64 -> (n, nreg) float64, row-major region order."""
    a = np.asarray(analysis).astype(np.float64)
    n, H, W, C = a.shape
    Hr, Wr, bh, bw = geometry(H, W, region)
    ops = {"mean": np.add, "max": np.maximum}
    v = a[..., 0].copy()
    for c in range(1, C):
        v = ops[reduce](v, a[..., c])
    if reduce == "mean":
        v = v / float(C)
    vp = v[:, _padded_index(H, region[0], Hr, bh)][:, :, _padded_index(W, region[1], Wr, bw)]
    s = _raster_sum(vp, region, ops[aggregate])
    if aggregate == "mean":
        s = s / float(region[0] * region[1])
    s = s.reshape(n, Hr * Wr)
    return -s if negate else s


def ranks_from_scores(scores):
    """rank[i] = #{j : s_j > s_i or (s_j == s_i and j < i)}; NaN last (a stable descending sort)."""
    order = np.argsort(-np.asarray(scores, dtype=np.float64), axis=-1, kind="stable")
    return np.argsort(order, axis=-1, kind="stable").astype(np.int32)


def region_ranks(analysis, region, reduce="mean", aggregate="mean", negate=False):
    return ranks_from_scores(region_scores(analysis, region, reduce, aggregate, negate))


def min_relative_gap(scores):
    """Smallest gap between two sorted scores of one map, relative to the map's largest magnitude."""
    s = np.sort(np.asarray(scores, dtype=np.float64), axis=-1)
    return float((np.diff(s, axis=-1).min(axis=-1) / np.abs(s).max(axis=-1)).min())


def perturbate(x, ranks, k, region, mode, img_idx=None, noise=None, all_channels=False, value_range=None):
    """x (B, H, W, C) float32, ranks (n, nreg), k (n,) or a scalar -> (n, H, W, C) float32.  Unit u is image img_idx[u]
    (default u) with the regions of rank <= k - 1 replaced in channel 0 (or every channel).  With a value range a unit with
    k >= 1 is clipped, perturbed and clipped again."""
    x = np.asarray(x, dtype=np.float32)
    ranks = np.asarray(ranks)
    n = len(ranks)
    B, H, W, C = x.shape
    Hr, Wr, bh, bw = geometry(H, W, region)
    k = np.broadcast_to(np.asarray(k, dtype=np.float64), (n,))
    img_idx = np.arange(n) if img_idx is None else np.asarray(img_idx)
    reg = _region_of_pixels(H, W, region)
    iy, ix = _padded_index(H, region[0], Hr, bh), _padded_index(W, region[1], Wr, bw)
    out = np.empty((n, H, W, C), dtype=np.float32)
    for u in range(n):
        if not 0 <= img_idx[u] < B:
            out[u] = np.nan
            continue
        xi = x[img_idx[u]].copy()
        clip = value_range is not None and k[u] >= 1
        if clip:
            lo, hi = np.float32(value_range[0]), np.float32(value_range[1])
            xi = np.clip(xi, lo, hi)
        mask = (ranks[u] <= k[u] - 1)[reg]
        o = xi.copy()
        for c in range(C if all_channels else 1):
            if mode == "zeros":
                new = np.zeros((H, W), dtype=np.float32)
            elif mode == "invert":
                new = -xi[..., c]
            elif mode == "noise":
                new = np.asarray(noise[u][..., c], dtype=np.float32)
            elif mode == "mean":
                xp = xi[..., c][iy][:, ix].astype(np.float64)
                m = (_raster_sum(xp[None], region, np.add)[0] / float(region[0] * region[1])).astype(np.float32)
                new = m.reshape(-1)[reg]
            else:
                raise ValueError(mode)
            o[..., c] = np.where(mask, new, xi[..., c])
        out[u] = np.clip(o, lo, hi) if clip else o
    return out


def mean_bound(x, region, value_range=None):
    """(n, H, W) bound on |reference - restatement| inside a region perturbed with 'mean': the reference adds the rh * rw
    float32 values of the region in float32 and rounds the quotient, (rh * rw + 1) * 2^-24 * mean |x| over the padded region
    (of the clipped image when a value range is set)."""
    x = np.asarray(x, dtype=np.float32)
    if value_range is not None:
        x = np.clip(x, np.float32(value_range[0]), np.float32(value_range[1]))
    n, H, W, C = x.shape
    Hr, Wr, bh, bw = geometry(H, W, region)
    iy, ix = _padded_index(H, region[0], Hr, bh), _padded_index(W, region[1], Wr, bw)
    xp = np.abs(x[..., 0].astype(np.float64))[:, iy][:, :, ix]
    m = _raster_sum(xp, region, np.add) / float(region[0] * region[1])
    reg = _region_of_pixels(H, W, region)
    return (region[0] * region[1] + 1) * 2.0 ** -24 * m.reshape(n, -1)[:, reg]


# ---------------------------------------------------------------------------------------------------- the goldens
GOLDENS = ("perturbation_18x27_r9", "perturbation_20x29_r9", "perturbation_23x23_r4x6", "perturbation_20x29_r9_c1")


def load_golden(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def golden_base(z, ki, ri):
    """What a stored output is a difference against: x, clipped when (value range and k >= 1)."""
    x = z["x"]
    if RANGES[ri] is not None and z["ks"][ki] >= 1:
        return np.clip(x, np.float32(RANGES[ri][0]), np.float32(RANGES[ri][1]))
    return x.copy()


def golden_output(z, fn, ki, ri):
    """The reference's perturbate_on_batch output for (function, k index, range index), decoded from its sparse form."""
    out = golden_base(z, ki, ri)
    key = "%s_k%d_r%d" % (fn, ki, ri)
    out.reshape(-1)[z["idx_" + key]] = z["val_" + key]
    return out


def check_against_golden(z, fn, ki, ri, got):
    """zeros / invert: bit-equal.  mean: bit-equal outside the perturbed regions, within mean_bound inside."""
    want = golden_output(z, fn, ki, ri)
    assert got.dtype == np.float32 and got.shape == want.shape
    same = got.view(np.uint32) == want.view(np.uint32)
    if fn != "mean":
        assert same.all(), (fn, ki, ri, int((~same).sum()))
        return 0.0
    region = tuple(z["region"])
    inside = (z["ranks"] <= z["ks"][ki] - 1)[:, _region_of_pixels(want.shape[1], want.shape[2], region)]
    outside = np.ones(want.shape, dtype=bool)
    outside[..., 0] = ~inside
    assert same[outside].all(), (fn, ki, ri)
    bound = mean_bound(z["x"], region, RANGES[ri] if z["ks"][ki] >= 1 else None)
    err = np.abs(got[..., 0].astype(np.float64) - want[..., 0].astype(np.float64))
    assert (err[inside] <= bound[inside]).all(), (fn, ki, ri, float((err - bound)[inside].max()))
    return float(err[inside].max()) if inside.any() else 0.0
