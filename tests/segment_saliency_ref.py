"""numpy float64 restatement of the LIME / KernelSHAP operators (include/lrp_hip.h, csrc/segment_kernels.h): the draws on
gradient_family_ref.philox4x32_10, the segment mask apply, the weighted regression as numpy.linalg.lstsq on the augmented problem
(rows scaled by sqrt(w), sqrt(ridge) rows appended; the Shapley form by the same elimination; deliberately not the normal
equations the device solves), the map gather, and Shapley values by the subset formula."""
from fractions import Fraction
from itertools import combinations
from math import comb, factorial

import numpy as np

from gradient_family_ref import philox4x32_10

BERNOULLI, SHAPLEY = 0, 1
WORDS = 4


# ---------------------------------------------------------------------------------------------------- draws
def size_cumulative(d):
    """exact C(1) .. C(d - 2): the cumulative of p(m) ~ (d - 1) / (m (d - m)), m = 1 .. d - 1, as Fractions"""
    pm = [Fraction(d - 1, m * (d - m)) for m in range(1, d)]
    tot = sum(pm)
    out, c = [], Fraction(0)
    for m in range(d - 2):
        c += pm[m] / tot
        out.append(c)
    return out


def _philox(c0, c1, c2, c3, seed):
    ctr = np.array([c0, c1, c2, c3], dtype=np.uint64)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    return [int(v) for v in philox4x32_10(ctr, key)]


def pack(subset, d):
    z = [0] * WORDS
    for j in subset:
        assert 0 <= j < d
        z[j // 32] |= 1 << (j % 32)
    return z


def unpack(bits, d):
    """bits (..., 4) uint32 -> (..., d) 0 / 1 int64"""
    bits = np.asarray(bits).astype(np.uint32)
    j = np.arange(d)
    return ((bits[..., j // 32] >> (j % 32).astype(np.uint32)) & np.uint32(1)).astype(np.int64)


def draws(keys, ks, d, mode, p=0.5, thr=None, seed=0):
    """-> (n, 4) uint32.  Bernoulli: segment j takes lane j % 4 of counter (j / 4, k, key, 2), on iff (x >> 8) < floor(p 2^24).
    Shapley: q = k >> 1, u = lane 0 of (0xFFFFFFFF, q, key, 3), s = 1 + #{u >= thr[i]}, partial Fisher-Yates with
    j = i + mulhi32(lane i % 4 of (i / 4, q, key, 3), d - i); an odd k is the complement of k - 1."""
    out = np.zeros((len(ks), WORDS), dtype=np.uint32)
    for r, (key, k) in enumerate(zip(keys, ks)):
        key, k = int(key) & 0xFFFFFFFF, int(k) & 0xFFFFFFFF
        if mode == BERNOULLI:
            thresh = int(np.floor(float(p) * 2.0 ** 24))
            x = [philox for g in range((d + 3) // 4) for philox in _philox(g, k, key, 2, seed)]
            sub = [j for j in range(d) if (x[j] >> 8) < thresh]
        else:
            q = k >> 1
            u = _philox(0xFFFFFFFF, q, key, 3, seed)[0]
            s = 1 + sum(1 for i in range(d - 2) if u >= int(thr[i]))
            perm = list(range(d))
            for i in range(s):
                if i % 4 == 0:
                    x = _philox(i // 4, q, key, 3, seed)
                j = i + ((x[i % 4] * (d - i)) >> 32)
                perm[i], perm[j] = perm[j], perm[i]
            sub = perm[:s]
            if k & 1:
                sub = sorted(set(range(d)) - set(sub))
        out[r] = pack(sub, d)
    return out


# ---------------------------------------------------------------------------------------------------- apply and map
def apply(x, img_idx, bits, label, fill, d):
    """x (B, H, W, C) float32 -> (n, H, W, C) float32: x where the pixel's segment is on, fill[c] where it is off; NaN for an
    image index outside [0, B) (the row) or a label outside [0, d) (the pixel)"""
    B, H, W, C = x.shape
    fill = np.broadcast_to(np.asarray(fill, dtype=np.float32).reshape(-1), (C,))
    out = np.full((len(img_idx), H, W, C), np.nan, dtype=np.float32)
    for r, b in enumerate(img_idx):
        if not 0 <= b < B:
            continue
        z = unpack(bits[r], d)
        lab = np.asarray(label[b])
        ok = (lab >= 0) & (lab < d)
        on = np.zeros((H, W), dtype=bool)
        on[ok] = z[lab[ok]] == 1
        row = np.where(on[..., None], x[b], fill[None, None, :]).astype(np.float32)
        row[~ok] = np.nan
        out[r] = row
    return out


def segment_map(phi, label, d):
    """phi (n_img, T, d) float64, label (n_img, H, W) -> (n_img, T, H, W) float32, NaN for a label outside [0, d)"""
    n_img, T, _ = phi.shape
    lab = np.asarray(label)
    ok = (lab >= 0) & (lab < d)
    out = np.full((n_img, T) + lab.shape[1:], np.nan, dtype=np.float32)
    for i in range(n_img):
        out[i][:, ok[i]] = phi[i][:, lab[i][ok[i]]].astype(np.float32)
    return out


# ---------------------------------------------------------------------------------------------------- the fit
def design(bits, wtab, d, shapley):
    """one image: bits (K, 4) -> (U (K, n) float64, w (K,), zl (K,)): the design matrix with the intercept as column 0 (LIME
    form, n = d + 1) or the eliminated columns z_j - z_{d-1} (Shapley form, n = d - 1), the row weights, the last segment"""
    z = unpack(bits, d).astype(np.float64)
    w = np.asarray(wtab, dtype=np.float64)[z.sum(axis=1).astype(np.int64)]
    if shapley:
        return z[:, :d - 1] - z[:, d - 1:], w, z[:, d - 1]
    return np.concatenate([np.ones((len(z), 1)), z], axis=1), w, z[:, d - 1]


def penalty(d, ridge, shapley):
    """the diagonal the ridge adds to the normal equations: not on the intercept"""
    return ridge * (np.ones(d - 1) if shapley else np.concatenate([[0.0], np.ones(d)]))


def system(bits, wtab, d, ridge, shapley):
    """the matrix of the normal equations, the intercept kept as a bordered column"""
    U, w, _ = design(bits, wtab, d, shapley)
    return U.T @ (w[:, None] * U) + np.diag(penalty(d, ridge, shapley))


def _targets(y, zl, delta, shapley):
    return y - zl[:, None] * delta[None, :] if shapley else y


def _finish(x, d, delta, shapley):
    """x (n, T) -> phi (T, d), icpt (T,)"""
    if shapley:
        return np.concatenate([x, (delta - x.sum(axis=0))[None, :]], axis=0).T.copy(), np.zeros(x.shape[1])
    return x[1:].T.copy(), x[0].copy()


def fit(bits, wtab, y, d, ridge=0.0, delta=None):
    """one image: bits (K, 4), y (K, T), delta (T,) or None -> phi (T, d), icpt (T,): lstsq on [sqrt(w) U; sqrt(penalty) I]"""
    shapley = delta is not None
    U, w, zl = design(bits, wtab, d, shapley)
    keep = w != 0
    sw = np.sqrt(w[keep])
    A = np.concatenate([sw[:, None] * U[keep], np.diag(np.sqrt(penalty(d, ridge, shapley)))], axis=0)
    b = np.concatenate([sw[:, None] * _targets(y, zl, delta, shapley)[keep], np.zeros((U.shape[1], y.shape[1]))], axis=0)
    x = np.linalg.lstsq(A, b, rcond=None)[0]
    return _finish(x, d, delta, shapley)


def fit_cholesky(bits, wtab, y, d, ridge=0.0, delta=None):
    """the same problem by numpy.linalg.cholesky on the normal equations (what the device does, in numpy's order of sums)"""
    shapley = delta is not None
    U, w, zl = design(bits, wtab, d, shapley)
    G = U.T @ (w[:, None] * U) + np.diag(penalty(d, ridge, shapley))
    r = U.T @ (w[:, None] * _targets(y, zl, delta, shapley))
    L = np.linalg.cholesky(G)
    x = np.linalg.solve(L.T, np.linalg.solve(L, r))
    return _finish(x, d, delta, shapley)


def fit_bar(bits, wtab, d, ridge, shapley, phi_ref):
    """-> (cond_2 of the system, bar (T, 1)): |phi - phi_ref| <= (K + 10 (d + 1)) 2^-52 cond_2 max|phi_ref| per word.  K: the
    formation error of a K-term sum per Gram entry; 10 (d + 1): Cholesky's backward error gamma_{3n+1} (Higham, Accuracy and
    Stability of Numerical Algorithms, theorem 10.4) and a factor 2 for the right-hand side."""
    K = len(bits)
    cond = float(np.linalg.cond(system(bits, wtab, d, ridge, shapley), 2))
    return cond, (K + 10 * (d + 1)) * 2.0 ** -52 * cond * np.abs(phi_ref).max(axis=1, keepdims=True)


def lime_weights(d, kernel_width=0.25):
    m = np.arange(d + 1, dtype=np.float64)
    return np.sqrt(np.exp(-(1.0 - np.sqrt(m / d)) ** 2 / kernel_width ** 2))


def sampled_shapley_weights(d):
    w = np.ones(d + 1)
    w[0] = w[d] = 0.0
    return w


# (n_img, K, T, d) of the operator tests, CPU and GPU alike; the first runs at ridge 1 only
FIT_CASES = [(1, 8, 1, 2), (3, 64, 5, 16), (2, 300, 8, 33), (1, 520, 3, 128)]
FIT_RUNS = [(c, r) for c in FIT_CASES for r in (0.0, 1.0) if not (c[3] == 2 and r == 0.0)]


def fit_case(n_img, K, T, d, shapley, thr):
    """A regression problem of the given size on the restated draws: Bernoulli rows behind the all-ones row (LIME form) or
    antithetic Shapley pairs; y is a linear set function of unit-size coefficients plus 5 % noise, as a word score is to first
    order.  -> bits (n_img, K, 4) uint32, wtab, y (n_img, K, T), delta (n_img, T) or None"""
    rs = np.random.RandomState(1000 * d + K + (7 if shapley else 0))
    keys = rs.randint(0, 2 ** 32, size=n_img, dtype=np.int64)
    seed = (int(rs.randint(1, 2 ** 31)) << 32) + 99
    if shapley:
        bits = np.stack([draws([k] * K, range(K), d, SHAPLEY, thr=thr, seed=seed) for k in keys])
        wtab = sampled_shapley_weights(d)
    else:
        bits = np.stack([np.concatenate([np.array([pack(range(d), d)], dtype=np.uint32),
                                         draws([k] * (K - 1), range(K - 1), d, BERNOULLI, 0.5, seed=seed)]) for k in keys])
        wtab = lime_weights(d)
    coef = rs.randn(n_img, d, T)
    z = unpack(bits, d).astype(np.float64)
    y = z @ coef + 0.05 * rs.randn(n_img, K, T) + (0.0 if shapley else rs.randn(n_img, 1, T))
    delta = coef.sum(axis=1) + 0.05 * rs.randn(n_img, T) if shapley else None
    return bits, wtab, y, delta


# ---------------------------------------------------------------------------------------------------- Shapley values
def enumeration(d):
    """every proper subset 1 .. 2^d - 2 in ascending integer order as (2^d - 2, 4) uint32, and the Shapley kernel's weight table
    wtab[m] = (d - 1) / (C(d, m) m (d - m))"""
    bits = np.zeros((2 ** d - 2, WORDS), dtype=np.uint32)
    bits[:, 0] = np.arange(1, 2 ** d - 1, dtype=np.uint32)
    wtab = np.zeros(d + 1)
    for m in range(1, d):
        wtab[m] = (d - 1.0) / (comb(d, m) * m * (d - m))
    return bits, wtab


def shapley_brute(v, d):
    """v (2^d, ...) indexed by the subset's integer -> (d, ...): phi_i = sum over S without i of |S|! (d - |S| - 1)! / d!
    (v(S + i) - v(S))"""
    v = np.asarray(v, dtype=np.float64)
    phi = np.zeros((d,) + v.shape[1:])
    for i in range(d):
        rest = [j for j in range(d) if j != i]
        for m in range(d):
            c = factorial(m) * factorial(d - m - 1) / factorial(d)
            for S in combinations(rest, m):
                s = sum(1 << j for j in S)
                phi[i] += c * (v[s | (1 << i)] - v[s])
    return phi
