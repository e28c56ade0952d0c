"""numpy restatement of the CAM family operators (include/lrp_hip.h, csrc/cam_kernels.h): the five coarse maps of lrp_op_cam, the
three weightings of lrp_op_cam_weighted and the finish in float64, with lrp_eval_expand_matrix for M as tests/test_gpu_gradcam.py
does; the Score-CAM mask in float32 in the operator's rounding order; the ablation as index assignment.  Every float64 result
comes with its `mass`: the same expression over absolute values, which the error bar is stated against (as saliency_ref.map_bar)."""
import numpy as np

MODES = ("gradcam", "gradcam++", "xgradcam", "layercam", "hirescam")
WEIGHTS = ("softmax", "linear", "ablation")
_M = {}


def expand_matrix(g, up):
    if (g, up) not in _M:
        from lrp_imagecaptioning_amd import engine as E
        _M[(g, up)] = E.eval_expand_matrix(g, up)              # (S, g) float64, host arithmetic
        _M[(g, up)].setflags(write=False)
    return _M[(g, up)]


# ---------------------------------------------------------------------------------------------------- coarse maps
def coarse(F, G, mode):
    """F, G (L, D) -> (A, A_abs) each (L,) float64: the coarse map and the same sums over absolute values"""
    F, G = np.asarray(F, dtype=np.float64), np.asarray(G, dtype=np.float64)
    aF, aG = np.abs(F), np.abs(G)
    if mode == "gradcam":
        w, wa = G.mean(axis=0), aG.mean(axis=0)
    elif mode == "gradcam++":
        S = F.sum(axis=0)
        den = 2.0 * G ** 2 + S[None, :] * G ** 3
        alpha = np.where(den != 0.0, G ** 2 / np.where(den != 0.0, den, 1.0), 0.0)
        w, wa = (alpha * np.maximum(G, 0.0)).sum(axis=0), (np.abs(alpha) * np.maximum(G, 0.0)).sum(axis=0)
    elif mode == "xgradcam":
        S = F.sum(axis=0) + 1e-7
        w, wa = (F * G).sum(axis=0) / S, (aF * aG).sum(axis=0) / np.abs(S)
    elif mode == "layercam":
        return (np.maximum(G, 0.0) * F).sum(axis=1), (np.maximum(G, 0.0) * aF).sum(axis=1)
    elif mode == "hirescam":
        return (G * F).sum(axis=1), (aG * aF).sum(axis=1)
    else:
        raise ValueError(mode)
    return F @ w, aF @ wa


def weights(s0, s, s_fill, mode):
    """s (D,) the channel scores of one word -> (w, w_abs) each (D,)"""
    s = np.asarray(s, dtype=np.float64)
    if mode == "softmax":
        e = np.exp(s - s.max())
        w = e / e.sum()
        return w, w
    if mode == "linear":
        return s - s_fill, np.abs(s) + abs(s_fill)
    if mode == "ablation":
        if s0 == 0.0:
            return np.zeros_like(s), np.zeros_like(s)
        return (s0 - s) / abs(s0), (abs(s0) + np.abs(s)) / abs(s0)
    raise ValueError(mode)


# ---------------------------------------------------------------------------------------------------- the finish
def finish(A, A_abs, g, up):
    """A (L,) -> (cam (S, S) float64, mass (S, S), mx): cam = max(M A M^T, 0) / (max + 1e-6); mass = |M| A_abs |M|^T in the units
    of the unnormalised cam, mx its maximum: an element's bar is c * mass / (mx + 1e-6)"""
    M = expand_matrix(g, up)
    cam = np.maximum(M @ np.asarray(A).reshape(g, g) @ M.T, 0.0)
    mx = cam.max()
    mass = np.abs(M) @ np.asarray(A_abs).reshape(g, g) @ np.abs(M).T
    return cam / (mx + 1e-6), mass, mx


def bar(L, D, mass, mx):
    """|got - ref| <= 4 L D 2^-52 mass / (max + 1e-6): L D products per coarse map (every form sums at most that many), each with
    a handful of roundings, carried through the linear finish"""
    return 4.0 * L * D * 2.0 ** -52 * mass / (mx + 1e-6)


def cam(F, G, mode, g, up):
    """-> (cam, bar) of one unit"""
    A, Aa = coarse(F, G, mode)
    c, mass, mx = finish(A, Aa, g, up)
    return c, bar(F.shape[0], F.shape[1], mass, mx)


def cam_weighted(scores, F, mode, g, up):
    """scores (R, T) of one image, F (L, D) -> (cams (T, S, S), bars (T, S, S)); a NaN score gives a NaN map"""
    L, D = F.shape
    F = np.asarray(F, dtype=np.float64)
    cams, bars = [], []
    for t in range(scores.shape[1]):
        w, wa = weights(scores[0, t], scores[1:1 + D, t], scores[1 + D, t] if mode == "linear" else 0.0, mode)
        c, mass, mx = finish(F @ w, np.abs(F) @ wa, g, up)
        cams.append(c)
        bars.append(bar(L, D, mass, mx))
    return np.stack(cams), np.stack(bars)


# ---------------------------------------------------------------------------------------------------- Score-CAM mask, float32
def _axis32(pos, up, s):
    """the half-pixel-centre rule of lrp_op_rise_apply at shift 0: n = 2 pos + 1 - up, a0 = floor_div(n, 2 up), f = (n - 2 up a0) /
    (2 up) as one float32 division of two exactly represented ints; a0 and a0 + 1 clamped into [0, s]"""
    n = 2 * pos + 1 - up
    a0 = n // (2 * up)
    f = (n - 2 * up * a0).astype(np.float32) / np.float32(2 * up)
    return np.clip(a0, 0, s), np.clip(a0 + 1, 0, s), f


def scorecam_mask(v, g, up):
    """v (L,) float32 -> (S, S) float32: (v - min) / (max - min) on the coarse grid (zeros where max == min), then top = n00 + fx
    (n01 - n00), bot alike, m = top + fy (bot - top), every operation a float32 operation"""
    v = np.asarray(v, dtype=np.float32).reshape(g, g)
    lo, hi = v.min(), v.max()
    n = np.zeros_like(v) if hi == lo else (v - lo) / (hi - lo)
    assert n.dtype == np.float32
    a0, a1, fy = _axis32(np.arange(g * up), up, g - 1)
    c0, c1, fx = a0, a1, fy
    top = n[a0][:, c0] + fx[None, :] * (n[a0][:, c1] - n[a0][:, c0])
    bot = n[a1][:, c0] + fx[None, :] * (n[a1][:, c1] - n[a1][:, c0])
    m = top + fy[:, None] * (bot - top)
    assert m.dtype == np.float32
    return m


def scorecam_apply(x, feat, img_idx, ks, g, up, fill=0.0):
    """x (B, H, W, C), feat (B, L, D) float32 -> (n, H, W, C) float32: fill + m (x - fill); k = -1 the image, k = D the fill image;
    an image index outside [0, B) or a k outside [-1, D] a NaN row"""
    B, H, W, C = x.shape
    D = feat.shape[2]
    f = np.broadcast_to(np.asarray(fill, dtype=np.float32).reshape(-1), (C,))
    out = np.empty((len(ks), H, W, C), dtype=np.float32)
    for r, (b, k) in enumerate(zip(img_idx, ks)):
        if not (0 <= b < B and -1 <= k <= D):
            out[r] = np.nan
        elif k == -1:
            out[r] = x[b]
        elif k == D:
            out[r] = f
        else:
            m = scorecam_mask(feat[b, :, k], g, up)
            out[r] = f + m[..., None] * (x[b] - f)
    assert out.dtype == np.float32
    return out


def feature_ablate(feat, img_idx, ks):
    """feat (B, L, D) -> (n, L, D): channel k set to 0, k = -1 a copy; out of range a NaN row"""
    B, L, D = feat.shape
    out = np.empty((len(ks), L, D), dtype=np.float32)
    for r, (b, k) in enumerate(zip(img_idx, ks)):
        if not (0 <= b < B and -1 <= k < D):
            out[r] = np.nan
            continue
        out[r] = feat[b]
        if k >= 0:
            out[r, :, k] = 0.0
    return out
