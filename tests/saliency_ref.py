"""numpy restatement of the occlusion and RISE operators (include/lrp_hip.h, lrp_op_occlude / _occlusion_map / _rise_*): the window
geometry, the occluded rows, the occlusion map, the RISE grids on gradient_family_ref.philox4x32_10, the mask formula in float64 and
the RISE map.  Plain loops where a loop is the clearest statement; everything is float64 unless it is a copy."""
import numpy as np

from gradient_family_ref import philox4x32_10


def _pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def geometry(H, W, window, stride=None):
    """(Hn, Wn): Hn = ceil((H - ph) / sh) + 1"""
    (ph, pw), (sh, sw) = _pair(window), _pair(window if stride is None else stride)
    assert 1 <= sh <= ph <= H and 1 <= sw <= pw <= W
    return -(-(H - ph) // sh) + 1, -(-(W - pw) // sw) + 1


def window_box(k, H, W, window, stride=None):
    """rows [y0, y1) and columns [x0, x1) of window k = i * Wn + j, clipped at the image"""
    (ph, pw), (sh, sw) = _pair(window), _pair(window if stride is None else stride)
    _, Wn = geometry(H, W, window, stride)
    i, j = divmod(int(k), Wn)
    return i * sh, min(i * sh + ph, H), j * sw, min(j * sw + pw, W)


def occlude(x, img_idx, ks, window, stride=None, fill=0.0):
    """x (B, H, W, C) float32 -> (n, H, W, C) float32; k = -1 copies; an index or k out of range gives a NaN row"""
    B, H, W, C = x.shape
    Hn, Wn = geometry(H, W, window, stride)
    f = np.broadcast_to(np.asarray(fill, dtype=np.float32).reshape(-1), (C,))
    out = np.empty((len(ks), H, W, C), dtype=np.float32)
    for r, (b, k) in enumerate(zip(img_idx, ks)):
        if not (0 <= b < B and -1 <= k < Hn * Wn):
            out[r] = np.nan
            continue
        out[r] = x[b]
        if k >= 0:
            y0, y1, x0, x1 = window_box(k, H, W, window, stride)
            out[r, y0:y1, x0:x1] = f
    return out


def coverage(H, W, window, stride=None):
    """c (H, W): the number of windows covering each pixel"""
    Hn, Wn = geometry(H, W, window, stride)
    c = np.zeros((H, W), dtype=np.int64)
    for k in range(Hn * Wn):
        y0, y1, x0, x1 = window_box(k, H, W, window, stride)
        c[y0:y1, x0:x1] += 1
    return c


def occlusion_map(scores, H, W, window, stride=None):
    """scores (n_img, 1 + Hn Wn, T) float64 -> (S, A) each (n_img, T, H, W) float64: S = sum over covering k (ascending) of
    (s_0 - s_{1+k}) / c, A = sum |s_0 - s_{1+k}| / c (the magnitude the error bar is stated against)"""
    scores = np.asarray(scores, dtype=np.float64)
    n_img, rows, T = scores.shape
    Hn, Wn = geometry(H, W, window, stride)
    assert rows == 1 + Hn * Wn
    S, A = np.zeros((n_img, T, H, W)), np.zeros((n_img, T, H, W))
    for k in range(Hn * Wn):
        y0, y1, x0, x1 = window_box(k, H, W, window, stride)
        d = scores[:, 0, :] - scores[:, 1 + k, :]
        S[:, :, y0:y1, x0:x1] += d[:, :, None, None]
        A[:, :, y0:y1, x0:x1] += np.abs(d)[:, :, None, None]
    c = coverage(H, W, window, stride).astype(np.float64)
    return S / c, A / c


def rise_cell(H, W, s):
    return -(-H // s), -(-W // s)


def rise_grids(keys, ks, s, p, seed, cell):
    """-> grid (n, (s + 1)^2) uint8, shift (n, 2) int32.  Cell e takes lane e % 4 of Philox counter (e / 4, k, key, 1) under the
    key (seed & 0xFFFFFFFF, seed >> 32); G = 1 iff (x >> 8) < floor(p 2^24); the shift from counter (0xFFFFFFFF, k, key, 1)."""
    ch, cw = cell
    keys = np.asarray(keys, dtype=np.int64) & 0xFFFFFFFF
    ks = np.asarray(ks, dtype=np.int64) & 0xFFFFFFFF
    n, cells = len(ks), (s + 1) ** 2
    groups = (cells + 3) // 4
    ctr = np.zeros((n, groups + 1, 4), dtype=np.uint64)
    ctr[:, :groups, 0] = np.arange(groups, dtype=np.uint64)[None, :]
    ctr[:, groups, 0] = 0xFFFFFFFF
    ctr[:, :, 1] = ks[:, None]
    ctr[:, :, 2] = keys[:, None]
    ctr[:, :, 3] = 1
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    x = philox4x32_10(ctr, np.broadcast_to(key, ctr.shape[:-1] + (2,)))
    thresh = int(np.floor(float(p) * 2.0 ** 24))
    grid = ((x[:, :groups] >> np.uint32(8)).astype(np.int64) < thresh).astype(np.uint8).reshape(n, -1)[:, :cells]
    shift = np.stack([x[:, groups, 0].astype(np.int64) % ch, x[:, groups, 1].astype(np.int64) % cw], axis=1).astype(np.int32)
    return np.ascontiguousarray(grid), shift


def _axis(pos, cell, s):
    """Y = y + dy (an int array): ny = 2 Y + 1 - cell, a0 = floor_div(ny, 2 cell), f = (ny - 2 cell a0) / (2 cell); a0 and a0 + 1
    clamped into [0, s]"""
    ny = 2 * pos + 1 - cell
    a0 = ny // (2 * cell)                                      # numpy's // floors
    f = (ny - 2 * cell * a0) / float(2 * cell)
    return np.clip(a0, 0, s), np.clip(a0 + 1, 0, s), f


def rise_masks(grid, shift, H, W, s, cell):
    """(n, H, W) float64: m = top + fy (bot - top), top = G[a0][c0] + fx (G[a0][c1] - G[a0][c0]), bot alike on row a1"""
    ch, cw = cell
    grid = np.asarray(grid)
    out = np.empty((len(grid), H, W))
    for r in range(len(grid)):
        G = grid[r].reshape(s + 1, s + 1).astype(np.float64)
        a0, a1, fy = _axis(np.arange(H) + int(shift[r][0]), ch, s)
        c0, c1, fx = _axis(np.arange(W) + int(shift[r][1]), cw, s)
        top = G[a0][:, c0] + fx[None, :] * (G[a0][:, c1] - G[a0][:, c0])
        bot = G[a1][:, c0] + fx[None, :] * (G[a1][:, c1] - G[a1][:, c0])
        out[r] = top + fy[:, None] * (bot - top)
    return out


def rise_apply(x, img_idx, grid, shift, s, cell, fill=0.0):
    """float64 statement of fill + m (x - fill): -> (n, H, W, C) float64"""
    B, H, W, C = x.shape
    f = np.broadcast_to(np.asarray(fill, dtype=np.float64).reshape(-1), (C,))
    m = rise_masks(grid, shift, H, W, s, cell)
    xs = x[np.asarray(img_idx)].astype(np.float64)
    return f + m[..., None] * (xs - f)


def rise_map(scores, grid, shift, H, W, s, p, cell):
    """scores (n_img, K, T), grid (n_img, K, cells), shift (n_img, K, 2) -> (S, A) each (n_img, T, H, W) float64:
    S = sum_k s_k[t] m_k / (K p), A = sum_k |s_k[t]| m_k / (K p)"""
    scores = np.asarray(scores, dtype=np.float64)
    n_img, K, T = scores.shape
    S, A = np.zeros((n_img, T, H, W)), np.zeros((n_img, T, H, W))
    for i in range(n_img):
        m = rise_masks(np.asarray(grid)[i], np.asarray(shift)[i], H, W, s, cell)          # (K, H, W)
        S[i] = np.einsum("kt,kyx->tyx", scores[i], m)
        A[i] = np.einsum("kt,kyx->tyx", np.abs(scores[i]), m)
    return S / (K * p), A / (K * p)


def map_bar(ref, mag):
    """the bar of the map operators: one float32 rounding of the result, and the float64 summation error of the terms"""
    return 2.0 ** -23 * np.abs(ref) + 1e-12 * mag
