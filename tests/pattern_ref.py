"""Restatement of PatternNet / PatternAttribution for the VGG-style encoders, in torch on the CPU (float64 unless said otherwise).

Fit (innvestigate/tools/pattern.py:220-336): per conv, over the im2col rows X (K = 9 cin in HWIO order, zero padded) of the layer
input and Y = X W (no bias, no activation), with mask = 1 ('linear'), [Y + b > 0] ('relu' = 'relu.positive') or [Y + b <= 0]
('relu.negative') per position and channel:
    cnt = sum mask,  Sx = X^T mask,  Sxy = X^T (Y mask),  Sy = sum Y,  P = positions
    mean_x = Sx / safe(cnt), mean_xy = Sxy / safe(cnt), mean_y = Sy / P,  safe(v) = v + [v == 0]
    cov = mean_xy - mean_x mean_y,  A = cov / safe(sum_k W cov)
`fit_sums` + `compute_pattern` is that with plain sums; `fit_running` keeps the reference's running means batch by batch
(layers.py RunningMeans: new = old (1 - f) + batch f, f = batch count / safe(total count)), in any dtype.

Walk (analyzer/pattern_based.py:68-281): per conv + ReLU layer the ReLU's gradient, then the conv's gradient with the kernel replaced
by A (PatternNet) or A * W (PatternAttribution); pools take their own gradient; with reverse_project_bottleneck_layers (the
default) every reversed tensor — the head, the tensor at every layer's input, the result — is first divided per sample by its
absolute maximum (1 where that is 0)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import cnn_lrp_ref as C

TYPES = ("linear", "relu", "relu.positive", "relu.negative")


def conv_entries(layers):
    return [L for L in layers if L[0] == "conv"]


def im2col(x_nchw):
    """(N, C, H, W) -> (N H W, 9 C): column k = (ky * 3 + kx) * C + c, zero padded"""
    N, Cc, H, W = x_nchw.shape
    cols = F.unfold(x_nchw, 3, padding=1).view(N, Cc, 9, H * W)            # unfold's rows are (c, ky, kx)
    return cols.permute(0, 3, 2, 1).reshape(N * H * W, 9 * Cc)


def _mask(Y, b, pattern_type):
    if pattern_type == "linear":
        return torch.ones_like(Y)
    if pattern_type in ("relu", "relu.positive"):
        return (Y + b > 0).to(Y.dtype)
    if pattern_type == "relu.negative":
        return (Y + b <= 0).to(Y.dtype)
    raise ValueError("unknown pattern type %r" % (pattern_type,))


def _layer_xy(layers, X_nhwc, dtype):
    """per conv: (im2col rows of its input, W as (9 cin, cout), b) in `dtype`"""
    _, inputs = C.forward(layers, X_nhwc, dtype, return_inputs=True)
    out = []
    for L, x in zip(layers, inputs):
        if L[0] == "conv":
            W = torch.as_tensor(np.ascontiguousarray(L[1])).to(dtype).reshape(-1, L[1].shape[-1])
            out.append((im2col(x), W, torch.as_tensor(np.ascontiguousarray(L[2])).to(dtype)))
    return out


def fit_sums(layers, X_nhwc, pattern_type, dtype=torch.float64, with_abs=False):
    """per conv a dict of numpy arrays Sx, Sxy (9 cin, cout), cnt, Sy (cout,), P; with_abs: also the sums of the terms' absolute
    values (aSx, aSxy, aSy) that bound a float32 summation's error"""
    out = []
    for Xc, W, b in _layer_xy(layers, X_nhwc, dtype):
        Y = Xc @ W
        m = _mask(Y, b, pattern_type)
        d = dict(Sx=Xc.t() @ m, Sxy=Xc.t() @ (Y * m), cnt=m.sum(0), Sy=Y.sum(0), P=float(Xc.shape[0]))
        if with_abs:
            d.update(aSx=Xc.abs().t() @ m, aSxy=Xc.abs().t() @ (Y.abs() * m), aSy=Y.abs().sum(0))
        out.append({k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    return out


def add_sums(a, b):
    return [{k: x[k] + y[k] for k in x} for x, y in zip(a, b)]


def _safe(v):
    return v + (v == 0)


def pattern_from_means(W2d, mean_x, mean_xy, mean_y):
    cov = mean_xy - mean_x * mean_y
    d = (W2d * cov).sum(0)
    return cov / _safe(d)[None, :]


def compute_pattern(W_hwio, s):
    """sums -> A (3, 3, cin, cout), in the dtype of the sums"""
    W2d = np.asarray(W_hwio).reshape(-1, W_hwio.shape[-1]).astype(s["Sx"].dtype)
    cnt = _safe(s["cnt"])
    A = pattern_from_means(W2d, s["Sx"].reshape(W2d.shape) / cnt, s["Sxy"].reshape(W2d.shape) / cnt, s["Sy"] / s["P"])
    return A.reshape(W_hwio.shape)


def fit(layers, X_nhwc, pattern_type, dtype=torch.float64):
    """patterns from the plain sums over all of X: a list of (3, 3, cin, cout) arrays"""
    sums = fit_sums(layers, X_nhwc, pattern_type, dtype)
    return [compute_pattern(L[1], s) for L, s in zip(conv_entries(layers), sums)]


def fit_running(layers, X_nhwc, pattern_type, batch, dtype=torch.float32):
    """the reference's running means, batch by batch, in `dtype` throughout"""
    np_dt = np.float32 if dtype == torch.float32 else np.float64
    state = None
    for lo in range(0, len(X_nhwc), batch):
        sums = fit_sums(layers, X_nhwc[lo:lo + batch], pattern_type, dtype)
        if state is None:
            state = [dict(mx=np.zeros_like(s["Sx"]), cx=np.zeros_like(s["cnt"]), mxy=np.zeros_like(s["Sxy"]),
                          my=np.zeros_like(s["Sy"]), cy=np_dt(0)) for s in sums]
        for st, s in zip(state, sums):
            cnt, P = s["cnt"].astype(np_dt), np_dt(s["P"])
            f = cnt / _safe(cnt + st["cx"])
            st["mx"] = st["mx"] * (1 - f) + s["Sx"] / _safe(cnt) * f
            st["mxy"] = st["mxy"] * (1 - f) + s["Sxy"] / _safe(cnt) * f
            st["cx"] = st["cx"] + cnt
            fy = P / _safe(P + st["cy"])
            st["my"] = st["my"] * (1 - fy) + s["Sy"] / P * fy
            st["cy"] = st["cy"] + P
    out = []
    for L, st in zip(conv_entries(layers), state):
        W2d = np.asarray(L[1]).reshape(-1, L[1].shape[-1]).astype(np_dt)
        out.append(pattern_from_means(W2d, st["mx"], st["mxy"], st["my"]).astype(np_dt).reshape(L[1].shape))
    return out


def project(t):
    """t (N, ...) / its per-sample absolute maximum, 1 where that is 0"""
    m = t.abs().reshape(t.shape[0], -1).max(1).values
    m = m + (m == 0).to(t.dtype)
    return t / m.reshape((-1,) + (1,) * (t.dim() - 1))


def walk(layers, X_nhwc, head_nhwc, patterns, attribution=False, projection=True, dtype=torch.float64):
    """`PatternNet(model, patterns).analyze([X, head])` (attribution: PatternAttribution): (N, H, W, 3) numpy"""
    _, inputs = C.forward(layers, X_nhwc, dtype, return_inputs=True)
    pats = list(patterns)
    g = C._nchw(C._t(head_nhwc, dtype))
    if projection:
        g = project(g)
    for L, x in zip(reversed(layers), reversed(inputs)):
        if L[0] == "conv":
            w, b = C._w_oihw(L[1], dtype), C._t(L[2], dtype)
            a = C._w_oihw(pats.pop(), dtype)
            if attribution:
                a = a * w
            g = g * (F.conv2d(x, w, b, padding=1) > 0).to(dtype)            # the ReLU's gradient
            g = F.conv_transpose2d(g, a, padding=1)                          # the conv's gradient with its kernel replaced
        else:
            g = C.gradient_route(x, lambda v: F.max_pool2d(v, 2, 2), g)
        if projection:
            g = project(g)
    return C._nhwc(g).numpy()
