"""Test helper (not a test module): CPU restatements of DeepLIFT and DeepTaylor on the VGG-style encoders.

  * deeplift_vgg          `DeepLIFT(model, neuron_selection_mode="replace", reference_inputs=r, approximate_gradient=...)
                          .analyze([X, head])` (innvestigate/analyzer/deeplift.py:44-250), literal: one autograd call per GradientWRT
                          of the published graph, as oracle.cnn_lrp_ref.gradient_analyze is written.  Every Conv2D(activation='relu')
                          contains a kernel and takes LinearRule on the FUSED layer (:77-115); max-pools take the plain gradient; the
                          head is the caller's tensor (_head_mapping is not applied in 'replace' mode); the reference activations come
                          from a full forward of ONE reference, broadcast to (1, H, W, 3), through the same layers.
  * deeplift_vgg_cached   what the device does: per layer and image the gate D = M ? safe(Y - Yr) : 0 (through a pool: at the image's
                          first arg-max), two chains [t ; g] against the transposed conv with the full w, the per-element select
  * deeplift_stats        per conv: the share of units that are alive with dY == 0 (SafeDivide's A x 1e7 branch)
  * dyadic_vgg_weights    a net on which float32 and float64 forwards agree bit for bit (see its docstring)
  * op_deeplift_conv_ref  lrp_op_deeplift_conv in torch, and the mass each of its output elements was summed from
  * deeptaylor_vgg        DeepTaylor / BoundedDeepTaylor (deeptaylor.py:40-199), literal
"""
import numpy as np
import torch
import torch.nn.functional as F

import rule_table_ref as RT
from oracle import cnn_lrp_ref as C

EPS = 1e-7      # K.epsilon()


def _reference(reference, X_nhwc):
    """reference_inputs broadcast to ONE image (utils/keras/__init__.py:60-74)"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(reference, dtype=np.float64), (1,) + tuple(X_nhwc.shape[1:])))


def _fused(L, dtype):
    w, b = C._w_oihw(L[1], dtype), C._t(L[2], dtype)
    return lambda v: F.relu(F.conv2d(v, w, b, padding=1))


def _grad(f, x, S):
    xr = x.detach().requires_grad_(True)
    g, = torch.autograd.grad(f(xr), xr, grad_outputs=S)
    return g.detach()


def deeplift_vgg(layers, X_nhwc, head_nhwc, reference=0, approximate_gradient=True, dtype=torch.float64):
    _, inputs = C.forward(layers, X_nhwc, dtype, return_inputs=True)
    _, ref_inputs = C.forward(layers, _reference(reference, X_nhwc), dtype, return_inputs=True)
    A = C._nchw(C._t(head_nhwc, dtype))
    for L, x, xr in zip(reversed(layers), reversed(inputs), reversed(ref_inputs)):
        if L[0] == "pool":
            A = _grad(lambda v: F.max_pool2d(v, 2, 2), x, A)
            continue
        f = _fused(L, dtype)
        dX, dY = x - xr, f(x) - f(xr)                          # Subtract()([x, r]): the one reference broadcasts over the batch
        tmp = dX * _grad(f, x, C.safe_divide(A, dY))           # :98-108
        if approximate_gradient:
            g = _grad(f, x, A)                                  # :111
            A = torch.where(dX.abs() < EPS, g, tmp)             # :79-81
        else:
            A = tmp
    return C._nhwc(A).numpy()


def _gates(layers, X_nhwc, reference, dtype):
    """per conv (input first): (x, xr, D, pooled) — D at the conv's own resolution, non-zero where the unit is alive and, with a
    pool behind it, is the first arg-max of its window"""
    convs = []
    x = C._nchw(C._t(X_nhwc, dtype))
    xr = C._nchw(C._t(_reference(reference, X_nhwc), dtype))
    i = 0
    while i < len(layers):
        f = _fused(layers[i], dtype)
        y, yr = f(x), f(xr)
        pooled = i + 1 < len(layers) and layers[i + 1][0] == "pool"
        M = y > 0
        if pooled:
            p, ind = F.max_pool2d(y, 2, 2, return_indices=True)
            M = M & (F.max_unpool2d(torch.ones_like(p), ind, 2, 2, output_size=y.shape[2:]) > 0)
        dY = y - yr
        D = torch.where(M, dY + (dY == 0).to(dtype) * EPS, torch.zeros_like(dY))
        convs.append((x, xr, D, pooled, layers[i]))
        x, xr = (F.max_pool2d(y, 2, 2), F.max_pool2d(yr, 2, 2)) if pooled else (y, yr)
        i += 2 if pooled else 1
    return convs


def deeplift_vgg_cached(layers, X_nhwc, idx, head_nhwc, reference=0, approximate_gradient=True, dtype=torch.float64):
    """X_nhwc: the B encoded images; idx: row -> image of the n heads"""
    convs = _gates(layers, X_nhwc, reference, dtype)
    idx = torch.as_tensor(list(idx), dtype=torch.long)
    two = bool(approximate_gradient)

    def gate(o, D):                                          # both gates of one layer from what arrives at its output
        on = D[idx] != 0
        t = torch.where(on, o / torch.where(on, D[idx], torch.ones_like(o)), torch.zeros_like(o))
        return torch.cat([t, torch.where(on, o, torch.zeros_like(o))]) if two else t

    n = len(idx)
    S = gate(C._nchw(C._t(head_nhwc, dtype)), convs[-1][2])
    for li in range(len(convs) - 1, -1, -1):
        x, xr, _, _, L = convs[li]
        c = F.conv_transpose2d(S, C._w_oihw(L[1], dtype), padding=1)
        dX = x[idx] - xr
        o = torch.where(dX.abs() < EPS, c[n:], dX * c[:n]) if two else dX * c
        if li == 0:
            return C._nhwc(o).numpy()
        if convs[li - 1][3]:
            o = F.interpolate(o, scale_factor=2, mode="nearest")
        S = gate(o, convs[li - 1][2])


def deeplift_stats(layers, X_nhwc, reference=0, dtype=torch.float64):
    """per conv: units alive (ReLU on; behind a pool also the window's arg-max is NOT asked) whose dY is exactly 0, over all units"""
    out = []
    _, inputs = C.forward(layers, X_nhwc, dtype, return_inputs=True)
    _, ref_inputs = C.forward(layers, _reference(reference, X_nhwc), dtype, return_inputs=True)
    for L, x, xr in zip(layers, inputs, ref_inputs):
        if L[0] == "conv":
            f = _fused(L, dtype)
            y, yr = f(x), f(xr)
            out.append(float(((y > 0) & (y == yr)).to(torch.float64).mean()))
    return out


def dyadic_vgg_weights(rs, cfg):
    """Weights k 2^-s with k in {-1, 0, 1}, P(+-1) = 0.125 each, s = round(log2 sqrt(9 cin / 4)); biases multiples of 0.5 in
    [-1, 1].  With integer images in [-4, 4] and integer references every activation of a shallow, narrow net is a dyadic
    rational with few bits, so float32 and float64 forwards agree BIT FOR BIT: dX and dY are exact, every ReLU / switch / dY == 0
    decision is the same in any arithmetic, and |A / dY| is bounded by 2^(sum of s) |A|.  The property does not survive a finer
    grid or a deeper / wider net: a test asserts it for its own draw (forward_is_exact) before using it."""
    w = {}
    for name, cin, cout, _ in cfg:
        s = int(round(np.log2(np.sqrt(9 * cin * 0.25))))
        k = rs.choice([-1.0, 0.0, 1.0], size=(3, 3, cin, cout), p=[0.125, 0.75, 0.125])
        w[name + "_W"] = (k * 2.0 ** -s).astype(np.float32)
        w[name + "_b"] = (rs.randint(-2, 3, size=cout) * 0.5).astype(np.float32)
    return w


def forward_is_exact(layers, X_nhwc):
    """float32 forward == float64 forward in every layer input and the output, bit for bit"""
    o32, i32 = C.forward(layers, X_nhwc, torch.float32, return_inputs=True)
    o64, i64 = C.forward(layers, X_nhwc, torch.float64, return_inputs=True)
    return bool(np.array_equal(o32.astype(np.float64), o64)) and all(torch.equal(a.double(), b) for a, b in zip(i32, i64))


# ------------------------------------------------------------------------------------------------------------ operator
def op_deeplift_conv_ref(x, xr, a, w_hwio, bias, pool, approximate_gradient=True, dtype=torch.float64):
    """lrp_op_deeplift_conv on NHWC torch tensors (x (NB, H, W, Cin), xr (H, W, Cin), a at pooled resolution with pool) ->
    (out, mass): mass = |dX| (|M a / safe(dY)| convT |w|), or (|M a| convT |w|) where the gradient is selected"""
    layers = [("conv", np.asarray(w_hwio), np.asarray(bias))] + ([("pool",)] if pool else [])
    xn, xrn = C._nchw(x.to(dtype)), C._nchw(xr.to(dtype)[None])
    f = _fused(layers[0], dtype)
    A = C._nchw(a.to(dtype))
    if pool:
        A = _grad(lambda v: F.max_pool2d(v, 2, 2), f(xn), A)
    dX, dY = xn - xrn, f(xn) - f(xrn)
    M = (f(xn) > 0).to(dtype)
    wt = C._w_oihw(w_hwio, dtype)
    s = C.safe_divide(A, dY) * M
    t = dX * F.conv_transpose2d(s, wt, padding=1)
    g = F.conv_transpose2d(A * M, wt, padding=1)
    mt = dX.abs() * F.conv_transpose2d(s.abs(), wt.abs(), padding=1)
    mg = F.conv_transpose2d((A * M).abs(), wt.abs(), padding=1)
    if approximate_gradient:
        sel = dX.abs() < EPS
        return C._nhwc(torch.where(sel, g, t)), C._nhwc(torch.where(sel, mg, mt))
    return C._nhwc(t), C._nhwc(mt)


# ------------------------------------------------------------------------------------------------------------ DeepTaylor
def deeptaylor_vgg(layers, X_nhwc, head_nhwc, bounds=None, dtype=torch.float64):
    """DeepTaylor(model).analyze([X, head]) (deeptaylor.py:40-155), BoundedDeepTaylor with bounds = (low, high) (:157-199): the model
    gets a ReLU on its output (:144-154), which a head in 'replace' mode passes by the gradient mapping (:69-75); every fused conv
    takes Alpha1Beta0Rule (:55-61), the input conv BoundedRule under bounds (:184-195); pools by the gradient (:83-87)."""
    feat, inputs = C.forward(layers, X_nhwc, dtype, return_inputs=True)
    top = C._nchw(C._t(feat, dtype))
    R = _grad(F.relu, top, C._nchw(C._t(head_nhwc, dtype)))
    for k in range(len(layers) - 1, -1, -1):
        L, x = layers[k], inputs[k]
        if L[0] == "pool":
            R = _grad(lambda v: F.max_pool2d(v, 2, 2), x, R)
        elif k == 0 and bounds is not None:
            R = RT.bounded_conv(x, C._w_oihw(L[1], dtype), R, bounds[0], bounds[1], dtype)
        else:
            R = C.alpha1beta0_conv(x, L[1], L[2], R, dtype)
    return C._nhwc(R).numpy()
