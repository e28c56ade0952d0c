"""Test helper: CPU restatement of AlphaBetaRule.apply (relevance_rule.py:274-322, bias=True) for general (alpha, beta), in the
shape of oracle.cnn_lrp_ref.alpha1beta0_conv / analyze — one autograd call per GradientWRT of the published graph.

    x+ = x [x >= 0], x- = x [x < 0];  w+-, b+- likewise (RR:256-260, :279-280)
    act = f(layer+, layer-, x+, x-):  Z = conv(x+, w+) + b+ + conv(x-, w-) + b-;  S = SafeDivide(R, Z)
                                      x+ * grad(conv(x+, w+), S) + x- * grad(conv(x-, w-), S)
    inh = f(layer-, layer+, x+, x-):  the same with the layers swapped          (only computed when beta != 0, RR:314)
    R_in = alpha act - beta inh

`dtype` float64 is the reference of the GPU tests, float32 the same graph in the arithmetic the reference runs in (the tests'
own error bar)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.cnn_lrp_ref import _nchw, _nhwc, _t, _w_oihw, forward, gradient_route, safe_divide


def _branch(x1, x2, w1, b1, w2, b2, R):
    """f(layer1, layer2, X1, X2) of RR:283-303."""
    x1 = x1.detach().requires_grad_(True)
    x2 = x2.detach().requires_grad_(True)
    Z1 = F.conv2d(x1, w1, b1, padding=w1.shape[-1] // 2)
    Z2 = F.conv2d(x2, w2, b2, padding=w2.shape[-1] // 2)
    S = safe_divide(R, (Z1 + Z2).detach())
    g1, = torch.autograd.grad(Z1, x1, grad_outputs=S)
    g2, = torch.autograd.grad(Z2, x2, grad_outputs=S)
    return (x1 * g1 + x2 * g2).detach()


def alphabeta_conv(x, W_hwio, b, R, alpha, beta, dtype):
    """RR:274-322 for one Conv2D (NCHW tensors)."""
    w = _w_oihw(W_hwio, dtype)
    bias = _t(b, dtype)
    wp, wn = w * (w >= 0).to(dtype), w * (w < 0).to(dtype)
    bp, bn = bias * (bias >= 0).to(dtype), bias * (bias < 0).to(dtype)
    xp, xn = x * (x >= 0).to(dtype), x * (x < 0).to(dtype)
    act = _branch(xp, xn, wp, bp, wn, bn, R)
    if not beta:
        return act
    inh = _branch(xp, xn, wn, bn, wp, bp, R)
    return act * alpha - inh * beta


def analyze(layers, X_nhwc, R_nhwc, alpha, beta, dtype=torch.float64):
    """`LRPAlphaBeta(model, alpha, beta).analyze([X, R])`: every conv by alphabeta_conv, max-pools by gradient routing."""
    _, inputs = forward(layers, X_nhwc, dtype, return_inputs=True)
    R = _nchw(_t(R_nhwc, dtype))
    for L, x in zip(reversed(layers), reversed(inputs)):
        if L[0] == "conv":
            R = alphabeta_conv(x, L[1], L[2], R, alpha, beta, dtype)
        else:
            R = gradient_route(x, lambda v: F.max_pool2d(v, 2, 2), R)
    return _nhwc(R).numpy()


def min_abs_denominator(layers, X_nhwc, dtype=torch.float64):
    """smallest |Z_act| and |Z_inh| over every unit of every conv (conditioning of a draw)."""
    _, inputs = forward(layers, X_nhwc, dtype, return_inputs=True)
    worst = np.inf
    for L, x in zip(layers, inputs):
        if L[0] != "conv":
            continue
        w, bias = _w_oihw(L[1], dtype), _t(L[2], dtype)
        wp, wn = w * (w >= 0).to(dtype), w * (w < 0).to(dtype)
        xp, xn = x * (x >= 0).to(dtype), x * (x < 0).to(dtype)
        za = F.conv2d(xp, wp, padding=1) + F.conv2d(xn, wn, padding=1) + bias.view(1, -1, 1, 1)
        zi = F.conv2d(xp, wn, padding=1) + F.conv2d(xn, wp, padding=1) + bias.view(1, -1, 1, 1)
        worst = min(worst, float(za.abs().min()), float(zi.abs().min()))
    return worst


def op_conv_ab_ref(sp, sn, w_hwio, alpha, beta, gp, gn, pool, dtype=torch.float64):
    """lrp_op_conv_ab in torch (NHWC tensors in, NHWC out), in the dtype given:
    c = convT(sp, alpha w+) + convT(sn, -beta w-), 2x2 nearest with pool; (c gp, c gn)."""
    w = torch.as_tensor(np.ascontiguousarray(w_hwio)).to(sp.device, dtype).permute(3, 2, 0, 1).contiguous()     # (Cout, Cin, 3, 3)
    wp, wn = w * (w >= 0).to(dtype), w * (w < 0).to(dtype)
    c = F.conv_transpose2d(_nchw(sp.to(dtype)), wp * alpha, padding=1) + F.conv_transpose2d(_nchw(sn.to(dtype)), wn * (-beta), padding=1)
    if pool:
        c = F.interpolate(c, scale_factor=2, mode="nearest")
    c = _nhwc(c)
    return c * gp.to(dtype), c * gn.to(dtype)
