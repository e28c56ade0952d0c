"""Test helper: CPU restatement of the conv rules behind LRP(model, rule=..., input_layer_rule=...) (relevance_rule.py:74-441), one
rule per conv, in the shape of tests/alphabeta_ref.py — one autograd call per GradientWRT of the published graph.

A rule is the record LRPEngine.set_cnn_rules takes (lrp_imagecaptioning_amd.analyzer.normalize_rule):
    ("alphabeta", alpha, beta, bias)   AlphaBetaRule / AlphaBetaIgnoreBiasRule (RR:216-331): bias False drops b from both layers
    ("epsilon", eps, bias)             eps = 0: ZRule (RR:74-109), SafeDivide;  eps > 0: EpsilonRule (RR:113-152),
                                       Z + (2 [Z >= 0] - 1) eps and a plain divide
    ("flat",) / ("wsquare",)           FlatRule / WSquareRule (RR:156-211): Ys = layer'(x), Zs = layer'(1), R_in = grad(Ys, x; R / Zs)
                                       with layer' = the conv with weights 1 / w^2 and no bias — no multiply by x
    ("bounded", low, high)             BoundedRule (RR:372-441)

`dtype` float64 is the reference of the GPU tests, float32 the same graph in the arithmetic the reference runs in."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.cnn_lrp_ref import _nchw, _nhwc, _t, _w_oihw, forward, gradient_route, safe_divide


def _grad(Z, x, S):
    g, = torch.autograd.grad(Z, x, grad_outputs=S)
    return g


def alphabeta_conv(x, w, bias, R, alpha, beta, use_bias, dtype):
    """RR:274-322; use_bias False: RR:251-252, :257-258 (the bias is dropped before the sign split)."""
    wp, wn = w * (w >= 0).to(dtype), w * (w < 0).to(dtype)
    bp = bias * (bias >= 0).to(dtype) if use_bias else None
    bn = bias * (bias < 0).to(dtype) if use_bias else None
    xp, xn = x * (x >= 0).to(dtype), x * (x < 0).to(dtype)

    def f(w1, b1, w2, b2):
        x1 = xp.detach().requires_grad_(True)
        x2 = xn.detach().requires_grad_(True)
        Z1 = F.conv2d(x1, w1, b1, padding=1)
        Z2 = F.conv2d(x2, w2, b2, padding=1)
        S = safe_divide(R, (Z1 + Z2).detach())
        return (x1 * _grad(Z1, x1, S) + x2 * _grad(Z2, x2, S)).detach()

    act = f(wp, bp, wn, bn)
    if not beta:
        return act
    return act * alpha - f(wn, bn, wp, bp) * beta


def epsilon_conv(x, w, bias, R, eps, use_bias, dtype):
    """RR:85-98 (eps = 0) / RR:128-144."""
    xr = x.detach().requires_grad_(True)
    Z = F.conv2d(xr, w, bias if use_bias else None, padding=1)
    Zd = Z.detach()
    S = safe_divide(R, Zd) if not eps else R / (Zd + ((Zd >= 0).to(dtype) * 2 - 1) * eps)
    return (xr * _grad(Z, xr, S)).detach()


def wsquare_conv(x, w_sub, R):
    """RR:174-187 with the layer's weights replaced by w_sub (w^2, or ones for FlatRule)."""
    xr = x.detach().requires_grad_(True)
    Ys = F.conv2d(xr, w_sub, None, padding=1)
    Zs = F.conv2d(torch.ones_like(x), w_sub, None, padding=1)
    return _grad(Ys, xr, safe_divide(R, Zs)).detach()


def bounded_conv(x, w, R, low, high, dtype):
    """RR:411-441 (the sign masks of RR:392-393: > 0 and < 0)."""
    wp, wn = w * (w > 0).to(dtype), w * (w < 0).to(dtype)
    xr = x.detach().requires_grad_(True)
    lo = (x * 0 + low).detach().requires_grad_(True)
    hi = (x * 0 + high).detach().requires_grad_(True)
    A = F.conv2d(xr, w, None, padding=1)
    B = F.conv2d(lo, wp, None, padding=1)
    Cc = F.conv2d(hi, wn, None, padding=1)
    S = safe_divide(R, (A - (B + Cc)).detach())
    return (xr * _grad(A, xr, S) - (lo * _grad(B, lo, S) + hi * _grad(Cc, hi, S))).detach()


def bounded_denominator(x, w, low, high, dtype):
    """Zs of RR:420-424."""
    wp, wn = w * (w > 0).to(dtype), w * (w < 0).to(dtype)
    return F.conv2d(x, w, None, padding=1) - (F.conv2d(x * 0 + low, wp, None, padding=1) + F.conv2d(x * 0 + high, wn, None, padding=1))


def rule_conv(x, W_hwio, b, R, rule, dtype):
    w, bias = _w_oihw(W_hwio, dtype), _t(b, dtype)
    kind = rule[0]
    if kind == "alphabeta":
        return alphabeta_conv(x, w, bias, R, rule[1], rule[2], rule[3] if len(rule) > 3 else True, dtype)
    if kind == "epsilon":
        return epsilon_conv(x, w, bias, R, rule[1], rule[2] if len(rule) > 2 else True, dtype)
    if kind == "flat":
        return wsquare_conv(x, torch.ones_like(w), R)
    if kind == "wsquare":
        return wsquare_conv(x, w * w, R)
    if kind == "bounded":
        return bounded_conv(x, w, R, rule[1], rule[2], dtype)
    raise ValueError(rule)


def analyze(layers, X_nhwc, R_nhwc, table, dtype=torch.float64):
    """`LRP(model, rule=table[1:], input_layer_rule=table[0]).analyze([X, R])`: conv i by table[i] (input layer first), max-pools
    by gradient routing."""
    _, inputs = forward(layers, X_nhwc, dtype, return_inputs=True)
    R = _nchw(_t(R_nhwc, dtype))
    rules = [r for r in table]
    assert len(rules) == sum(1 for L in layers if L[0] == "conv")
    for L, x in zip(reversed(layers), reversed(inputs)):
        if L[0] == "conv":
            R = rule_conv(x, L[1], L[2], R, rules.pop(), dtype)      # RA:413-415: popped from the end, walking in reverse
        else:
            R = gradient_route(x, lambda v: F.max_pool2d(v, 2, 2), R)
    return _nhwc(R).numpy()


def min_abs_denominator(layers, X_nhwc, table, dtype=torch.float64):
    """smallest |denominator| a rule of `table` divides by, over every unit of every conv (conditioning of a draw); the
    epsilon kinds: over the units whose ReLU is on (relevance arrives nowhere else) of the layers below the top"""
    _, inputs = forward(layers, X_nhwc, dtype, return_inputs=True)
    convs = [(L, x) for L, x in zip(layers, inputs) if L[0] == "conv"]
    worst = np.inf
    for i, ((L, x), rule) in enumerate(zip(convs, table)):
        w, bias = _w_oihw(L[1], dtype), _t(L[2], dtype)
        wp, wn = w * (w >= 0).to(dtype), w * (w < 0).to(dtype)
        xp, xn = x * (x >= 0).to(dtype), x * (x < 0).to(dtype)
        if rule[0] == "alphabeta":
            bb = bias.view(1, -1, 1, 1) if (rule[3] if len(rule) > 3 else True) else 0.0
            zs = [F.conv2d(xp, wp, padding=1) + F.conv2d(xn, wn, padding=1) + bb]
            if rule[2]:
                zs.append(F.conv2d(xp, wn, padding=1) + F.conv2d(xn, wp, padding=1) + bb)
        elif rule[0] == "epsilon":
            use_bias = rule[2] if len(rule) > 2 else True
            z = F.conv2d(x, w, bias if use_bias else None, padding=1)
            z = z + ((z >= 0).to(dtype) * 2 - 1) * rule[1]
            if i + 1 < len(convs):
                z = z[F.conv2d(x, w, bias, padding=1) > 0]
            zs = [z]
        elif rule[0] == "bounded":
            zs = [bounded_denominator(x, w, rule[1], rule[2], dtype)]
        else:
            ws = torch.ones_like(w) if rule[0] == "flat" else w * w
            zs = [F.conv2d(torch.ones_like(x), ws, None, padding=1)]
        worst = min([worst] + [float(z.abs().min()) for z in zs if z.numel()])
    return worst


def op_conv_rule_ref(chains, w_hwio, coef, gates, pool, dtype=torch.float64):
    """lrp_op_conv_rule in torch (NHWC tensors in, NHWC out): c = sum_j convT(chains[j], p_j w+ + q_j w-), 2x2 nearest with pool;
    [c g for g in gates]."""
    w = torch.as_tensor(np.ascontiguousarray(w_hwio)).to(chains[0].device, dtype).permute(3, 2, 0, 1).contiguous()     # (Cout, Cin, 3, 3)
    wp, wn = w * (w >= 0).to(dtype), w * (w < 0).to(dtype)
    c = sum(F.conv_transpose2d(_nchw(s.to(dtype)), wp * p + wn * q, padding=1) for s, (p, q) in zip(chains, coef))
    if pool:
        c = F.interpolate(c, scale_factor=2, mode="nearest")
    c = _nhwc(c)
    return [c * g.to(dtype) for g in gates]
