"""Test helper: CPU restatements of AlphaBetaRule (relevance_rule.py:274-322, bias=True) with general (alpha, beta) on the ResNet
encoder — every Conv2D under the rule, BatchNormalization, Add, pools and pads reversed as in oracle.resnet_lrp_ref.

  analyze         (a) the literal reverse walk: the tape of oracle.resnet_lrp_ref._Tape, interpreted as RN.analyze interprets it,
                  with the conv step replaced by a stride- and pad-aware form of alphabeta_ref.alphabeta_conv (one autograd call
                  per GradientWRT of the published graph).  float64 is the reference of the GPU tests, float32 the same graph in
                  the arithmetic the reference runs in (the tests' own error bar).
  analyze_cached  (b) the two-chain algorithm of the HIP path (csrc/resnet_encoder.h explain_ab), float64 on the CPU.  Per conv
                  + BN unit with input x >= 0:  c = conv(x, w) + b, Za = conv(x, w+) + b, Zi = conv(x, w-) + b (BOTH with the full
                  bias: the reference adds b+ and b- in either branch, see alphabeta_ref's docstring), y = BN(c),
                  Bn = c (y - beta_bn) / stab((c - mu) y), Qa = Bn / safe(Za), Qi = Bn / safe(Zi); relevance R at y reaches the
                  input as x [convT(R Qa, alpha w+) + convT(R Qi, -beta w-)].  The stem's input is signed: Za = conv(x+, w+) +
                  conv(x-, w-) + b, Zi = conv(x+, w-) + conv(x-, w+) + b."""
import torch
import torch.nn.functional as F

from oracle import resnet_lrp_ref as RN
from oracle.cnn_lrp_ref import SAFE_EPS, safe_divide


def _branch(x1, x2, w1, b1, w2, b2, R, stride, pad):
    """f(layer1, layer2, X1, X2) of RR:283-303 for a Conv2D with stride and padding."""
    x1 = x1.detach().requires_grad_(True)
    x2 = x2.detach().requires_grad_(True)
    Z1 = F.conv2d(x1, w1, b1, stride=stride, padding=pad)
    Z2 = F.conv2d(x2, w2, b2, stride=stride, padding=pad)
    S = safe_divide(R, (Z1 + Z2).detach())
    g1, = torch.autograd.grad(Z1, x1, grad_outputs=S)
    g2, = torch.autograd.grad(Z2, x2, grad_outputs=S)
    return (x1 * g1 + x2 * g2).detach()


def alphabeta_conv(x, W, b, stride, pad, R, alpha, beta, dtype):
    """RR:274-322 for one Conv2D (NCHW tensors, OIHW kernel)."""
    wp, wn = W * (W >= 0).to(dtype), W * (W < 0).to(dtype)
    bp, bn = b * (b >= 0).to(dtype), b * (b < 0).to(dtype)
    xp, xn = x * (x >= 0).to(dtype), x * (x < 0).to(dtype)
    act = _branch(xp, xn, wp, bp, wn, bn, R, stride, pad)
    if not beta:
        return act
    inh = _branch(xp, xn, wn, bn, wp, bp, R, stride, pad)
    return act * alpha - inh * beta


def analyze(w, spec, X_nhwc, R_nhwc, alpha, beta, dtype=torch.float64):
    """(a): (N,H,W,3), (N,h,w,C) -> (N,H,W,3)."""
    tape = RN._Tape(w, spec, dtype)
    tape.forward(X_nhwc)
    R = RN._t(R_nhwc, dtype).permute(0, 3, 1, 2).contiguous()
    pending = []
    for kind, p in reversed(tape.ops):
        if kind == "add":
            sc, y3, _ = p
            S = safe_divide(R, sc + y3)                               # RA:260-286
            pending.append({"R_sc": sc * S, "R_main": y3 * S, "acc": None})
            R = None
        elif kind == "endbranch":
            R = pending[-1]["R_main"] if p == "main" else pending[-1]["R_sc"]
        elif kind == "branch":
            d = pending[-1]
            d["acc"] = R if d["acc"] is None else d["acc"] + R
            if p == "shortcut":
                d["had_sc_branch"] = True
            R = None
        elif kind == "fork":
            d = pending.pop()
            if not d.get("had_sc_branch"):
                d["acc"] = d["acc"] + d["R_sc"]
            R = d["acc"]                                              # KG:799-803
        elif kind == "conv":
            x, W, b, stride, pad = p
            R = alphabeta_conv(x, W, b, stride, pad, R, alpha, beta, dtype)
        elif kind == "bn":
            x, y, name = p
            R = RN._bn_reverse(x, y, name, tape.w, R, dtype)
        elif kind == "pool":
            ap = p.detach().requires_grad_(True)
            g, = torch.autograd.grad(F.max_pool2d(ap, 3, 2), ap, grad_outputs=R)     # RA:470-480
            R = g.detach()
        elif kind == "pad":
            R = R[:, :, p:-p, p:-p]
    return R.permute(0, 2, 3, 1).contiguous().numpy()


def analyze_cached(w, spec, X_nhwc, R_nhwc, alpha, beta, dtype=torch.float64):
    """(b): the cached two-chain algorithm."""
    x = RN._t(X_nhwc, dtype).permute(0, 3, 1, 2).contiguous()

    def stab(d):
        return d + ((d >= 0).to(dtype) * 2 - 1) * SAFE_EPS

    def safe(z):
        return z + (z == 0) * SAFE_EPS

    def unit(t_in, name, stride, pad, both_signs=False):
        W, b = RN._w(w[name + "_conv_W"], dtype), RN._t(w[name + "_conv_b"], dtype)
        wp, wn = W * (W >= 0), W * (W < 0)
        c = F.conv2d(t_in, W, b, stride=stride, padding=pad)
        if both_signs:
            tp, tn = t_in * (t_in >= 0), t_in * (t_in < 0)
            Za = F.conv2d(tp, wp, None, stride=stride, padding=pad) + F.conv2d(tn, wn, b, stride=stride, padding=pad)
            Zi = F.conv2d(tp, wn, None, stride=stride, padding=pad) + F.conv2d(tn, wp, b, stride=stride, padding=pad)
        else:
            Za = F.conv2d(t_in, wp, b, stride=stride, padding=pad)
            Zi = F.conv2d(t_in, wn, b, stride=stride, padding=pad)
        y = RN._bn(c, w, name, dtype)
        bt = RN._t(w[name + "_bn_beta"], dtype).view(1, -1, 1, 1)
        mu = RN._t(w[name + "_bn_mean"], dtype).view(1, -1, 1, 1)
        Bn = safe_divide(c * (y - bt), stab((c - mu) * y))
        return y, Bn / safe(Za), Bn / safe(Zi), wp, wn

    def back(Sa, Si, wp, wn, **kw):                     # both chains' transposed conv: one GEMM over [alpha w+ ; -beta w-]
        return F.conv_transpose2d(Sa, alpha * wp, **kw) + F.conv_transpose2d(Si, -beta * wn, **kw)

    xp = F.pad(x, (3, 3, 3, 3))
    y0, Q0a, Q0i, wp0, wn0 = unit(xp, "conv1", 2, 0, both_signs=True)
    ap = F.pad(F.relu(y0), (1, 1, 1, 1))
    t = F.max_pool2d(ap, 3, 2)
    blocks = []
    for sname, f, n, s1 in spec["stacks"]:
        for b in range(1, n + 1):
            nm = "%s_block%d" % (sname, b)
            stride = s1 if b == 1 else 1
            d = {"t": t, "stride": stride, "proj": b == 1}
            if b == 1:
                sc, d["Q0a"], d["Q0i"], d["w0p"], d["w0n"] = unit(t, nm + "_0", stride, 0)
            else:
                sc = t
            y1, d["Q1a"], d["Q1i"], d["w1p"], d["w1n"] = unit(t, nm + "_1", stride, 0)
            a1 = F.relu(y1)
            y2, d["Q2a"], d["Q2i"], d["w2p"], d["w2n"] = unit(a1, nm + "_2", 1, 1)
            a2 = F.relu(y2)
            y3, d["Q3a"], d["Q3i"], d["w3p"], d["w3n"] = unit(a2, nm + "_3", 1, 0)
            den = safe(sc + y3)
            d["fA"], d["fS"], d["a1"], d["a2"] = y3 / den, sc / den, a1, a2
            blocks.append(d)
            t = F.relu(sc + y3)
    R = RN._t(R_nhwc, dtype).permute(0, 3, 1, 2).contiguous()
    for d in reversed(blocks):
        s = d["stride"]
        C3 = back(R * d["fA"] * d["Q3a"], R * d["fA"] * d["Q3i"], d["w3p"], d["w3n"])
        C2 = back(C3 * d["a2"] * d["Q2a"], C3 * d["a2"] * d["Q2i"], d["w2p"], d["w2n"], padding=1)
        Rt = d["t"] * back(C2 * d["a1"] * d["Q1a"], C2 * d["a1"] * d["Q1i"], d["w1p"], d["w1n"], stride=s, output_padding=s - 1)
        if d["proj"]:
            Rt = Rt + d["t"] * back(R * d["fS"] * d["Q0a"], R * d["fS"] * d["Q0i"], d["w0p"], d["w0n"], stride=s, output_padding=s - 1)
        else:
            Rt = Rt + R * d["fS"]
        R = Rt
    apr = ap.detach().requires_grad_(True)
    g, = torch.autograd.grad(F.max_pool2d(apr, 3, 2), apr, grad_outputs=R)
    Ra0 = g[:, :, 1:-1, 1:-1]
    Sa, Si = Ra0 * Q0a, Ra0 * Q0i
    kw = dict(stride=2, output_padding=1)
    xpp, xpn = xp * (xp >= 0), xp * (xp < 0)
    Rx = alpha * (xpp * F.conv_transpose2d(Sa, wp0, **kw) + xpn * F.conv_transpose2d(Sa, wn0, **kw)) \
        - beta * (xpp * F.conv_transpose2d(Si, wn0, **kw) + xpn * F.conv_transpose2d(Si, wp0, **kw))
    return Rx[:, :, 3:-3, 3:-3].permute(0, 2, 3, 1).contiguous().numpy()


def min_abs_denominator(w, spec, X_nhwc, dtype=torch.float64):
    """smallest |Za| and |Zi| over every unit of every conv (conditioning of a draw; 0 = a unit none of whose active inputs has a
    weight of that sign: what arrives there is dropped by that branch, RR's SafeDivide)."""
    tape = RN._Tape(w, spec, dtype)
    tape.forward(X_nhwc)
    worst = float("inf")
    for kind, p in tape.ops:
        if kind != "conv":
            continue
        x, W, b, stride, pad = p
        wp, wn = W * (W >= 0).to(dtype), W * (W < 0).to(dtype)
        xp, xn = x * (x >= 0).to(dtype), x * (x < 0).to(dtype)
        za = F.conv2d(xp, wp, b, stride=stride, padding=pad) + F.conv2d(xn, wn, None, stride=stride, padding=pad)
        zi = F.conv2d(xp, wn, b, stride=stride, padding=pad) + F.conv2d(xn, wp, None, stride=stride, padding=pad)
        worst = min(worst, float(za.abs().min()), float(zi.abs().min()))
    return worst
