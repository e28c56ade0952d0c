"""Test helper: CPU restatements of the ResNet encoder's LRP walk under a rule PAIR (lrp_set_resnet_rules) — one
record for the stem conv (the conv with 3 input channels) and one for every other conv; BatchNormalization, Add, pools and pads
reversed as in oracle.resnet_lrp_ref whatever the pair.  A record is what analyzer.normalize_rule returns (tests/rule_table_ref.py).

  analyze         (a) the literal reverse walk: the tape of oracle.resnet_lrp_ref._Tape, interpreted as tests/resnet_ab_ref.analyze
                  interprets it, with the conv step dispatched on the record — stride- and pad-aware forms of the steps of
                  tests/rule_table_ref.py, one autograd call per GradientWRT of the published graph.  float64 is the reference of
                  the GPU tests, float32 the same graph in the arithmetic the reference runs in (the tests' own error bar).
  analyze_cached  (b) the algorithm of the HIP path (csrc/resnet_encoder.h rule_gates, explain, explain_ab, stem_end), float64:
                  relevance R at y = BN(c) of a unit reaches its input as m . convT(R Bn / D, M), with
                      Bn = c (y - beta_bn) / stab((c - mu) y)
                      rule                D                                    M                     m
                      alpha-beta          safe(Za - [nobias] b), safe(Zi - ..)  alpha w+ ; -beta w-   x
                      epsilon             stab_eps(c - [nobias] b)              w                     x
                      flat (stem)         147                                   1                     1
                      w-square (stem)     sum of w^2 over the 147 taps          w^2                   1
                      bounded (stem)      (c - b) - low sum(w+) - high sum(w-)  w+ ; w-               (x - low) ; (x - high)
                  The stem is a valid conv over the explicitly padded image: all 147 taps count at every output pixel, and what
                  is sent to pad cells is cropped away."""
import torch
import torch.nn.functional as F

from oracle import resnet_lrp_ref as RN
from oracle.cnn_lrp_ref import SAFE_EPS, safe_divide


def _grad(Z, x, S):
    g, = torch.autograd.grad(Z, x, grad_outputs=S)
    return g


def _bias_of(rule):
    if rule[0] == "alphabeta":
        return rule[3] if len(rule) > 3 else True
    if rule[0] == "epsilon":
        return rule[2] if len(rule) > 2 else True
    return False


def rule_conv(x, W, b, stride, pad, R, rule, dtype):
    """One Conv2D (NCHW tensors, OIHW kernel) under `rule`: relevance_rule.py:74-441."""
    kw = dict(stride=stride, padding=pad)
    kind = rule[0]
    if kind == "alphabeta":                                # RR:274-322; IgnoreBias: RR:251-258
        alpha, beta, use_bias = rule[1], rule[2], _bias_of(rule)
        wp, wn = W * (W >= 0).to(dtype), W * (W < 0).to(dtype)
        bp = b * (b >= 0).to(dtype) if use_bias else None
        bn = b * (b < 0).to(dtype) if use_bias else None
        xp, xn = x * (x >= 0).to(dtype), x * (x < 0).to(dtype)

        def f(w1, b1, w2, b2):
            x1, x2 = xp.detach().requires_grad_(True), xn.detach().requires_grad_(True)
            Z1, Z2 = F.conv2d(x1, w1, b1, **kw), F.conv2d(x2, w2, b2, **kw)
            S = safe_divide(R, (Z1 + Z2).detach())
            return (x1 * _grad(Z1, x1, S) + x2 * _grad(Z2, x2, S)).detach()

        act = f(wp, bp, wn, bn)
        return act if not beta else act * alpha - f(wn, bn, wp, bp) * beta
    if kind == "epsilon":                                  # RR:85-98 (eps = 0) / RR:128-144
        eps = rule[1]
        xr = x.detach().requires_grad_(True)
        Z = F.conv2d(xr, W, b if _bias_of(rule) else None, **kw)
        Zd = Z.detach()
        S = safe_divide(R, Zd) if not eps else R / (Zd + ((Zd >= 0).to(dtype) * 2 - 1) * eps)
        return (xr * _grad(Z, xr, S)).detach()
    if kind in ("flat", "wsquare"):                        # RR:174-187 / RR:192-211
        ws = torch.ones_like(W) if kind == "flat" else W * W
        xr = x.detach().requires_grad_(True)
        Ys = F.conv2d(xr, ws, None, **kw)
        Zs = F.conv2d(torch.ones_like(x), ws, None, **kw)
        return _grad(Ys, xr, safe_divide(R, Zs)).detach()
    if kind == "bounded":                                  # RR:411-441
        low, high = rule[1], rule[2]
        wp, wn = W * (W > 0).to(dtype), W * (W < 0).to(dtype)
        xr = x.detach().requires_grad_(True)
        lo = (x * 0 + low).detach().requires_grad_(True)
        hi = (x * 0 + high).detach().requires_grad_(True)
        A, Bc, Cc = F.conv2d(xr, W, None, **kw), F.conv2d(lo, wp, None, **kw), F.conv2d(hi, wn, None, **kw)
        S = safe_divide(R, (A - (Bc + Cc)).detach())
        return (xr * _grad(A, xr, S) - (lo * _grad(Bc, lo, S) + hi * _grad(Cc, hi, S))).detach()
    raise ValueError(rule)


def analyze(w, spec, X_nhwc, R_nhwc, stem_rule, unit_rule, dtype=torch.float64):
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
            R = rule_conv(x, W, b, stride, pad, R, stem_rule if W.shape[1] == 3 else unit_rule, dtype)
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


def analyze_cached(w, spec, X_nhwc, R_nhwc, stem_rule, unit_rule, dtype=torch.float64):
    """(b): gates per unit from c, Za, Zi and per-channel constants; one or two chains per tensor."""
    x = RN._t(X_nhwc, dtype).permute(0, 3, 1, 2).contiguous()

    def stab(d):
        return d + ((d >= 0).to(dtype) * 2 - 1) * SAFE_EPS

    def safe(z):
        return z + (z == 0) * SAFE_EPS

    def stab_eps(z, eps):
        return z + ((z >= 0).to(dtype) * 2 - 1) * eps if eps else safe(z)

    def unit(t_in, name, stride, pad, rule, signed=False):
        """-> y, [(gate Bn / D, matrix M)] per chain"""
        W, b = RN._w(w[name + "_conv_W"], dtype), RN._t(w[name + "_conv_b"], dtype)
        bv = b.view(1, -1, 1, 1)
        kw = dict(stride=stride, padding=pad)
        wp, wn = W * (W >= 0), W * (W < 0)
        c = F.conv2d(t_in, W, b, **kw)
        y = RN._bn(c, w, name, dtype)
        bt = RN._t(w[name + "_bn_beta"], dtype).view(1, -1, 1, 1)
        mu = RN._t(w[name + "_bn_mean"], dtype).view(1, -1, 1, 1)
        Bn = safe_divide(c * (y - bt), stab((c - mu) * y))
        nb = 0.0 if _bias_of(rule) else bv
        kind = rule[0]
        if kind == "alphabeta":
            tp, tn = (t_in * (t_in >= 0), t_in * (t_in < 0)) if signed else (t_in, t_in * 0)
            Za = F.conv2d(tp, wp, None, **kw) + F.conv2d(tn, wn, b, **kw)      # both with the full bias, as the forward makes them
            chains = [(Bn / safe(Za - nb), (rule[1] * wp, rule[1] * wn))]
            if rule[2]:
                Zi = F.conv2d(tp, wn, None, **kw) + F.conv2d(tn, wp, b, **kw)
                chains.append((Bn / safe(Zi - nb), (-rule[2] * wn, -rule[2] * wp)))
            return y, chains
        if kind == "epsilon":
            return y, [(Bn / stab_eps(c - nb, rule[1]), W)]
        ones = torch.ones_like(Bn)
        if kind == "flat":
            return y, [(Bn / (147.0 * ones), torch.ones_like(W))]
        if kind == "wsquare":
            return y, [(Bn / safe((W * W).sum(dim=(1, 2, 3)).view(1, -1, 1, 1) * ones), W * W)]
        low, high = rule[1], rule[2]
        D = (c - bv) - low * wp.sum(dim=(1, 2, 3)).view(1, -1, 1, 1) - high * wn.sum(dim=(1, 2, 3)).view(1, -1, 1, 1)
        return y, [(Bn / safe(D), (wp, wn))]

    def back(R, chains, **kw):
        """sum over the chains of convT(R gate, M) for x >= 0 (M of alpha-beta: the w+ half)"""
        return sum(F.conv_transpose2d(R * g, M[0] if isinstance(M, tuple) else M, **kw) for g, M in chains)

    xp = F.pad(x, (3, 3, 3, 3))
    y0, stem = unit(xp, "conv1", 2, 0, stem_rule, signed=True)
    ap = F.pad(F.relu(y0), (1, 1, 1, 1))
    t = F.max_pool2d(ap, 3, 2)
    blocks = []
    for sname, f, n, s1 in spec["stacks"]:
        for b in range(1, n + 1):
            nm = "%s_block%d" % (sname, b)
            stride = s1 if b == 1 else 1
            d = {"t": t, "stride": stride, "proj": b == 1}
            if b == 1:
                sc, d["u0"] = unit(t, nm + "_0", stride, 0, unit_rule)
            else:
                sc = t
            y1, d["u1"] = unit(t, nm + "_1", stride, 0, unit_rule)
            a1 = F.relu(y1)
            y2, d["u2"] = unit(a1, nm + "_2", 1, 1, unit_rule)
            a2 = F.relu(y2)
            y3, d["u3"] = unit(a2, nm + "_3", 1, 0, unit_rule)
            den = safe(sc + y3)
            d["fA"], d["fS"], d["a1"], d["a2"] = y3 / den, sc / den, a1, a2
            blocks.append(d)
            t = F.relu(sc + y3)
    R = RN._t(R_nhwc, dtype).permute(0, 3, 1, 2).contiguous()
    for d in reversed(blocks):
        s = d["stride"]
        C3 = back(R * d["fA"], d["u3"])
        C2 = back(C3 * d["a2"], d["u2"], padding=1)
        Rt = d["t"] * back(C2 * d["a1"], d["u1"], stride=s, output_padding=s - 1)
        if d["proj"]:
            Rt = Rt + d["t"] * back(R * d["fS"], d["u0"], stride=s, output_padding=s - 1)
        else:
            Rt = Rt + R * d["fS"]
        R = Rt
    apr = ap.detach().requires_grad_(True)
    g, = torch.autograd.grad(F.max_pool2d(apr, 3, 2), apr, grad_outputs=R)
    Ra0 = g[:, :, 1:-1, 1:-1]
    kw = dict(stride=2, output_padding=1)
    kind = stem_rule[0]
    if kind == "alphabeta":                                # MODE 0: x+ . T+ + x- . T-
        xpp, xpn = xp * (xp >= 0), xp * (xp < 0)
        Rx = sum(xpp * F.conv_transpose2d(Ra0 * g_, M[0], **kw) + xpn * F.conv_transpose2d(Ra0 * g_, M[1], **kw) for g_, M in stem)
    elif kind == "epsilon":                                # MODE 2: x . T+
        Rx = xp * F.conv_transpose2d(Ra0 * stem[0][0], stem[0][1], **kw)
    elif kind == "bounded":                                # MODE 3: (x - low) . T+ + (x - high) . T-
        g_, (wp0, wn0) = stem[0]
        Rx = (xp - stem_rule[1]) * F.conv_transpose2d(Ra0 * g_, wp0, **kw) + (xp - stem_rule[2]) * F.conv_transpose2d(Ra0 * g_, wn0, **kw)
    else:                                                  # MODE 1: T+
        Rx = F.conv_transpose2d(Ra0 * stem[0][0], stem[0][1], **kw)
    return Rx[:, :, 3:-3, 3:-3].permute(0, 2, 3, 1).contiguous().numpy()
