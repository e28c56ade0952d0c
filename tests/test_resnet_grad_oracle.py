"""Pin the ResNet gradient oracle (tests/resnet_grad_ref.py) on the CPU: its forward is oracle/resnet_lrp_ref's, Gradient is
the derivative (central finite differences inside one linear region), Guided Backprop is the layer-by-layer reversed graph
with the clamp after the fan-out sums; and the argument checks of the gradient analyzers (lrp_imagecaptioning_amd/analyzer.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_grad_ref as RG
from conftest import rel_l1
from gpu_util import NONSQUARE_RESNETS, transpose_spatial
from lrp_imagecaptioning_amd.synthetic import resnet_weights
from oracle import resnet_lrp_ref as RN

TINY = ((4, 2), (8, 2))


def _case(seed, stacks=TINY, stem=8, hw=32, n=2):
    rs = np.random.RandomState(seed)
    w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
    X = rs.uniform(-120, 130, size=(n, hw, hw, 3))
    return rs, w, RN.resnet_spec(stacks, stem=stem), X


@pytest.mark.parametrize("stacks,stem,hw", [(TINY, 8, 32), (((8, 2), (16, 3), (32, 2)), 16, 64)])
def test_forward_equals_lrp_oracle(stacks, stem, hw):
    _, w, spec, X = _case(1, stacks, stem, hw)
    a, b = RG.forward(w, spec, X), RN.forward(w, spec, X)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


def _decisions(w, spec, x):
    """every ReLU sign pattern and pool arg-max of the forward at x (N,3,H,W): what fixes the linear region"""
    out = []
    relu = lambda v: (out.append((v > 0).numpy().copy()), F.relu(v))[1]
    y = RG.conv_bn(w, "conv1", F.pad(x, (3, 3, 3, 3)), 2, 0, torch.float64)
    ap = F.pad(relu(y), (1, 1, 1, 1))
    _, idx = F.max_pool2d(ap, 3, 2, return_indices=True)
    out.append(idx.numpy().copy())
    RG.forward_nchw(w, spec, x, torch.float64, relu)
    return out


@pytest.mark.parametrize("seed", [0, 1])
def test_gradient_equals_finite_differences(seed):
    rs, w, spec, X = _case(seed, n=1)
    feat = RG.forward(w, spec, X)
    head = rs.standard_normal(feat.shape)
    g = RG.gradient_analyze(w, spec, X, head, "gradient")
    assert np.abs(g).sum() > 0

    def f(Xe):
        return float((RG.forward(w, spec, Xe) * head).sum())
    x0 = torch.as_tensor(X).permute(0, 3, 1, 2)
    checked = 0
    for trial in range(12):
        v = np.zeros_like(X)
        if trial < 8:                                   # single pixels ...
            v[0, rs.randint(32), rs.randint(32), rs.randint(3)] = 1.0
        else:                                           # ... and dense directions
            v = rs.standard_normal(X.shape)
        eps = 1e-4
        dp = _decisions(w, spec, x0 + eps * torch.as_tensor(v).permute(0, 3, 1, 2))
        dm = _decisions(w, spec, x0 - eps * torch.as_tensor(v).permute(0, 3, 1, 2))
        if not all(np.array_equal(a, b) for a, b in zip(dp, dm)):
            continue                                    # a ReLU kink / pool tie inside the stencil: not a linear region
        fd = (f(X + eps * v) - f(X - eps * v)) / (2 * eps)
        an = float((g * v).sum())
        scale = max(1e-12, float(np.abs(g).sum()) * 1e-9, abs(an))
        assert abs(fd - an) <= 1e-6 * scale, (trial, fd, an)
        checked += 1
    assert checked >= 8


def _bn_scale(w, name):
    g, v = (np.asarray(w[name + k], dtype=np.float64) for k in ("_bn_gamma", "_bn_var"))
    return torch.as_tensor(g / np.sqrt(v + RN.BN_EPS)).view(1, -1, 1, 1)


def _convT(w, name, g, stride, pad, out_hw):
    """the gradient of conv + BN at its input: convT with W scaled per output channel"""
    W = torch.as_tensor(np.asarray(w[name + "_conv_W"], dtype=np.float64)).permute(3, 2, 0, 1).contiguous()
    op = 0
    if stride > 1:                                   # output_padding restores the rows a strided conv dropped
        op = int(out_hw[0]) - ((g.shape[-2] - 1) * stride - 2 * pad + W.shape[-1])
    return F.conv_transpose2d(g * _bn_scale(w, name), W, stride=stride, padding=pad, output_padding=op)


def _guided_by_hand(w, spec, X, head, clamp_after_sum=True):
    """GuidedBackprop layer by layer on the reversed graph; clamp_after_sum=False clamps every fan-out branch and every pool
    window separately (what the three traps of the issue are about) — only to show that the difference is visible"""
    x = torch.as_tensor(X).permute(0, 3, 1, 2).contiguous()
    rho = F.relu
    y0 = RG.conv_bn(w, "conv1", F.pad(x, (3, 3, 3, 3)), 2, 0, torch.float64)
    a0 = F.relu(y0)
    ap = F.pad(a0, (1, 1, 1, 1))
    t, pidx = F.max_pool2d(ap, 3, 2, return_indices=True)
    blocks = []
    for sname, f, n, s1 in spec["stacks"]:
        for b in range(1, n + 1):
            nm = "%s_block%d" % (sname, b)
            stride = s1 if b == 1 else 1
            sc = RG.conv_bn(w, nm + "_0", t, stride, 0, torch.float64) if b == 1 else t
            a1 = F.relu(RG.conv_bn(w, nm + "_1", t, stride, 0, torch.float64))
            a2 = F.relu(RG.conv_bn(w, nm + "_2", a1, 1, 1, torch.float64))
            o = F.relu(sc + RG.conv_bn(w, nm + "_3", a2, 1, 0, torch.float64))
            blocks.append((nm, stride, b == 1, t.shape[-2:], a1, a2, o))
            t = o
    g = torch.as_tensor(head).permute(0, 3, 1, 2).contiguous()       # arrives at the last block's output ReLU
    for nm, stride, proj, in_hw, a1, a2, o in reversed(blocks):
        G = rho(g) * (o > 0)
        s2 = _convT(w, nm + "_3", G, 1, 0, None)
        s2 = rho(s2) * (a2 > 0)
        s1 = _convT(w, nm + "_2", s2, 1, 1, None)
        s1 = rho(s1) * (a1 > 0)
        main = _convT(w, nm + "_1", s1, stride, 0, in_hw)
        short = _convT(w, nm + "_0", G, stride, 0, in_hw) if proj else G
        if not clamp_after_sum and not (nm == blocks[0][0]):
            main, short = rho(main), rho(short)                      # (wrong: per branch)
        g = main + short                                             # the fan-out sum; the next block's ReLU clamps it
    # pool: route every window's value to its first arg-max, summed over the overlapping windows, then the stem ReLU
    N, C, Ho, Wo = g.shape
    flat = torch.zeros(N, C, ap.shape[-2] * ap.shape[-1], dtype=g.dtype)
    vals = g.reshape(N, C, -1)
    if not clamp_after_sum:
        vals = rho(vals)                                             # (wrong: per window)
    flat.scatter_add_(2, pidx.reshape(N, C, -1), vals)
    ga0 = flat.reshape(ap.shape)[:, :, 1:-1, 1:-1]
    S = rho(ga0) * (a0 > 0)
    gx = _convT(w, "conv1", S, 2, 0, (X.shape[1] + 6, X.shape[2] + 6))
    return gx[:, :, 3:-3, 3:-3].permute(0, 2, 3, 1).contiguous().numpy()


@pytest.mark.parametrize("seed", [0, 3])
def test_guided_backprop_equals_layer_by_layer_walk(seed):
    rs, w, spec, X = _case(seed)
    feat = RG.forward(w, spec, X)
    head = rs.standard_normal(feat.shape)
    auto = RG.gradient_analyze(w, spec, X, head, "guided_backprop")
    hand = _guided_by_hand(w, spec, X, head)
    assert np.abs(hand).sum() > 0
    assert rel_l1(auto, hand) < 1e-12
    # the clamp placement matters on this net: clamping per branch / per window is visibly different
    assert rel_l1(_guided_by_hand(w, spec, X, head, clamp_after_sum=False), hand) > 1e-3
    # plain gradient and Input x Gradient through the same hand walk without the clamps
    grad = RG.gradient_analyze(w, spec, X, head, "gradient")
    ixg = RG.gradient_analyze(w, spec, X, head, "input_x_gradient")
    np.testing.assert_allclose(ixg, grad * X, rtol=1e-12, atol=0)
    assert rel_l1(grad, auto) > 1e-3


def test_analyzer_argument_validation():
    """gradient_based.py:110-112 and base.py:332-333 / :489-492: bad arguments raise before any device work"""
    from lrp_imagecaptioning_amd import analyzer as A
    _, w, _, _ = _case(0)
    spec = A.ImageModelSpec(w, img_hw=(32, 32), resnet={"stem": 8, "stacks": TINY})
    assert spec.output_shape() == (4, 4, 32)
    for bad in ("sqrt", "", 1):
        with pytest.raises(ValueError):
            A.Gradient(spec, postprocess=bad)
        with pytest.raises(ValueError):
            A.InputTimesGradient(spec, postprocess=bad)
    for cls in (A.Gradient, A.InputTimesGradient, A.GuidedBackprop):
        with pytest.raises(ValueError):
            cls(spec, neuron_selection_mode="nope")
        with pytest.raises(NotImplementedError):
            cls(spec, neuron_selection_mode="max_activation")
    with pytest.raises(TypeError):
        A.GuidedBackprop(spec, postprocess="abs")                 # (not an argument of GuidedBackprop, :243)
    w2 = dict(w)
    del w2["conv2_block1_2_bn_var"]
    with pytest.raises(A.NotAnalyzeableModelException):
        A.ImageModelSpec(w2, img_hw=(32, 32), resnet={"stem": 8, "stacks": TINY})


@pytest.mark.parametrize("name", ["stem64", "mid", "tiny"])
def test_gradient_walks_are_transposition_equivariant_at_h_ne_w(name):
    """The gradient oracle at H != W: kernels, image and head transposed in their spatial axes -> the transposed map, for
    all three walks (1e-12: only the summation order differs); with the stem kernel alone transposed the map moves by more
    than half its own mass (symmetric inputs would give 1e-12; guided backprop's maps, rectified at every layer, stay
    correlated and land just under 1, the other two walks above it)."""
    stacks, stem, (H, W) = NONSQUARE_RESNETS[name]
    rs = np.random.RandomState(3)
    w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
    spec = RN.resnet_spec(stacks, stem=stem)
    X = rs.uniform(-120, 130, size=(2, H, W, 3))
    feat = RG.forward(w, spec, X)
    head = rs.standard_normal(feat.shape)
    wt, Xt, ht = transpose_spatial(w), np.swapaxes(X, 1, 2), np.swapaxes(head, 1, 2)
    assert rel_l1(np.swapaxes(RG.forward(wt, spec, Xt), 1, 2), feat) < 1e-12
    only_stem = dict(w, conv1_conv_W=wt["conv1_conv_W"])
    for walk in ("gradient", "input_x_gradient", "guided_backprop"):
        ref = RG.gradient_analyze(w, spec, X, head, walk)
        assert np.abs(ref).sum() > 0
        assert rel_l1(np.swapaxes(RG.gradient_analyze(wt, spec, Xt, ht, walk), 1, 2), ref) < 1e-12, walk
        assert rel_l1(RG.gradient_analyze(only_stem, spec, X, head, walk), ref) > 0.5, walk
