"""Test helper (not a test module): float64 torch restatement of the ResNet-v1 forward of oracle/resnet_lrp_ref.py
(ZeroPad(3), 7x7/2 conv, BN, ReLU, ZeroPad(1), 3x3/2 max-pool; bottleneck blocks conv+BN(+ReLU) x3, optional projection
conv+BN, Add, ReLU), same spec (`resnet_spec`) and weight names, differentiated by autograd:

    gradient_analyze(w, spec, X, head, mode) == <Analyzer>(image_model, neuron_selection_mode="replace").analyze([X, head])

for innvestigate.analyzer.gradient_based Gradient (:101), InputTimesGradient (:154) and GuidedBackprop (:228-265).
Guided backprop replaces every ReLU layer (an Activation layer of the Keras graph; the convs have none) by a function whose
backward is relu(g) * [x > 0]: autograd hands a node the SUM of what its consumers sent back before calling its backward, so
the clamp acts on the completed fan-out sum of a block input and on the sum over the overlapping pool windows at the stem,
like the reversed Keras graph.  torch's max-pool backward routes to the first arg-max of a window and ReLU's gradient at 0
is 0, as in TensorFlow."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.resnet_lrp_ref import BN_EPS, resnet_spec  # noqa: F401  (re-exported: the spec every caller builds)


class GuidedReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return x.clamp(min=0)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return F.relu(g) * (x > 0).to(g.dtype)


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype)


def conv_bn(w, name, x, stride, pad, dtype):
    W = _t(w[name + "_conv_W"], dtype).permute(3, 2, 0, 1).contiguous()
    c = F.conv2d(x, W, _t(w[name + "_conv_b"], dtype), stride=stride, padding=pad)
    g, b, mu, var = (_t(w[name + "_bn_" + k], dtype).view(1, -1, 1, 1) for k in ("gamma", "beta", "mean", "var"))
    return g * (c - mu) / torch.sqrt(var + BN_EPS) + b


def forward_nchw(w, spec, x, dtype=torch.float64, relu=F.relu):
    """x (N,3,H,W) -> conv5_block3_out (N,C,h,w); `relu` is applied at every ReLU layer."""
    y = conv_bn(w, "conv1", F.pad(x, (3, 3, 3, 3)), 2, 0, dtype)
    t = F.max_pool2d(F.pad(relu(y), (1, 1, 1, 1)), 3, 2)
    for sname, f, n, s1 in spec["stacks"]:
        for b in range(1, n + 1):
            nm = "%s_block%d" % (sname, b)
            stride = s1 if b == 1 else 1
            sc = conv_bn(w, nm + "_0", t, stride, 0, dtype) if b == 1 else t
            a1 = relu(conv_bn(w, nm + "_1", t, stride, 0, dtype))
            a2 = relu(conv_bn(w, nm + "_2", a1, 1, 1, dtype))
            t = relu(sc + conv_bn(w, nm + "_3", a2, 1, 0, dtype))
    return t


def forward(w, spec, X_nhwc, dtype=torch.float64):
    x = _t(X_nhwc, dtype).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        return forward_nchw(w, spec, x, dtype).permute(0, 2, 3, 1).contiguous().numpy()


def gradient_analyze(w, spec, X_nhwc, head_nhwc, mode="gradient", dtype=torch.float64):
    """(N,H,W,3), (N,h,w,C) -> (N,H,W,3): 'gradient' | 'input_x_gradient' | 'guided_backprop'."""
    if mode not in ("gradient", "input_x_gradient", "guided_backprop"):
        raise ValueError(mode)
    x = _t(X_nhwc, dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    relu = GuidedReLU.apply if mode == "guided_backprop" else F.relu
    out = forward_nchw(w, spec, x, dtype, relu)
    g, = torch.autograd.grad(out, x, grad_outputs=_t(head_nhwc, dtype).permute(0, 3, 1, 2).contiguous())
    if mode == "input_x_gradient":
        g = g * x
    return g.detach().permute(0, 2, 3, 1).contiguous().numpy()
