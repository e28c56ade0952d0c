"""Test helper (not a test module): restatements for the Deconvnet walk and the augment / reduce wrappers.

  * deconvnet_vgg        oracle.cnn_lrp_ref.gradient_analyze's loop with DeconvnetReverseReLULayer (gradient_based.py:180-196):
                         g = relu(g), then the gradient of the conv WITHOUT its ReLU; pools by gradient routing
  * deconvnet_resnet     tests/resnet_grad_ref.forward_nchw with a `relu=` autograd Function whose backward is relu(grad)
  * python_based_*       literal numpy transcriptions of _python_based_augment / _python_based_reduce of AugmentReduceBase,
                         GaussianSmoother (the noise passed in) and PathIntegrator (innvestigate/analyzer/wrapper.py:168-174, :221-225, :261-296)
  * philox4x32_10, gaussian_noise   the generator of lrp_op_augment_gaussian in numpy integers and float64
"""
import numpy as np
import torch
import torch.nn.functional as F

import resnet_grad_ref as RG
from oracle import cnn_lrp_ref as C


# ---------------------------------------------------------------------------------------------------------- Deconvnet
def deconvnet_vgg(layers, X_nhwc, head_nhwc, dtype=torch.float64, drop_zero_windows=False):
    """`Deconvnet(image_model, neuron_selection_mode="replace").analyze([X, head])` on a vgg_layers list.
    drop_zero_windows: discard what is routed through pool windows whose inputs are all zero (what a walk that lost the
    position of such windows computes) — for the tests' own check that a draw exercises them."""
    _, inputs = C.forward(layers, X_nhwc, dtype, return_inputs=True)
    g = C._nchw(C._t(head_nhwc, dtype))
    for L, x in zip(reversed(layers), reversed(inputs)):
        if L[0] == "conv":
            g = F.relu(g)
            w, b = C._w_oihw(L[1], dtype), C._t(L[2], dtype)
            g = C.gradient_route(x, lambda v: F.conv2d(v, w, b, padding=1), g)
        else:
            if drop_zero_windows:
                g = g * (F.max_pool2d(x, 2, 2) != 0).to(dtype)
            g = C.gradient_route(x, lambda v: F.max_pool2d(v, 2, 2), g)
    return C._nhwc(g).numpy()


class DeconvReLU(torch.autograd.Function):
    """forward relu(x); backward relu(grad): the forward decision is not read"""
    @staticmethod
    def forward(ctx, x):
        return x.clamp(min=0)

    @staticmethod
    def backward(ctx, g):
        return F.relu(g)


def _forward_nchw_drop(w, spec, x, dtype):
    """RG.forward_nchw with DeconvReLU, and the stem pool's all-zero windows cut out of the graph"""
    y = RG.conv_bn(w, "conv1", F.pad(x, (3, 3, 3, 3)), 2, 0, dtype)
    t = F.max_pool2d(F.pad(DeconvReLU.apply(y), (1, 1, 1, 1)), 3, 2)
    t = t * (t.detach() != 0).to(dtype)
    for sname, f, n, s1 in spec["stacks"]:
        for b in range(1, n + 1):
            nm = "%s_block%d" % (sname, b)
            stride = s1 if b == 1 else 1
            sc = RG.conv_bn(w, nm + "_0", t, stride, 0, dtype) if b == 1 else t
            a1 = DeconvReLU.apply(RG.conv_bn(w, nm + "_1", t, stride, 0, dtype))
            a2 = DeconvReLU.apply(RG.conv_bn(w, nm + "_2", a1, 1, 1, dtype))
            t = DeconvReLU.apply(sc + RG.conv_bn(w, nm + "_3", a2, 1, 0, dtype))
    return t


def deconvnet_resnet(w, spec, X_nhwc, head_nhwc, dtype=torch.float64, drop_zero_windows=False):
    x = RG._t(X_nhwc, dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    out = _forward_nchw_drop(w, spec, x, dtype) if drop_zero_windows else RG.forward_nchw(w, spec, x, dtype, DeconvReLU.apply)
    g, = torch.autograd.grad(out, x, grad_outputs=RG._t(head_nhwc, dtype).permute(0, 3, 1, 2).contiguous())
    return g.detach().permute(0, 2, 3, 1).contiguous().numpy()


def single_thread_float32(fn, *args, **kw):
    """fn(..., dtype=torch.float32) on one thread with torch's own conv kernels: a figure that does not move with the host's
    thread count (test_gpu_resnet_alphabeta._literal_float32)."""
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.backends.mkldnn.flags(enabled=False):
            return fn(*args, dtype=torch.float32, **kw)
    finally:
        torch.set_num_threads(nt)


# ---------------------------------------------------------------------------------------------------------- wrappers
def python_based_augment_base(x, n):
    return np.repeat(x, n, axis=0)                                            # wrapper.py:168-169


def python_based_reduce_base(x, n):
    return x.reshape((-1, n) + x.shape[1:]).mean(axis=1)                      # wrapper.py:171-174


def python_based_augment_gaussian(x, n, noise):
    """wrapper.py:221-225 with the draw `np.random.normal(0, noise_scale, size)` handed in as `noise`"""
    return python_based_augment_base(x, n) + noise


def python_based_augment_path(x, n, reference, standard=False):
    """wrapper.py:261-288 (standard=False: literally; True: the published path from the reference to x)"""
    x = np.asarray(x)
    difference = x - reference
    tmp = python_based_augment_base(x, n)
    tmp = tmp.reshape((-1, n) + tmp.shape[1:])
    difference = difference.reshape((-1, 1) + difference.shape[1:])
    alpha = (np.arange(n).astype(x.dtype) / np.asarray(n, x.dtype)).reshape((1, n) + tuple(np.ones_like(difference.shape[2:])))
    path_steps = alpha * difference
    ret = (tmp - difference if standard else tmp) + path_steps
    return ret.reshape((-1,) + ret.shape[2:])


def python_based_reduce_path(maps, n, x, reference):
    return python_based_reduce_base(maps, n) * (x - reference)               # wrapper.py:290-296


# ---------------------------------------------------------------------------------------------------------- generator
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """ctr (..., 4), key (..., 2) uint32 -> (..., 4) uint32 (Salmon et al., Random123's philox4x32 with 10 rounds)"""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(W0)) & m32, (k[1] + np.uint64(W1)) & m32]
    return np.stack(c, axis=-1).astype(np.uint32)


def gaussian_noise(seed, rows, per_image):
    """N(seed, r, i) for r in rows, i in [0, per_image) as float64: key = the seed's halves, counter = (group lo, group hi, r, 0)
    with group = i / 4, u = ((x >> 8) + 0.5) 2^-24, Box-Muller on (x0, x1) and (x2, x3)."""
    rows = np.asarray(rows, dtype=np.uint64)
    groups = np.arange((per_image + 3) // 4, dtype=np.uint64)
    ctr = np.zeros((len(rows), len(groups), 4), dtype=np.uint64)
    ctr[..., 0] = groups[None, :] & np.uint64(0xFFFFFFFF)
    ctr[..., 1] = groups[None, :] >> np.uint64(32)
    ctr[..., 2] = rows[:, None]
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    x = philox4x32_10(ctr, np.broadcast_to(key, ctr.shape[:-1] + (2,)))
    u = ((x >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    rad0, rad1 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    z = np.stack([rad0 * np.cos(2 * np.pi * u[..., 1]), rad0 * np.sin(2 * np.pi * u[..., 1]),
                  rad1 * np.cos(2 * np.pi * u[..., 3]), rad1 * np.sin(2 * np.pi * u[..., 3])], axis=-1)
    return z.reshape(len(rows), -1)[:, :per_image]
