"""Test helper: the reversed tensors of the reverse analyzers' inspection switches (innvestigate/analyzer/base.py:570-603,
:715-802; utils/keras/graph.py:770-816, :898-940), restated in torch on the walk of tests/rule_table_ref.py.

The encoder is a VGG-style conv list cut at its last conv; its nodes are the convs and 2x2 max-pools in execution order,
nid = 0 .. N-1.  The reversed tensors carry the ids
    (-1, 0)   the head itself (the R the caller passed)
    (nid, 0)  the relevance at the INPUT of node nid, in that tensor's shape; (0, 0) is the image-level result
A pool node's input tensor is at full resolution: the pool's output relevance routed to the arg-max (first in scan order, the
project's convention and torch's), exact zeros elsewhere.

Draws shared with the GPU tests (tests/test_gpu_layer_trace.py) are cached here, computed once and never written to."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import rule_table_cases as K
import rule_table_ref as RT
from oracle.cnn_lrp_ref import _nchw, _nhwc, _t, forward, gradient_route

AB10 = ("alphabeta", 1, 0, True)
# the GPU parity cases: name -> precisions; "default" is the handle's default walk, alpha1beta0 with the bias on every conv
PARITY_TABLES = {"default": ("fp32", "bf16x3"), "presetAflat": ("fp32", "bf16x3"), "presetBflat": ("fp32", "bf16x3"),
                 "a2b1_bounded": ("fp32", "bf16x3"), "mixed_ab": ("fp32", "bf16x3"), "composite": ("fp32",), "z_middle": ("fp32",)}
PARITY_NETS = ("tiny", "mid")


def node_ids(cfg):
    """sorted ids of the reversed tensors of a conv cfg (name, cin, cout, pool_after)"""
    n = sum(2 if pool else 1 for _, _, _, pool in cfg)
    return [(nid, 0) for nid in range(-1, n)]


def analyze_traced(layers, X_nhwc, R_nhwc, table, dtype=torch.float64):
    """rule_table_ref.analyze with every reversed tensor returned: a sorted list of ((nid, 0), ndarray (N, H, W, C))."""
    _, inputs = forward(layers, X_nhwc, dtype, return_inputs=True)
    R = _nchw(_t(R_nhwc, dtype))
    out = {(-1, 0): _nhwc(R).numpy()}
    rules = [r for r in table]
    assert len(rules) == sum(1 for L in layers if L[0] == "conv")
    for nid in range(len(layers) - 1, -1, -1):
        L, x = layers[nid], inputs[nid]
        if L[0] == "conv":
            R = RT.rule_conv(x, L[1], L[2], R, rules.pop(), dtype)
        else:
            R = gradient_route(x, lambda v: F.max_pool2d(v, 2, 2), R)
        out[(nid, 0)] = _nhwc(R).numpy()
    return sorted(out.items())


def table_of(name):
    return (AB10,) * 5 if name == "default" else K.table(name)


def seed_of(name, net_name):
    return K.SEED if name == "default" else K.seed_of(name, net_name)


@functools.lru_cache(maxsize=None)
def refs(net_name, table_name):
    """(float64, float32) reversed tensors of the net's tokens under the table, as dicts id -> read-only ndarray"""
    w, X, idx, R, layers = K.net(net_name, seed=seed_of(table_name, net_name))
    Xi = X[list(idx)]
    t = table_of(table_name)
    r64 = dict(analyze_traced(layers, Xi, R, t))
    r32 = dict(analyze_traced(layers, Xi, R, t, dtype=torch.float32))
    for d in (r64, r32):
        for a in d.values():
            a.setflags(write=False)
    return r64, r32


def rel_l1_rows(out, ref):
    """per row: sum|out - ref| / sum|ref| in float64; a row whose reference is all zero scores 0 if `out` is, inf otherwise"""
    a = np.asarray(out, dtype=np.float64).reshape(len(out), -1)
    b = np.asarray(ref, dtype=np.float64).reshape(len(ref), -1)
    num, den = np.abs(a - b).sum(axis=1), np.abs(b).sum(axis=1)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))
