"""The draws of the pattern tests, computed once per process and never written to: tests/test_pattern_ref.py checks their
conditions on the CPU, tests/test_gpu_pattern.py runs the device on them.

Fit draws: dyadic weights and integer images (deeplift_ref.dyadic_vgg_weights) — the float32 and float64 forwards agree bit for
bit, so every mask is the same in any arithmetic and a float32 fit differs from float64 by summation error alone.
Walk draws: Gaussian weights, pixels in [-120, 130], patterns from the float64 'relu' fit of six such images."""
import functools

import numpy as np
import torch

import deeplift_ref as DL
import gradient_family_ref as GF
import pattern_ref as PR
import rule_table_cases as K
from lrp_imagecaptioning_amd.synthetic import vgg_weights
from oracle import cnn_lrp_ref as C

FIVE_CFG = [("c1", 3, 16, False), ("c2", 16, 16, True), ("c3", 16, 32, False), ("c4", 32, 32, True), ("c5", 32, 64, False)]
FIT_DRAWS = (("tiny", 1), ("tiny", 2), ("five", 2))
FIT_TYPES = ("linear", "relu", "relu.negative")
WALK_SEEDS = (1, 2, 3)
HW = 16


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def fit_draw(net, seed):
    cfg = K.TINY_CFG if net == "tiny" else FIVE_CFG
    rs = np.random.RandomState(seed)
    w = DL.dyadic_vgg_weights(rs, cfg)
    X = _ro(rs.randint(-4, 5, size=(6, HW, HW, 3)).astype(np.float32))
    return dict(cfg=cfg, w=w, layers=C.vgg_layers(w, cfg), X=X)


@functools.lru_cache(maxsize=None)
def fit_refs(net, seed, pattern_type):
    """float64 sums of the whole draw (with the sums of absolute terms), float64 patterns, and the float32 restatement's patterns
    by running means over the batches 3 + 3"""
    d = fit_draw(net, seed)
    sums = PR.fit_sums(d["layers"], d["X"], pattern_type, with_abs=True)
    pats = [PR.compute_pattern(L[1], s) for L, s in zip(PR.conv_entries(d["layers"]), sums)]
    pats32 = GF.single_thread_float32(lambda dtype: PR.fit_running(d["layers"], d["X"], pattern_type, 3, dtype))
    return dict(sums=sums, patterns=pats, patterns32=pats32)


@functools.lru_cache(maxsize=None)
def walk_draw(seed):
    """the five-conv net, 3 images, 6 heads crossing images; patterns: float64 'relu' fit of 6 further images of the same kind"""
    rs = np.random.RandomState(seed)
    w = vgg_weights(rs, FIVE_CFG, bias_std=0.05)
    layers = C.vgg_layers(w, FIVE_CFG)
    X = _ro(rs.uniform(-120, 130, size=(3, HW, HW, 3)).astype(np.float32))
    idx = (0, 1, 2, 2, 0, 1)
    head = _ro(rs.standard_normal((6, 4, 4, 64)).astype(np.float32))
    Xfit = _ro(rs.uniform(-120, 130, size=(6, HW, HW, 3)).astype(np.float32))
    pats = [_ro(p.astype(np.float32)) for p in PR.fit(layers, Xfit, "relu")]
    pats32 = GF.single_thread_float32(lambda dtype: PR.fit_running(layers, Xfit, "relu", 3, dtype))
    pats64 = PR.fit(layers, Xfit, "relu")
    return dict(w=w, layers=layers, X=X, idx=idx, head=head, Xfit=Xfit, patterns=pats, fit32=pats32, fit64=pats64)


@functools.lru_cache(maxsize=None)
def walk_refs(seed, attribution, projection):
    """(float64, float32) restatement of the walk on the draw's rows, with the float32-rounded patterns the device is given"""
    d = walk_draw(seed)
    Xi = d["X"][list(d["idx"])]
    r64 = PR.walk(d["layers"], Xi, d["head"], d["patterns"], attribution, projection)
    r32 = GF.single_thread_float32(lambda dtype: PR.walk(d["layers"], Xi, d["head"], d["patterns"], attribution, projection, dtype))
    return _ro(r64), _ro(r32)


def rel_l1(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).sum() / max(np.abs(b).sum(), 1e-300))
