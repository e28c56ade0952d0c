"""Pin the ResNet oracle (oracle/resnet_lrp_ref.py): the literal reverse walk against the
restructured cached-gate algorithm the HIP path implements, plus hand-checkable pieces."""
import numpy as np
import pytest
import torch

from conftest import rel_l1
from gpu_util import NONSQUARE_RESNETS, transpose_spatial
from lrp_imagecaptioning_amd.synthetic import resnet_conv_list, resnet_weights
from oracle import resnet_lrp_ref as RN

TINY = ((4, 2), (8, 2))


def test_architecture_bookkeeping():
    convs = resnet_conv_list()
    assert len(convs) == 1 + (3 * 3 + 1) + (4 * 3 + 1) + (23 * 3 + 1) + (3 * 3 + 1)        # 104 convs in ResNet-101
    assert convs[0] == ("conv1", 7, 3, 64, 2)
    assert convs[-1] == ("conv5_block3_3", 1, 512, 2048, 1)
    assert ("conv3_block1_0", 1, 256, 512, 2) in convs and ("conv2_block1_1", 1, 64, 64, 1) in convs
    assert RN.conv_names(RN.resnet_spec()) == convs


@pytest.mark.parametrize("seed", [0, 1])
def test_cached_algorithm_equals_literal_walk(seed):
    rs = np.random.RandomState(seed)
    spec = RN.resnet_spec(TINY, stem=8)
    w = resnet_weights(rs, TINY, stem=8, bias_std=0.2)
    X = rs.uniform(-120, 130, size=(2, 32, 32, 3))
    feat = RN.forward(w, spec, X)
    assert feat.shape == (2, 4, 4, 32) and (feat >= 0).all()
    R = rs.standard_normal(feat.shape) * feat
    lit = RN.analyze(w, spec, X, R)
    fast = RN.analyze_cached(w, spec, X, R)
    assert lit.shape == X.shape and np.isfinite(lit).all()
    assert rel_l1(fast, lit) < 1e-10


def test_identity_block_relevance_split():
    """One identity block, hand check of the Add rule: with the main path's last BN forced to
    gamma = 0, beta = 0 the block output equals relu(t) = t and ALL relevance takes the shortcut."""
    rs = np.random.RandomState(3)
    spec = RN.resnet_spec(((4, 2),), stem=8)
    w = resnet_weights(rs, ((4, 2),), stem=8)
    w["conv2_block2_3_bn_gamma"][:] = 0
    w["conv2_block2_3_bn_beta"][:] = 0
    X = rs.uniform(-120, 130, size=(1, 16, 16, 3))
    spec1 = RN.resnet_spec(((4, 1),), stem=8)
    f1 = RN.forward(w, spec1, X)                       # output of block 1
    f2 = RN.forward(w, spec, X)                        # output of block 2 == block 1's output
    np.testing.assert_allclose(f2, f1, rtol=1e-12)
    R = rs.standard_normal(f2.shape) * f2
    np.testing.assert_allclose(RN.analyze(w, spec, X, R), RN.analyze(w, spec1, X, R), rtol=1e-9, atol=1e-12)


def test_float32_close_to_float64():
    rs = np.random.RandomState(5)
    spec = RN.resnet_spec(TINY, stem=8)
    w = resnet_weights(rs, TINY, stem=8)
    X = rs.uniform(-120, 130, size=(1, 32, 32, 3)).astype(np.float32)
    feat = RN.forward(w, spec, X)
    R = (rs.standard_normal(feat.shape) * feat).astype(np.float32)
    assert rel_l1(RN.analyze(w, spec, X, R, torch.float32), RN.analyze(w, spec, X, R)) < 1e-4


@pytest.mark.parametrize("name", ["stem64", "mid", "tiny"])
def test_transposition_equivariance_at_h_ne_w(name):
    """The oracle at H != W: with every kernel transposed in its two spatial axes, the image and the relevance transposed,
    forward and analyze return the transposed result (to summation order: 1e-12) — an H / W mix-up anywhere in it, the
    7 x 7 / 2 stem's padding, the overlapping pool or the stride-2 blocks included, would break this.  Continuous random inputs:
    no pool ties.  Transposing the stem kernel alone moves the map by more than its own mass: the inputs are not
    accidentally symmetric."""
    stacks, stem, (H, W) = NONSQUARE_RESNETS[name]
    rs = np.random.RandomState(3)
    w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
    spec = RN.resnet_spec(stacks, stem=stem)
    X = rs.uniform(-120, 130, size=(2, H, W, 3))
    feat = RN.forward(w, spec, X)
    assert feat.shape[1:3] == (H // 4 // 2 ** (len(stacks) - 1), W // 4 // 2 ** (len(stacks) - 1))
    R = rs.standard_normal(feat.shape) * feat
    ref = RN.analyze(w, spec, X, R)
    wt, Xt, Rt = transpose_spatial(w), np.swapaxes(X, 1, 2), np.swapaxes(R, 1, 2)
    assert rel_l1(np.swapaxes(RN.forward(wt, spec, Xt), 1, 2), feat) < 1e-12
    assert rel_l1(np.swapaxes(RN.analyze(wt, spec, Xt, Rt), 1, 2), ref) < 1e-12
    assert rel_l1(np.swapaxes(RN.analyze_cached(wt, spec, Xt, Rt), 1, 2), ref) < 1e-10
    only_stem = dict(w, conv1_conv_W=wt["conv1_conv_W"])
    assert rel_l1(RN.analyze(only_stem, spec, X, R), ref) > 1.0
