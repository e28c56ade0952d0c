"""-m gpu: the per-launch profile records of the reverse walks (csrc/common.h Profiler; lrp_profile_enable / _query / _records).
One record per conv layer — a folded image layer and a sparse boundary still book exactly one record per layer — with the
layer's algorithmic flops on it; both encoders keep their records in the same Profiler, and both entries read the encoder the
handle was built with."""
import numpy as np
import pytest

from lrp_imagecaptioning_amd.synthetic import resnet_weights, vgg_weights
from test_gpu_cnn import MID_CFG, TINY_CFG, _engine

pytestmark = pytest.mark.gpu


def _walk_flop(cfg, hw, n):
    """sum over the layers li >= 1 of 2 n H W 9 cout cin, plus 2 n H0 W0 9 cout0 6 for the image layer (integers below 2^53)"""
    total, side = 0, hw
    for li, (_, cin, cout, pool) in enumerate(cfg):
        total += 2 * n * side * side * 9 * cout * (6 if li == 0 else cin)
        side = side // 2 if pool else side
    return total


@pytest.mark.parametrize("prec", ["bf16x3", "fp32"])
@pytest.mark.parametrize("name,cfg,hw,B", [("tiny", TINY_CFG, 16, 3), ("mid", MID_CFG, 32, 2)])
def test_vgg_walk_books_one_record_per_layer(name, cfg, hw, B, prec):
    rs = np.random.RandomState(7)
    w = vgg_weights(rs, cfg, bias_std=0.3)
    X = rs.uniform(-120, 130, size=(B, hw, hw, 3)).astype(np.float32)
    n = 2 * B
    eng, side = _engine(cfg, hw, B, n, w)
    eng.set_precision(prec)
    eng.encode_images(X)
    idx = list(range(B)) + list(range(B))[::-1]
    R = rs.standard_normal((n, side * side, cfg[-1][2])).astype(np.float32)
    want = _walk_flop(cfg, hw, n)
    assert want < 2 ** 53
    # off: a walk leaves nothing behind
    eng.cnn_explain(idx, R)
    assert eng.profile_query() == (0, 0.0, 0.0)
    eng.profile_enable(True)
    eng.cnn_explain(idx, R)
    launches, ms, flop = eng.profile_query()
    print(name, prec, launches, ms, flop, want)
    assert launches == len(cfg)
    assert flop == float(want)
    assert ms > 0
    assert eng.profile_query() == (0, 0.0, 0.0)            # the query empties the list
    eng.cnn_explain(idx, R)
    recs = eng.profile_records()
    assert len(recs) == len(cfg)
    assert sum(f for _, f in recs) == float(want)
    eng.profile_enable(False)
    eng.cnn_explain(idx, R)
    assert eng.profile_query() == (0, 0.0, 0.0)


@pytest.mark.parametrize("prec", ["bf16x3", "fp32"])
def test_resnet_walk_books_one_record_per_conv_launch(prec):
    """The `ident` net of test_gpu_resnet_alphabeta.py (one stack of a projection and an identity block, stem 8, 16 x 16), B = 2,
    4 maps: one record per transposed conv through a unit — 4 for the projection block, 3 for the identity block, none for the
    stem's tap GEMM — with 2 n Hout Wout k^2 cout cin on each; the two-chain walk of rule (2, 1) makes the same launches over both
    chains and books twice that on each."""
    from test_gpu_resnet_alphabeta import NETS, _engine as ab_engine
    stacks, stem, (h, wd), _, _ = NETS["ident"]
    assert (stacks, stem, (h, wd)) == (((8, 2),), 8, (16, 16))
    B, n = 2, 4
    rs = np.random.RandomState(5)
    w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
    X = rs.uniform(-120, 130, size=(B, h, wd, 3)).astype(np.float32)
    side, f = h // 4, stacks[0][0]
    # (k, cin, cout) of the units on their side x side output grid: block 1 has the projection shortcut, block 2 has none
    convs = [(1, stem, 4 * f), (1, stem, f), (3, f, f), (1, f, 4 * f), (1, 4 * f, f), (3, f, f), (1, f, 4 * f)]
    want = sum(2 * n * side * side * k * k * cout * cin for k, cin, cout in convs)
    assert want < 2 ** 53
    eng = ab_engine("ident", w, max_images=B, max_tokens=n)
    eng.set_precision(prec)
    idx = [0, 1, 1, 0]
    R = rs.standard_normal((n, side * side, 4 * f)).astype(np.float32)
    for rule, factor in ((None, 1), ((2, 1), 2)):
        if rule:
            eng.set_cnn_rule(*rule)
        eng.encode_images(X)
        eng.profile_enable(True)
        eng.cnn_explain(idx, R)
        launches, ms, flop = eng.profile_query()
        print("resnet ident", prec, rule, launches, ms, flop, factor * want)
        assert launches == len(convs) == 7
        assert flop == float(factor * want)
        assert ms > 0
        eng.cnn_explain(idx, R)
        recs = eng.profile_records()
        assert len(recs) == 7
        assert sum(fl for _, fl in recs) == float(factor * want)
        eng.profile_enable(False)


def test_resnet_handle_reports_its_own_records():
    """lrp_profile_query on a ResNet handle reads the ResNet encoder's records, as lrp_profile_records does: the launch count
    of one walk equals the row count of an identical second walk."""
    from test_gpu_resnet import _engine as resnet_engine
    stacks, stem, hw, B = ((4, 2), (8, 2)), 8, 32, 2
    rs = np.random.RandomState(3)
    w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
    X = rs.uniform(-120, 130, size=(B, hw, hw, 3)).astype(np.float32)
    eng, side, D = resnet_engine(stacks, stem, hw, B, 2 * B, w)
    eng.encode_images(X)
    idx = list(range(B)) + list(range(B))[::-1]
    R = rs.standard_normal((2 * B, side * side, D)).astype(np.float32)
    eng.profile_enable(True)
    eng.cnn_explain(idx, R)
    launches, ms, flop = eng.profile_query()
    print("resnet tiny", launches, ms, flop)
    assert launches > 0 and ms > 0 and flop > 0
    eng.cnn_explain(idx, R)
    assert len(eng.profile_records()) == launches
    assert eng.profile_query() == (0, 0.0, 0.0)
