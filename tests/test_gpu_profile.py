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
