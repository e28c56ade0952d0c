"""CPU: the restatement of the reversed tensors (tests/layer_trace_ref.py) pinned by hand-computable nets, the condition of the draws
the GPU tests use — per TENSOR now, not only at the image: the float32 restatement within 1e-5 relative L1 of the float64 one
(tests/rule_table_cases.py) — conservation under ZPlus, and the analyzers' argument contract for the reverse_* switches."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_trace_ref as LT
import rule_table_cases as K
import rule_table_ref as RT
from lrp_imagecaptioning_amd import analyzer as A
from lrp_imagecaptioning_amd.synthetic import vgg_weights
from oracle import cnn_lrp_ref as C


def test_one_conv_net_is_the_rule_itself():
    cfg = [("c1", 3, 8, False)]
    rs = np.random.RandomState(3)
    w = vgg_weights(rs, cfg, bias_std=0.3)
    layers = C.vgg_layers(w, cfg)
    X = rs.uniform(-120, 130, size=(2, 6, 5, 3)).astype(np.float32)
    R = rs.standard_normal((2, 6, 5, 8)).astype(np.float32)
    for rule in (LT.AB10, ("alphabeta", 2, 1, False), ("epsilon", 0.25, True), ("flat",), ("bounded", -124.0, 152.0)):
        got = LT.analyze_traced(layers, X, R, [rule])
        assert [i for i, _ in got] == [(-1, 0), (0, 0)] == LT.node_ids(cfg)
        assert np.array_equal(got[0][1], R.astype(np.float64))
        x = C._nchw(C._t(X, torch.float64))
        want = C._nhwc(RT.rule_conv(x, layers[0][1], layers[0][2], C._nchw(C._t(R, torch.float64)), rule, torch.float64)).numpy()
        assert np.array_equal(got[1][1], want)
        assert np.array_equal(got[1][1], RT.analyze(layers, X, R, [rule]))


def test_pool_input_is_the_pool_output_routed_to_the_first_argmax():
    cfg = [("c1", 3, 4, True), ("c2", 4, 4, False)]
    rs = np.random.RandomState(5)
    w = vgg_weights(rs, cfg, bias_std=0.3)
    w["c1_b"] = w["c1_b"] - 40.0                       # many dead units: whole windows of zeros, whose first cell takes the share
    layers = C.vgg_layers(w, cfg)
    X = rs.uniform(-120, 130, size=(2, 8, 6, 3)).astype(np.float32)
    R = rs.standard_normal((2, 4, 3, 4))
    got = dict(LT.analyze_traced(layers, X, R, [LT.AB10, LT.AB10]))
    assert sorted(got) == LT.node_ids(cfg) == [(-1, 0), (0, 0), (1, 0), (2, 0)]
    a1 = C._nhwc(F.relu(F.conv2d(C._nchw(C._t(X, torch.float64)), C._w_oihw(layers[0][1], torch.float64), C._t(layers[0][2], torch.float64),
                                 padding=1))).numpy()
    assert (a1.reshape(2, 4, 2, 3, 2, 4).max(axis=(2, 4)) == 0).any()        # the tie case is in the draw
    want = np.zeros_like(a1)
    for n in range(2):
        for y in range(4):
            for x in range(3):
                for c in range(4):
                    win = a1[n, 2 * y:2 * y + 2, 2 * x:2 * x + 2, c].reshape(4)
                    p = int(np.argmax(win))                                   # numpy: the first maximum in scan order
                    want[n, 2 * y + p // 2, 2 * x + p % 2, c] = got[(2, 0)][n, y, x, c]
    assert got[(1, 0)].shape == a1.shape
    assert np.array_equal(got[(1, 0)], want)
    assert ((got[(1, 0)] != 0).sum(axis=(1, 2, 3)) <= got[(2, 0)][0].size).all()
    assert np.array_equal(got[(0, 0)], RT.analyze(layers, X, R, [LT.AB10, LT.AB10]))


@pytest.mark.parametrize("name", sorted(LT.PARITY_TABLES) + ["zplus"])
@pytest.mark.parametrize("net", LT.PARITY_NETS)
def test_every_tensor_of_the_gpu_draws_meets_the_float32_condition(net, name):
    r64, r32 = LT.refs(net, name)
    cfg = K.NETS[net][0]
    assert sorted(r64) == LT.node_ids(cfg)
    worst = {i: float(LT.rel_l1_rows(r32[i], r64[i]).max()) for i in r64}
    print(net, name, {i[0]: "%.2e" % v for i, v in sorted(worst.items())})
    assert max(worst.values()) < 1e-5, worst
    # the image-level tensor is the walk the rule-table tests compare with
    if name != "default":
        assert np.array_equal(r64[(0, 0)], K.refs(net, name)[0])


@pytest.mark.parametrize("net", LT.PARITY_NETS)
def test_zplus_conserves_relevance_through_every_tensor(net):
    """Alpha1Beta0 without the bias conserves wherever Z+ != 0, the pools conserve: every tensor of a row has the head's sum."""
    r64, _ = LT.refs(net, "zplus")
    head = r64[(-1, 0)].reshape(len(r64[(-1, 0)]), -1).sum(axis=1)
    scale = np.abs(r64[(-1, 0)]).reshape(len(head), -1).sum(axis=1)
    assert (np.abs(head) > 1e-3 * scale).all()              # a sum that is not itself a cancellation
    for i, a in r64.items():
        s = a.reshape(len(a), -1).sum(axis=1)
        assert (np.abs(s - head) <= 1e-9 * np.abs(head)).all(), (i, s, head)


# ------------------------------------------------------------------------------------------------ analyzer arguments
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("an engine was created before the arguments were checked")
    monkeypatch.setattr(A, "LRPEngine", boom)


def _spec(resnet=False):
    if resnet:
        from lrp_imagecaptioning_amd.synthetic import resnet_weights
        stacks = ((4, 1), (8, 1))
        return A.ImageModelSpec(resnet_weights(np.random.RandomState(0), stacks, stem=8), img_hw=(32, 32), resnet={"stem": 8, "stacks": stacks})
    return A.ImageModelSpec(vgg_weights(np.random.RandomState(0), K.TINY_CFG), cnn_cfg=K.TINY_CFG, img_hw=(16, 16))


SWITCHES = ("reverse_keep_tensors", "reverse_check_min_max_values", "reverse_check_finite")
CLASSES = (lambda s, **k: A.LRPSequentialPresetA(s, **k), lambda s, **k: A.LRP(s, rule="Alpha2Beta1", input_layer_rule="Flat", **k),
           lambda s, **k: A.LRPSequentialPresetBFlat(s, **k), lambda s, **k: A.LRPAlpha2Beta1(s, **k), lambda s, **k: A.DeepTaylor(s, **k))


@pytest.mark.parametrize("make", CLASSES)
def test_the_three_switches_are_taken_by_name(no_engine, make):
    for sw in SWITCHES:
        with pytest.raises(AssertionError):                              # every argument is fine: now the engine is asked for
            make(_spec(), **{sw: True})
    with pytest.raises(AssertionError):
        make(_spec(), **dict((sw, True) for sw in SWITCHES))


@pytest.mark.parametrize("make", CLASSES)
def test_clip_project_and_resnet_are_refused(no_engine, make):
    for sw in ("reverse_clip_values", "reverse_project_bottleneck_layers"):
        with pytest.raises(NotImplementedError):
            make(_spec(), **{sw: True})
        with pytest.raises(AssertionError):
            make(_spec(), **{sw: False})
    if make is not CLASSES[-1]:                                          # (DeepTaylor refuses a ResNet spec whatever the switches)
        for sw in SWITCHES:
            with pytest.raises(NotImplementedError):
                make(_spec(resnet=True), **{sw: True})
        with pytest.raises(AssertionError):                              # without a switch a ResNet spec goes on to its engine
            make(_spec(resnet=True))


def test_switches_off_touch_no_trace_switch(monkeypatch):
    """With all three False nothing changes: no trace switch is set on the engine."""
    calls = []

    class Fake(object):
        def __init__(self, **k):
            pass

        def set_weights(self, w):
            calls.append("weights")

        def set_layer_trace(self, on):
            calls.append(("trace", on))

    monkeypatch.setattr(A, "LRPEngine", Fake)
    A.LRPSequentialPresetA(_spec())
    A.LRPSequentialPresetA(_spec(), reverse_keep_tensors=False, reverse_check_min_max_values=False, reverse_check_finite=False)
    assert calls == ["weights", "weights"]
    a = A.LRPSequentialPresetA(_spec(), reverse_check_finite=True)
    assert calls[-1] == ("trace", True)
    assert a.reversed_tensor_ids() == A.reversed_tensor_ids(K.TINY_CFG) == LT.node_ids(K.TINY_CFG) == [(i, 0) for i in range(-1, 7)]


def test_debug_output_has_the_reference_text(monkeypatch, capsys):
    """_handle_debug_output from per-row statistics: the reference's three lines (base.py:769-802), merged over rows."""
    a = A.LRPSequentialPresetA.__new__(A.LRPSequentialPresetA)
    a._reverse_keep_tensors, a._reverse_check_min_max_values, a._reverse_check_finite = True, True, True
    ids = [(-1, 0), (0, 0), (1, 0)]
    stats = np.array([[[-1.0, 2.0, 0.5, 0.0], [-3.0, 1.0, 0.25, 0.0]],
                      [[0.0, 4.0, 1.0, 0.0], [np.nan, np.nan, np.nan, 2.0]],
                      [[-0.5, 0.5, 0.0, 0.0], [-0.25, np.inf, np.inf, 1.0]]])
    parts = {i: [np.full((1, 1, 1, 1), k, dtype=np.float32), np.full((1, 1, 1, 1), 10 + k, dtype=np.float32)] for k, i in enumerate(ids)}
    a._handle_debug_output(ids, stats, parts)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 3
    assert out[0] == "Minimum values in tensors: ((NodeID, TensorID), Value) - {}".format(
        [((-1, 0), np.float32(-3.0)), ((0, 0), np.float32(np.nan)), ((1, 0), np.float32(-0.5))])
    assert out[1] == "Maximum values in tensors: ((NodeID, TensorID), Value) - {}".format(
        [((-1, 0), np.float32(2.0)), ((0, 0), np.float32(np.nan)), ((1, 0), np.float32(np.inf))])
    assert out[2] == "Not finite values found in following nodes: (NodeID, TensorID) - [(0, 0), (1, 0)]"
    assert [i for i, _ in a._reversed_tensors] == ids
    assert a._reversed_tensors[2][1].shape == (2, 1, 1, 1) and a._reversed_tensors[2][1].dtype == np.float32
    assert a._reversed_stats[(0, 0)]["nonfinite"] == 2 and np.isnan(a._reversed_stats[(0, 0)]["min"])
    assert np.array_equal(a._reversed_stats[(-1, 0)]["sum"], [0.5, 0.25])
