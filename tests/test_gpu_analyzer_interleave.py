"""-m gpu: the analyzers of the VGG encoder do not interfere with each other on one handle.

The rule table, the layer trace, DeepLIFT and the pattern fit / walk each keep state of their own on the handle (csrc/encoder_state.h)
and share the kept activations, the chain buffers and the encode caches.  One handle runs, in order: a default walk, a two-chain
table walk (Alpha2Beta1), the table cleared, a traced walk, the trace off, a DeepLIFT mode-2 walk, the reference cleared, a pattern
fit and a PatternAttribution walk, a default walk again.  Every result must be BIT-identical to the same call on a fresh handle
that did only that analyzer, the last default walk to the first, and lrp_workspace_bytes must not grow between the second and a
third repetition of the whole sequence (every analyzer's buffers are allocated once and found again).

TINY_CFG 16 x 16, B = 3, fp32, 4 maps (tests/rule_table_cases.py draws the net)."""
import functools

import numpy as np
import pytest

import rule_table_cases as K
from test_gpu_gradient_family import _vgg_engine

pytestmark = pytest.mark.gpu
N_MAPS = 4
STEPS = ("default", "table", "traced", "deeplift", "pattern")


@functools.lru_cache(maxsize=None)
def _case():
    w, X, idx, R, _ = K.net("tiny")
    rs = np.random.RandomState(23)
    ref = rs.uniform(-120, 130, size=(1, 16, 16, 3)).astype(np.float32)
    ref[:, :8] = X[0, :8]                                  # (agrees with image 0 on half the picture: DeepLIFT's dX == 0 branch runs)
    return w, X, list(idx[:N_MAPS]), np.ascontiguousarray(R[:N_MAPS]), ref


def _engine():
    cfg, hw, B = K.NETS["tiny"]
    return _vgg_engine(cfg, hw, _case()[0], B, N_MAPS)


def _step(eng, name):
    """one analyzer, switched on, run and switched off again: {label: numpy array}"""
    _, X, idx, R, ref = _case()
    if name == "default":
        eng.encode_images(X)
        return {"default": eng.cnn_explain(idx, R).cpu().numpy()}
    if name == "table":
        eng.set_cnn_rule(2, 1)
        eng.encode_images(X)
        out = eng.cnn_explain(idx, R).cpu().numpy()
        eng.set_cnn_rule(1, 0)
        return {"table": out}
    if name == "traced":
        eng.set_layer_trace(True)
        eng.encode_images(X)
        out, stats, kept = eng.cnn_explain_traced(idx, R, keep=True)
        res = {"traced": out.cpu().numpy(), "traced_stats": stats.cpu().numpy()}
        res.update({"traced_keep_%d" % k[0]: v.cpu().numpy() for k, v in kept.items()})
        eng.set_layer_trace(False)
        return res
    if name == "deeplift":
        eng.set_deeplift_reference(ref, approximate_gradient=True)
        eng.encode_images(X)
        out = eng.cnn_walk(idx, R, "deeplift").cpu().numpy()
        eng.set_deeplift_reference(approximate_gradient=None)
        return {"deeplift": out}
    patterns = eng.pattern_fit(X, "relu")
    res = {"pattern_A%d" % li: p for li, p in enumerate(patterns)}
    eng.encode_images(X)
    res["pattern_attribution"] = eng.cnn_walk(idx, R, "pattern_attribution").cpu().numpy()
    return res


def _sequence(eng):
    res = {}
    for name in STEPS:
        res.update(_step(eng, name))
    res["default_again"] = _step(eng, "default")["default"]
    return res


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_analyzers_interleaved_on_one_handle():
    alone = {}
    for name in STEPS:                                     # a fresh handle per analyzer
        alone.update(_step(_engine(), name))
    eng = _engine()
    got = _sequence(eng)
    assert sorted(got) == sorted(list(alone) + ["default_again"])
    for label, ref in alone.items():
        assert np.isfinite(got[label]).all(), label
        assert _same_bits(got[label], ref), "%s differs from the same call on a fresh handle" % label
    assert np.abs(got["default"]).sum() > 0 and np.abs(got["pattern_attribution"]).sum() > 0
    assert not _same_bits(got["table"], got["default"]) and not _same_bits(got["deeplift"], got["default"])
    assert _same_bits(got["default_again"], got["default"]), "the default walk changed after the analyzers ran"
    second = _sequence(eng)
    ws2 = eng.workspace_bytes
    third = _sequence(eng)
    ws3 = eng.workspace_bytes
    print("analyzer interleave: workspace after repetition 2 %d bytes, after repetition 3 %d bytes" % (ws2, ws3))
    assert ws3 == ws2, (ws2, ws3)
    for label in got:
        assert _same_bits(second[label], got[label]) and _same_bits(third[label], got[label]), label
