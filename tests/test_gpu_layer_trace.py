"""-m gpu: the layer trace of the VGG-style LRP walk (lrp_set_layer_trace, lrp_cnn_explain_traced, lrp_op_tensor_stats; the reverse
analyzers' reverse_keep_tensors / reverse_check_min_max_values / reverse_check_finite) against the float64 restatement of the
reversed tensors (tests/layer_trace_ref.py), and against itself.

Bounds.  Parity: every traced tensor and R_img within 1e-4 relative L1 of the float64 restatement per row (the README's parity bar;
tests/test_layer_trace_ref.py holds every tensor of every draw to the condition of that bar, the float32 restatement within 1e-5).
Consistency: minimum, maximum and non-finite count of the statistics equal those of the kept tensor exactly; the float64 sum within
per_row * 2^-52 * sum|kept| of numpy's (two summation orders of per_row float64 terms differ by at most (per_row - 1) * 2^-53 *
sum|x| each).  Conservation under ZPlus: 1e-4 relative to the head's sum, where the oracle holds 1e-9."""
import ctypes

import numpy as np
import pytest
import torch

import layer_trace_ref as LT
import rule_table_cases as K
from conftest import rel_l1
from gpu_util import report
from oracle import cnn_lrp_ref as C

pytestmark = pytest.mark.gpu


def _engine(cfg, hw, B, ntok, w, prec="bf16x3", table=None, trace=True, decoder="adaptive"):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    side = hw
    for _, _, _, p in cfg:
        side = side // 2 if p else side
    eng = LRPEngine(decoder=decoder, cnn_cfg=cfg, img_hw=(hw, hw), L=side * side, D=cfg[-1][2], H=32, E=32, V=50,
                    max_images=B, max_tokens=ntok, max_caption_len=4)
    eng.set_weights(w)
    eng.set_precision(prec)
    if table is not None:
        eng.set_cnn_rules(table)
    if trace:
        eng.set_layer_trace(True)
    return eng


def _draw(net, name):
    cfg, hw, B = K.NETS[net]
    w, X, idx, R, layers = K.net(net, seed=LT.seed_of(name, net))
    return cfg, hw, B, w, X, list(idx), R, layers


def _traced(net, name, prec, keep=True):
    cfg, hw, B, w, X, idx, R, layers = _draw(net, name)
    eng = _engine(cfg, hw, B, 2 * B, w, prec, None if name == "default" else LT.table_of(name))
    eng.encode_images(X)
    return eng, eng.cnn_explain_traced(idx, R, keep=keep)


# ---------------------------------------------------------------- operator
def _np_stats(x):
    x = x.reshape(len(x), -1)
    return np.stack([x.min(axis=1).astype(np.float64), x.max(axis=1).astype(np.float64), x.astype(np.float64).sum(axis=1),
                     (~np.isfinite(x)).sum(axis=1).astype(np.float64)], axis=1)


def _same_value(a, b):
    """equal as numbers, NaN matching NaN; the sign of a zero is checked where the test fixes it"""
    return np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def tiny_engine():
    cfg, hw, B = K.NETS["tiny"]
    return _engine(cfg, hw, B, 2 * B, K.net("tiny")[0], trace=False)


@pytest.mark.parametrize("rows", (1, 5))
@pytest.mark.parametrize("per_row", (1, 3, 255, 257, 1025, 16 * 16 * 8))
def test_tensor_stats_against_numpy(tiny_engine, rows, per_row):
    rs = np.random.RandomState(rows * 10007 + per_row)
    x = (rs.standard_normal((rows, per_row)) * 10.0 ** rs.uniform(-3, 3, size=(rows, 1))).astype(np.float32)
    x[0] = -np.abs(x[0]) - 1.0                           # all negative: a maximum initialised to 0 would show
    if rows > 1:
        x[1] = np.abs(x[1]) + 1.0                        # all positive: the same for the minimum
        x[2, -1] = np.nan                                # a NaN in the last element
        x[3, 0] = np.inf
        x[3, per_row // 2] = -np.inf if per_row > 2 else x[3, per_row // 2]
        x[4] = 0.0
        x[4, per_row // 3] = -0.0
    with np.errstate(invalid="ignore"):
        want = _np_stats(x)
    got = tiny_engine.tensor_stats(x).cpu().numpy()
    assert _same_value(got[:, 0], want[:, 0]) and _same_value(got[:, 1], want[:, 1]), (got, want)
    assert np.array_equal(got[:, 3], want[:, 3])
    for r in range(rows):
        if np.isfinite(want[r, 2]):
            assert abs(got[r, 2] - want[r, 2]) <= per_row * 2.0 ** -52 * np.abs(x[r].astype(np.float64)).sum(), r
        else:
            assert _same_value(got[r, 2], want[r, 2]), r
    if rows > 1:                                         # -0.0 orders below +0.0: a row of zeros with one -0.0
        assert np.signbit(got[4, 0]) and not np.signbit(got[4, 1] if per_row > 1 else 1.0) and got[4, 0] == 0.0 and got[4, 2] == 0.0
    # the same through a tensor of more axes, and a row of one element is its own minimum, maximum and sum
    one = tiny_engine.tensor_stats(x[:, :1].reshape(rows, 1, 1, 1)).cpu().numpy()
    assert _same_value(one[:, 0], x[:, 0].astype(np.float64)) and _same_value(one[:, 1], x[:, 0].astype(np.float64))
    assert _same_value(one[:, 2], x[:, 0].astype(np.float64))


def test_tensor_stats_refuses_bad_arguments(tiny_engine):
    from lrp_imagecaptioning_amd import _capi as CA
    with pytest.raises(ValueError):
        tiny_engine.tensor_stats(np.zeros((0, 4), dtype=np.float32))
    x = torch.zeros(4, device="cuda")
    with pytest.raises(ValueError):
        CA.check(tiny_engine._lib.lrp_op_tensor_stats(ctypes.c_void_p(x.data_ptr()), 0, 4, ctypes.c_void_p(x.data_ptr()), None))
    with pytest.raises(ValueError):
        CA.check(tiny_engine._lib.lrp_op_tensor_stats(None, 1, 4, ctypes.c_void_p(x.data_ptr()), None))


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("name,prec", [(n, p) for n in sorted(LT.PARITY_TABLES) for p in LT.PARITY_TABLES[n]])
@pytest.mark.parametrize("net", LT.PARITY_NETS)
def test_every_traced_tensor_matches_the_restatement(net, name, prec):
    eng, (R_img, stats, kept) = _traced(net, name, prec)
    r64, r32 = LT.refs(net, name)
    ids = [i for i, _ in eng.trace_tensors()]
    assert ids == sorted(r64) == LT.node_ids(K.NETS[net][0])
    assert sorted(kept) == ids
    worst = {}
    for i in ids:
        out = kept[i].cpu().numpy()
        assert out.shape == r64[i].shape and out.dtype == np.float32 and np.isfinite(out).all()
        worst[i] = float(LT.rel_l1_rows(out, r64[i]).max())
    own = max(float(LT.rel_l1_rows(r32[i], r64[i]).max()) for i in ids)
    img = float(LT.rel_l1_rows(R_img.cpu().numpy(), r64[(0, 0)]).max())
    report("layer_trace_%s_%s_%s" % (net, prec, name), r_img=img, f32_restatement=own, **{"t%d" % i[0]: v for i, v in worst.items()})
    print(net, prec, name, "R_img %.2e own %.2e" % (img, own), {i[0]: "%.2e" % v for i, v in sorted(worst.items())})
    assert own < 1e-5                                    # the draw's condition (tests/test_layer_trace_ref.py)
    assert max(worst.values()) < 1e-4, worst
    assert img < 1e-4
    assert torch.equal(R_img, kept[(0, 0)])              # the image-level tensor IS the result


# ---------------------------------------------------------------- consistency
def _check_consistency(eng, stats, kept, cfg, layers, X, idx):
    st = stats.cpu().numpy()
    ids = [i for i, _ in eng.trace_tensors()]
    for k, i in enumerate(ids):
        a = kept[i].cpu().numpy()
        n, per = len(a), a[0].size
        flat = a.reshape(n, -1)
        assert np.array_equal(st[k, :, 0], flat.min(axis=1).astype(np.float64)), i
        assert np.array_equal(st[k, :, 1], flat.max(axis=1).astype(np.float64)), i
        assert np.array_equal(st[k, :, 3], (~np.isfinite(flat)).sum(axis=1)), i
        ref = flat.astype(np.float64).sum(axis=1)
        bound = per * 2.0 ** -52 * np.abs(flat.astype(np.float64)).sum(axis=1)
        assert (np.abs(st[k, :, 2] - ref) <= bound).all(), (i, st[k, :, 2], ref, bound)
    # a pool-input tensor is the pool-output tensor at one cell per window, exact zeros elsewhere; that cell is the forward's
    # arg-max (the float64 forward's, up to the forward's own accuracy where two cells of a window nearly tie)
    _, inputs = C.forward(layers, X[idx], torch.float64, return_inputs=True)
    pools = 0
    for nid, L in enumerate(layers):
        if L[0] != "pool":
            continue
        pools += 1
        pin, pout = kept[(nid, 0)].cpu().numpy(), kept[(nid + 1, 0)].cpu().numpy()
        n, H, W, Cc = pin.shape
        win = pin.reshape(n, H // 2, 2, W // 2, 2, Cc).transpose(0, 1, 3, 5, 2, 4).reshape(n, H // 2, W // 2, Cc, 4)
        assert ((win != 0).sum(axis=-1) <= 1).all()
        pos = np.abs(win).argmax(axis=-1)
        routed = np.take_along_axis(win, pos[..., None], axis=-1)[..., 0]
        assert np.array_equal(routed.view(np.uint32) & 0x7fffffff, pout.view(np.uint32) & 0x7fffffff)     # (a zero: either sign)
        assert np.array_equal(routed[pout != 0], pout[pout != 0])
        act = C._nhwc(inputs[nid]).numpy()
        awin = act.reshape(n, H // 2, 2, W // 2, 2, Cc).transpose(0, 1, 3, 5, 2, 4).reshape(n, H // 2, W // 2, Cc, 4)
        at = np.take_along_axis(awin, pos[..., None], axis=-1)[..., 0]
        hit = pout != 0
        assert hit.any()
        assert (at[hit] >= awin.max(axis=-1)[hit] * (1 - 1e-5)).all()
    assert pools == sum(1 for c in cfg if c[3])


@pytest.mark.parametrize("net,name,prec", [("tiny", "default", "fp32"), ("mid", "presetBflat", "bf16x3"), ("mid", "default", "bf16x3"),
                                           ("mid", "composite", "fp32")])
def test_statistics_and_pool_routing_agree_with_the_kept_tensors(net, name, prec):
    cfg, hw, B, w, X, idx, R, layers = _draw(net, name)
    eng, (R_img, stats, kept) = _traced(net, name, prec)
    _check_consistency(eng, stats, kept, cfg, layers, X, idx)


@pytest.mark.parametrize("prec", ("fp32", "bf16x3"))
@pytest.mark.parametrize("net", LT.PARITY_NETS)
def test_zplus_conserves_through_every_tensor(net, prec):
    eng, (R_img, stats, kept) = _traced(net, "zplus", prec, keep=())
    s = stats.cpu().numpy()[:, :, 2]
    head = s[0]
    worst = float(np.abs((s - head) / head).max())
    report("layer_trace_conservation_%s_%s" % (net, prec), worst=worst)
    print(net, prec, "conservation %.2e" % worst)
    assert kept == {}
    assert worst < 1e-4, s


# ---------------------------------------------------------------- invariance and non-interference
@pytest.mark.parametrize("name,prec", [("default", "bf16x3"), ("presetBflat", "bf16x3"), ("mixed_ab", "fp32")])
def test_rows_do_not_depend_on_the_call(name, prec):
    cfg, hw, B, w, X, idx, R, layers = _draw("tiny", name)
    eng, (R_img, stats, kept) = _traced("tiny", name, prec)
    R_img, stats, kept = R_img.clone(), stats.clone(), {i: t.clone() for i, t in kept.items()}
    assert len(idx) == 6
    for r in (0, 4):                                     # n = 1 against the same row inside n = 6
        a, s, k = eng.cnn_explain_traced([idx[r]], R[r:r + 1], keep=True)
        assert torch.equal(a[0], R_img[r])
        assert torch.equal(s[:, 0].view(torch.int64), stats[:, r].view(torch.int64))
        for i in kept:
            assert torch.equal(k[i][0], kept[i][r]), i
    # subsets of the keep mask give the same bits as keep-all; ids as tuples or node ids
    ids = sorted(kept)
    for sub in ([ids[0]], [ids[1], ids[-1]], [i[0] for i in ids[2:5]], ids[3:4]):
        a, s, k = eng.cnn_explain_traced(idx, R, keep=sub)
        assert sorted(k) == sorted((i, 0) if isinstance(i, int) else i for i in sub)
        assert torch.equal(a, R_img) and torch.equal(s.view(torch.int64), stats.view(torch.int64))
        for i in k:
            assert torch.equal(k[i], kept[i]), i
    a, s, k = eng.cnn_explain_traced(idx, R)
    assert k == {} and torch.equal(a, R_img) and torch.equal(s.view(torch.int64), stats.view(torch.int64))
    with pytest.raises(ValueError):
        eng.cnn_explain_traced(idx, R, keep=[(len(ids), 0)])


@pytest.mark.parametrize("name,prec", [("default", "bf16x3"), ("default", "fp32"), ("presetBflat", "bf16x3")])
@pytest.mark.parametrize("net", ("tiny", "mid"))
def test_the_untraced_walk_does_not_see_the_switch(net, name, prec):
    cfg, hw, B, w, X, idx, R, layers = _draw(net, name)
    table = None if name == "default" else LT.table_of(name)
    fresh = _engine(cfg, hw, B, 2 * B, w, prec, table, trace=False)
    fresh.encode_images(X)
    want = fresh.cnn_explain(idx, R).clone()
    feat = fresh.get_features().clone()
    eng = _engine(cfg, hw, B, 2 * B, w, prec, table, trace=False)
    ws0 = eng.workspace_bytes
    eng.set_layer_trace(True)
    ws_on = eng.workspace_bytes
    kept_acts = sum(4 * B * (hw >> sum(1 for q in cfg[:li] if q[3])) ** 2 * c[2] for li, c in enumerate(cfg[:-1]) if not c[3])
    assert ws_on - ws0 in (0, kept_acts)                 # (a rule table has allocated them already)
    eng.set_layer_trace(True)                            # the same value again: nothing
    assert eng.workspace_bytes == ws_on
    with pytest.raises(RuntimeError):                    # no encode since the switch was set
        eng.cnn_explain_traced(idx, R)
    eng.encode_images(X)
    assert torch.equal(eng.get_features(), feat)
    assert torch.equal(eng.cnn_explain(idx, R), want)    # switch on, before any traced call
    ws_enc = eng.workspace_bytes
    eng.cnn_explain_traced(idx, R, keep=True)
    ws_traced = eng.workspace_bytes
    assert ws_traced > ws_enc                            # the partials of the reductions: with the first traced call ...
    eng.cnn_explain_traced(idx[:1], R[:1])
    eng.cnn_explain_traced(idx, R, keep=True)
    assert eng.workspace_bytes == ws_traced              # ... once
    assert torch.equal(eng.cnn_explain(idx, R), want)    # after traced calls
    eng.set_layer_trace(False)
    with pytest.raises(RuntimeError):
        eng.cnn_explain(idx, R)                          # the change dropped the caches
    eng.encode_images(X)
    assert torch.equal(eng.cnn_explain(idx, R), want)
    with pytest.raises(RuntimeError):                    # switch off
        eng.cnn_explain_traced(idx, R)


@pytest.mark.parametrize("dec", ("adaptive", "gridtd"))
def test_explain_tokens_does_not_see_the_switch(dec):
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, gridtd_weights
    cfg, hw, B, w, X, idx, R, layers = _draw("tiny", "default")
    w = dict(w)
    w.update((adaptive_weights if dec == "adaptive" else gridtd_weights)(np.random.RandomState(5), 16, 16, 32, 32, 50))
    caps = [[7, 19, 3, 1], [4, 1], [9, 2, 1]]
    outs = []
    for trace in (False, True):
        eng = _engine(cfg, hw, B, 12, w, "bf16x3", None, trace=trace, decoder=dec)
        eng.encode_images(X)
        eng.decoder_forward(caps)
        pairs = [(b, t) for b, c in enumerate(caps) for t in range(1, len(c))]
        if trace:
            first = eng.explain_tokens([p[0] for p in pairs], [p[1] for p in pairs], want_R_feat=True)
            eng.cnn_explain_traced([p[0] for p in pairs], first[1], keep=True)
        outs.append([t.clone() for t in eng.explain_tokens([p[0] for p in pairs], [p[1] for p in pairs], want_R_feat=True)[:2]])
        if trace:
            assert torch.equal(first[0], outs[-1][0])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][0].abs().sum()) > 0


# ---------------------------------------------------------------- finite check
@pytest.mark.parametrize("name,prec", [("default", "bf16x3"), ("presetBflat", "fp32")])
def test_non_finite_heads_are_counted_where_they_arrive(name, prec, capsys):
    """One head row with a NaN and one with +inf at a single position: data, not a fault."""
    from lrp_imagecaptioning_amd import analyzer as A
    cfg, hw, B, w, X, idx, R, layers = _draw("tiny", name)
    eng, (R_img, stats, kept) = _traced("tiny", name, prec, keep=())
    clean = stats.clone()
    bad = R.copy()
    bad[1, 1, 2, 3] = np.nan
    bad[4, 2, 1, 5] = np.inf
    _, st, _ = eng.cnn_explain_traced(idx, bad)
    st = st.cpu().numpy()
    for r in (1, 4):
        assert (st[:, r, 3] > 0).all(), st[:, r, 3]      # at the head and in every tensor below it
    assert st[0, 1, 3] == 1 and st[0, 4, 3] == 1 and np.isnan(st[0, 1, 0]) and st[0, 4, 1] == np.inf
    for r in (0, 2, 3, 5):
        assert np.array_equal(st[:, r].view(np.int64), clean.cpu().numpy()[:, r].view(np.int64)), r
    # through the analyzer: the reference's line names exactly the affected ids — all of them for these rows ...
    rule = dict(default="Alpha1Beta0", presetBflat="Alpha2Beta1")[name]
    an = A.LRP(A.ImageModelSpec(w, cnn_cfg=cfg, img_hw=(hw, hw)), rule=rule, input_layer_rule=None if name == "default" else "Flat",
               reverse_check_finite=True, max_batch=4)
    an._engine.set_precision(prec)
    capsys.readouterr()
    an.analyze([X[idx], bad])
    assert capsys.readouterr().out == "Not finite values found in following nodes: (NodeID, TensorID) - {}\n".format(LT.node_ids(cfg))
    assert all(v["nonfinite"] > 0 for v in an._reversed_stats.values())
    # ... and a clean batch prints nothing
    an.analyze([X[idx], R])
    assert capsys.readouterr().out == ""
    assert all(v["nonfinite"] == 0 for v in an._reversed_stats.values())


# ---------------------------------------------------------------- refusals
def test_refusals():
    from lrp_imagecaptioning_amd import _capi as CA
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import resnet_weights
    cfg, hw, B, w, X, idx, R, layers = _draw("tiny", "default")
    eng = _engine(cfg, hw, B, 2 * B, w, "bf16x3", None, trace=False)
    eng.encode_images(X)
    with pytest.raises(RuntimeError):                    # no switch
        eng.cnn_explain_traced(idx, R)
    eng.set_layer_trace(True)
    with pytest.raises(RuntimeError):                    # no encode since
        eng.cnn_explain_traced(idx, R)
    eng.encode_images(X)
    eng.cnn_explain_traced(idx, R)
    with pytest.raises(ValueError):
        eng.cnn_explain_traced(list(idx) + [0], np.concatenate([R, R[:1]]))      # n beyond max_tokens
    # a keep buffer smaller than the info entry says: nothing is launched
    info, total = eng._trace_info(len(idx), 0b101)
    assert [o >= 0 for _, _, o in info] == [True, False, True] + [False] * (len(info) - 3) and total > 0
    assert all(o % 4 == 0 for _, _, o in info if o >= 0)
    n = len(idx)
    ii = (ctypes.c_int32 * n)(*idx)
    Rd = torch.as_tensor(R).cuda().reshape(n, eng.L, eng.D).contiguous()
    out = torch.zeros((n, hw, hw, 3), device="cuda")
    st = torch.zeros((len(info), n, 4), dtype=torch.float64, device="cuda")
    buf = torch.zeros(total, device="cuda")
    launches = eng._lib.lrp_launch_count()
    rc = eng._lib.lrp_cnn_explain_traced(eng._h, n, ii, ctypes.c_void_p(Rd.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                         ctypes.c_void_p(st.data_ptr()), 0b101, ctypes.c_void_p(buf.data_ptr()), total - 1, None)
    assert rc == CA.LRP_ERR_INVALID
    rc = eng._lib.lrp_cnn_explain_traced(eng._h, n, ii, ctypes.c_void_p(Rd.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                         ctypes.c_void_p(st.data_ptr()), 1 << len(info), ctypes.c_void_p(buf.data_ptr()), total, None)
    assert rc == CA.LRP_ERR_INVALID                      # a mask that names no tensor
    torch.cuda.synchronize()
    assert eng._lib.lrp_launch_count() == launches
    assert float(out.abs().sum()) == 0 and float(st.abs().sum()) == 0 and float(buf.abs().sum()) == 0
    # modes
    eng.set_precision("f16x2")                          # (the mode is refused before the state is looked at)
    with pytest.raises(NotImplementedError):
        eng.cnn_explain_traced(idx, R)
    eng.set_precision("bf16x3")
    eng.set_cnn_rules(K.table("composite"))              # an epsilon table outside fp32
    with pytest.raises(NotImplementedError):
        eng.cnn_explain_traced(idx, R)
    eng.set_precision("fp32")
    eng.encode_images(X)
    eng.cnn_explain_traced(idx, R)
    # ResNet
    stacks, stem, rhw = ((4, 2), (8, 2)), 8, 32
    side = rhw // 4 // 2
    rn = LRPEngine(decoder="gridtd", img_hw=(rhw, rhw), L=side * side, D=4 * stacks[-1][0], H=32, E=32, V=50, max_images=1,
                   max_tokens=1, max_caption_len=6, resnet={"stem": stem, "stacks": stacks})
    rs = np.random.RandomState(0)
    rn.set_weights(resnet_weights(rs, stacks, stem=stem, bias_std=0.2))
    with pytest.raises(NotImplementedError):
        rn.set_layer_trace(True)
    with pytest.raises(NotImplementedError):
        rn.trace_tensors()
    rn.encode_images(rs.uniform(-120, 130, size=(1, rhw, rhw, 3)).astype(np.float32))
    with pytest.raises(NotImplementedError):
        rn.cnn_explain_traced([0], rs.standard_normal((1, side * side, 4 * stacks[-1][0])).astype(np.float32))


# ---------------------------------------------------------------- analyzer and explainer
def test_analyzer_keeps_and_prints_what_the_reference_does(capsys):
    from lrp_imagecaptioning_amd import analyzer as A
    cfg, hw, B, w, X, idx, R, layers = _draw("tiny", "default")
    r64, _ = LT.refs("tiny", "default")
    an = A.LRPSequentialPresetA(A.ImageModelSpec(w, cnn_cfg=cfg, img_hw=(hw, hw)), reverse_keep_tensors=True,
                                reverse_check_min_max_values=True, max_batch=2)
    capsys.readouterr()
    out = an.analyze([X[idx][:5], R[:5]])                # 5 inputs in chunks of 2
    lines = capsys.readouterr().out.splitlines()
    ids = LT.node_ids(cfg)
    assert an.reversed_tensor_ids() == ids == [i for i, _ in an._reversed_tensors]
    for i, a in an._reversed_tensors:
        assert a.dtype == np.float32 and a.shape == (5,) + r64[i].shape[1:]
        assert float(LT.rel_l1_rows(a, r64[i][:5]).max()) < 1e-4, i
    assert np.array_equal(out, dict(an._reversed_tensors)[(0, 0)])
    assert max(rel_l1(out[i], r64[(0, 0)][i]) for i in range(5)) < 1e-4
    mn = [(i, np.float32(a.min())) for i, a in an._reversed_tensors]
    mx = [(i, np.float32(a.max())) for i, a in an._reversed_tensors]
    assert lines == ["Minimum values in tensors: ((NodeID, TensorID), Value) - {}".format(mn),
                     "Maximum values in tensors: ((NodeID, TensorID), Value) - {}".format(mx)]
    for i, a in an._reversed_tensors:
        s = an._reversed_stats[i]
        assert s["min"] == float(a.min()) and s["max"] == float(a.max()) and s["nonfinite"] == 0 and s["sum"].shape == (5,)
        assert np.allclose(s["sum"], a.reshape(5, -1).astype(np.float64).sum(axis=1), rtol=0, atol=a[0].size * 2.0 ** -52 * np.abs(a).sum())
    # the same class without a switch: the same map, no output, no trace on its engine
    plain = A.LRPSequentialPresetA(A.ImageModelSpec(w, cnn_cfg=cfg, img_hw=(hw, hw)), max_batch=2)
    assert not getattr(plain._engine, "layer_trace", False) and not hasattr(plain, "_reversed_tensors")
    with pytest.raises(RuntimeError):
        plain._engine.cnn_explain_traced([0], R[:1])
    # DeepTaylor: the head passes the output ReLU first; its head tensor is the masked one
    dt = A.DeepTaylor(A.ImageModelSpec(w, cnn_cfg=cfg, img_hw=(hw, hw)), reverse_keep_tensors=True, max_batch=3)
    head = np.random.RandomState(2).standard_normal(R[:3].shape).astype(np.float32)
    got = dt.analyze([X, head])
    feat = C.forward(layers, X)
    assert np.array_equal(dict(dt._reversed_tensors)[(-1, 0)], head * (feat > 0))
    # (the untraced class walks the same rule on other launches: both within 1e-4 of the restatement, so 2e-4 of each other)
    plain_dt = A.DeepTaylor(A.ImageModelSpec(w, cnn_cfg=cfg, img_hw=(hw, hw)), max_batch=3).analyze([X, head])
    assert max(rel_l1(got[i], plain_dt[i]) for i in range(3)) < 2e-4


@pytest.mark.parametrize("dec", ("adaptive", "gridtd"))
def test_explainer_layer_relevance(dec):
    import lrp_imagecaptioning_amd.explainers as EX
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, gridtd_weights
    cfg, hw, B, w, X, idx, R, layers = _draw("tiny", "default")
    rs = np.random.RandomState(5)
    H, V, L, D = 32, 50, 16, 16
    w = dict(w)
    w.update((adaptive_weights if dec == "adaptive" else gridtd_weights)(rs, L, D, H, H, V))
    spec = EX.CaptionModelSpec(w, img_encoder="vgg16", hidden_dim=H, embedding_dim=H, L=L, D=D, vocab_size=V, cnn_cfg=cfg, img_hw=(hw, hw))
    stem = "ExplainImgCaptioning" + ("AdaptiveAttention" if dec == "adaptive" else "GridTDModel")
    ex = getattr(EX, stem)(spec, None, None, max_caption_length=6, layer_trace=True)
    cap = [7, 19, 3, 1]
    ex._forward_beam_search((None, X[:1]), cap)
    ids, stats, kept = ex.layer_relevance(ts=[1, 3], keep=[(0, 0), (-1, 0)])
    assert ids == LT.node_ids(cfg) and stats.shape == (2, len(ids), 4) and sorted(kept) == [(-1, 0), (0, 0)]
    Rf, _, _ = ex._engine.decoder_explain([0, 0], [1, 3], variant="sequence")
    img, st, k = ex._engine.cnn_explain_traced([0, 0], Rf, keep=True)
    assert np.array_equal(stats.view(np.int64), st.permute(1, 0, 2).cpu().numpy().view(np.int64))
    assert torch.equal(kept[(0, 0)], img) and torch.equal(kept[(-1, 0)], Rf.reshape(2, 4, 4, D))
    # (the untraced walk runs the same rule on other launches: both within 1e-4 of the restatement, so 2e-4 of each other)
    plain = ex._explain_CNN(X[:1], Rf.cpu().numpy().reshape(2, 4, 4, D))
    assert max(rel_l1(kept[(0, 0)][i].cpu().numpy(), plain[i]) for i in range(2)) < 2e-4
    assert ex.layer_relevance()[1].shape == (len(cap) - 1, len(ids), 4)
    with pytest.raises(NotImplementedError):
        ex.layer_relevance(ts=[9])
    # without the keyword: an error that says how to enable it
    off = getattr(EX, stem)(spec, None, None, max_caption_length=6)
    off._forward_beam_search((None, X[:1]), cap)
    with pytest.raises(RuntimeError, match="layer_trace=True"):
        off.layer_relevance()
    grad = getattr(EX, "ExplainImgCaptioning" + ("AdaptiveAttention" if dec == "adaptive" else "GridTD") + "Gradient")
    g = grad(spec, None, None, max_caption_length=6)
    with pytest.raises(NotImplementedError):
        g.layer_relevance()


# ---------------------------------------------------------------- full size
@pytest.fixture(scope="module")
def vgg16_case():
    from lrp_imagecaptioning_amd.synthetic import VGG16_CFG, vgg_weights
    rs = np.random.RandomState(len(VGG16_CFG) + 224)
    w = vgg_weights(rs, VGG16_CFG, bias_std=0.05)
    layers = C.vgg_layers(w, VGG16_CFG)
    X = rs.uniform(-120, 130, size=(1, 224, 224, 3)).astype(np.float32)
    feat = C.forward(layers, X)
    head = (rs.standard_normal((2,) + feat.shape[1:]) * feat).astype(np.float32)
    table = (LT.AB10,) * len(VGG16_CFG)
    Xi = np.repeat(X, 2, axis=0)
    r64 = dict(LT.analyze_traced(layers, Xi, head, table))
    r32 = dict(LT.analyze_traced(layers, Xi, head, table, dtype=torch.float32))
    return VGG16_CFG, w, X, head, r64, r32


@pytest.mark.parametrize("prec", ("fp32", "bf16x3"))
def test_vgg16_at_224(vgg16_case, prec):
    """One image, two heads.  R_img is held to the bar; the per-tensor distances are reported next to the float32 restatement's
    own, not barred: thirteen layers of ratios are not guaranteed to meet the small nets' condition."""
    cfg, w, X, head, r64, r32 = vgg16_case
    eng = _engine(cfg, 224, 1, 2, w, prec)
    eng.encode_images(X)
    R_img, stats, kept = eng.cnn_explain_traced([0, 0], head, keep=True)
    ids = [i for i, _ in eng.trace_tensors()]
    assert len(ids) == 18 and ids == sorted(r64)         # N = 17 nodes and the head
    st = stats.cpu().numpy()
    assert np.isfinite(st).all() and (st[:, :, 3] == 0).all()
    dist = {}
    for i in ids:
        a = kept[i].cpu().numpy()
        assert np.isfinite(a).all()
        dist[i] = (float(LT.rel_l1_rows(a, r64[i]).max()), float(LT.rel_l1_rows(r32[i], r64[i]).max()))
    report("layer_trace_vgg16_%s" % prec, **{"t%d" % i[0]: v[0] for i, v in dist.items()}, **{"f32_t%d" % i[0]: v[1] for i, v in dist.items()})
    print(prec, {i[0]: "%.2e (f32 %.2e)" % v for i, v in sorted(dist.items())})
    assert float(LT.rel_l1_rows(R_img.cpu().numpy(), r64[(0, 0)]).max()) < 1e-4
    R_img, stats = R_img.clone(), stats.clone()
    kept = {i: t.clone() for i, t in kept.items()}
    for r in range(2):                                   # n = 1 is the same row of n = 2, bit for bit
        a, s, k = eng.cnn_explain_traced([0], head[r:r + 1], keep=True)
        assert torch.equal(a[0], R_img[r]) and torch.equal(s[:, 0].view(torch.int64), stats[:, r].view(torch.int64))
        for i in ids:
            assert torch.equal(k[i][0], kept[i][r]), i
