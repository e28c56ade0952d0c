"""-m gpu: PatternNet / PatternAttribution on the device (lrp_pattern_*, LRP_WALK_PATTERNNET / _PATTERN_ATTRIBUTION)
against the float64 restatement of tests/pattern_ref.py, on the draws of tests/pattern_cases.py whose conditions
tests/test_pattern_ref.py checks on the CPU.

Fit and walk are tested apart: the sums and patterns on the dyadic draws (every mask is the same in any arithmetic), the walk on
patterns SET from the float64 fit, never from the device's.  Parity bar of the walk: test_gpu_gradient_family._check."""
import ctypes as C_

import numpy as np
import pytest
import torch

import pattern_cases as PC
import pattern_ref as PR
from lrp_imagecaptioning_amd import _capi
from lrp_imagecaptioning_amd.synthetic import VGG16_CFG, resnet_weights, vgg_weights
from oracle import cnn_lrp_ref as C
from test_gpu_gradient_family import RESNETS, _check, _resnet_engine, _vgg_engine

pytestmark = pytest.mark.gpu
WALKS = (("patternnet", False), ("pattern_attribution", True))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _row_max(out):
    return np.abs(out).reshape(len(out), -1).max(1)


# ------------------------------------------------------------------------------------------------------- 1, 2. sums, patterns
@pytest.mark.parametrize("pattern_type", PC.FIT_TYPES)
@pytest.mark.parametrize("net,seed", PC.FIT_DRAWS)
def test_fit_sums_and_patterns(net, seed, pattern_type):
    d = PC.fit_draw(net, seed)
    r = PC.fit_refs(net, seed, pattern_type)
    eng = _vgg_engine(d["cfg"], PC.HW, d["w"], 3, 3)
    eng.pattern_fit_begin(pattern_type)
    for lo in (0, 3):                                      # fed as 3 + 3 images
        eng.encode_images(d["X"][lo:lo + 3])
        eng.pattern_fit_batch()
    stats = eng.pattern_stats()
    eng.pattern_fit_end()
    got = eng.get_patterns()
    convs = PR.conv_entries(d["layers"])
    for li, (s, ref) in enumerate(zip(stats, r["sums"])):
        P = ref["P"]
        assert s["P"] == P and np.array_equal(s["cnt"], ref["cnt"]), li
        for k in ("Sx", "Sxy", "Sy"):                      # an fp32 sum of P products: P 2^-23 sum |terms|
            err = np.abs(s[k].reshape(ref[k].shape) - ref[k])
            bound = P * 2.0 ** -23 * ref["a" + k]
            print("pattern sums %s/%d %s conv %d %s: max err %.3e (max bound %.3e)" % (net, seed, pattern_type, li, k, err.max(), bound.max()))
            assert (err <= bound).all(), (li, k, float((err - bound).max()))
        # the patterns: against float64, against float64 compute_pattern on the device's own sums, zeros where the restatement has them
        dist32 = PC.rel_l1(r["patterns32"][li], r["patterns"][li])
        err = PC.rel_l1(got[li], r["patterns"][li])
        own = PR.compute_pattern(convs[li][1], dict(Sx=s["Sx"], Sxy=s["Sxy"], cnt=s["cnt"], Sy=s["Sy"], P=s["P"]))
        err_own = PC.rel_l1(got[li], own)
        print("pattern fit %s/%d %s conv %d: rel_l1 %.3e (float32 restatement %.3e), vs own sums %.3e" % (net, seed, pattern_type, li, err, dist32, err_own))
        assert np.isfinite(got[li]).all()
        assert err < max(1e-4, 3 * dist32), (li, err, dist32)
        assert err_own < 1e-6, (li, err_own)
        dead = np.abs(r["patterns"][li]).sum((0, 1, 2)) == 0
        assert not got[li][..., dead].any(), li


# ------------------------------------------------------------------------------------------------------- 3, 4. walk, invariance
@pytest.mark.parametrize("seed", PC.WALK_SEEDS)
def test_walk_parity_and_invariance(seed):
    d = PC.walk_draw(seed)
    idx = list(d["idx"])
    eng = _vgg_engine(PC.FIVE_CFG, PC.HW, d["w"], 3, 6)
    eng.set_patterns(d["patterns"])                        # from the float64 fit, never the device's
    eng.encode_images(d["X"])
    for name, attribution in WALKS:
        for projection in (True, False):
            eng.set_pattern_projection(projection)
            out = eng.cnn_walk(idx, d["head"], name).cpu().numpy()
            ref, ref32 = PC.walk_refs(seed, attribution, projection)
            _check("pattern_" + name, out, ref, ref32, seed=seed, projection=projection)
            if projection:
                assert np.array_equal(_row_max(out), np.ones(len(out), np.float32)), _row_max(out)
                for i in range(len(idx)):                  # a row alone is the row inside the larger call, bit for bit
                    one = eng.cnn_walk([idx[i]], d["head"][i:i + 1], name).cpu().numpy()
                    assert np.array_equal(_bits(one[0]), _bits(out[i])), (name, i)


def test_unprojected_patternnet_with_w_is_the_gradient_walk():
    d = PC.walk_draw(1)
    idx = list(d["idx"])
    eng = _vgg_engine(PC.FIVE_CFG, PC.HW, d["w"], 3, 6)
    eng.set_patterns([L[1] for L in PR.conv_entries(d["layers"])])
    eng.set_pattern_projection(False)
    eng.encode_images(d["X"])
    got = eng.cnn_walk(idx, d["head"], "patternnet").cpu().numpy()
    want = eng.cnn_walk(idx, d["head"], "gradient").cpu().numpy()
    assert np.abs(want).max() > 0
    assert np.array_equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------------- 5. non-interference
def test_patterns_leave_the_other_paths_alone():
    d = PC.walk_draw(2)
    idx = list(d["idx"])
    R = (d["head"] * C.forward(d["layers"], d["X"])[idx]).astype(np.float32)

    def outputs(eng):
        eng.encode_images(d["X"])
        return (eng.get_features().cpu().numpy(), eng.cnn_explain(idx, R).cpu().numpy(), eng.cnn_walk(idx, d["head"], "gradient").cpu().numpy())

    fresh = _vgg_engine(PC.FIVE_CFG, PC.HW, d["w"], 3, 6)
    want = outputs(fresh)
    ws_fresh = fresh.workspace_bytes
    eng = _vgg_engine(PC.FIVE_CFG, PC.HW, d["w"], 3, 6)
    outputs(eng)
    assert eng.workspace_bytes == ws_fresh                 # the same calls, the same bytes: no pattern entry, nothing new
    eng.pattern_fit(d["Xfit"], "relu", batch=3)
    ws_fit = eng.workspace_bytes
    sums = sum(8 * (2 * 9 * cin * cout + 2 * cout + 1) for _, cin, cout, _ in PC.FIVE_CFG)
    assert ws_fit >= ws_fresh + sums                       # what the pattern entries allocate is counted
    eng.set_patterns(d["patterns"])
    eng.encode_images(d["X"])
    eng.cnn_walk(idx, d["head"], "pattern_attribution")
    assert eng.workspace_bytes > ws_fit                    # (the packed matrices and the reduction partials of the first walk)
    for a, b in zip(outputs(eng), want):
        assert np.array_equal(_bits(a), _bits(b))
    assert fresh.workspace_bytes == ws_fresh


# ------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_launch_nothing():
    lib = _capi.load()
    d = PC.walk_draw(1)
    idx = list(d["idx"])
    eng = _vgg_engine(PC.FIVE_CFG, PC.HW, d["w"], 3, 6)
    eng.encode_images(d["X"])
    stacks, stem, hw = RESNETS["tiny"]
    rn, _ = _resnet_engine(stacks, stem, hw, 2, 2, resnet_weights(np.random.RandomState(3), stacks, stem=stem, bias_std=0.2))
    rn.encode_images(np.zeros((1, hw, hw, 3), np.float32))
    rn_head = torch.zeros((1, rn.L, rn.D), device="cuda")
    head = torch.as_tensor(d["head"]).cuda()
    one = torch.zeros((3, 3, 3, 16), device="cuda")
    torch.cuda.synchronize()
    n0 = lib.lrp_launch_count()
    # a ResNet handle: every entry
    for call in (lambda: rn.pattern_fit_begin("relu"), rn.pattern_fit_batch, rn.pattern_fit_end, rn.pattern_stats, rn.get_patterns,
                 lambda: rn.set_pattern_projection(True), lambda: rn.cnn_walk([0], rn_head, "patternnet"),
                 lambda: rn.cnn_walk([0], rn_head, "pattern_attribution")):
        with pytest.raises(NotImplementedError):
            call()
    assert lib.lrp_set_patterns(rn._h, 0, C_.c_void_p(one.data_ptr()), None) == _capi.LRP_ERR_UNSUPPORTED
    # call order
    with pytest.raises(RuntimeError, match="no pattern"):
        eng.cnn_walk(idx, head, "patternnet")
    with pytest.raises(RuntimeError, match="no pattern"):
        eng.get_patterns()
    with pytest.raises(RuntimeError, match="fit_begin"):
        eng.pattern_fit_batch()
    with pytest.raises(RuntimeError, match="fit_begin"):
        eng.pattern_fit_end()
    with pytest.raises(RuntimeError, match="no fit has run"):
        eng.pattern_stats()
    # bad values
    assert lib.lrp_pattern_fit_begin(eng._h, 3) == _capi.LRP_ERR_INVALID
    assert lib.lrp_pattern_fit_begin(eng._h, -1) == _capi.LRP_ERR_INVALID
    for conv in (-1, 5):
        assert lib.lrp_set_patterns(eng._h, conv, C_.c_void_p(one.data_ptr()), None) == _capi.LRP_ERR_INVALID
        assert lib.lrp_get_patterns(eng._h, conv, C_.c_void_p(one.data_ptr()), None) == _capi.LRP_ERR_INVALID
        assert lib.lrp_pattern_stats(eng._h, conv, C_.c_void_p(one.data_ptr()), 1, None) == _capi.LRP_ERR_INVALID
    assert lib.lrp_set_pattern_projection(eng._h, 2) == _capi.LRP_ERR_INVALID
    with pytest.raises(ValueError, match="unknown pattern type"):
        eng.pattern_fit_begin("dummy")
    with pytest.raises(ValueError, match="one pattern per conv"):
        eng.set_patterns(d["patterns"][:4])
    with pytest.raises(ValueError, match="expected HWIO"):
        eng.set_patterns(d["patterns"][::-1])
    # outside LRP_PREC_FP32
    eng.set_precision("bf16x3")
    with pytest.raises(NotImplementedError, match="LRP_PREC_FP32"):
        eng.pattern_fit_begin("relu")
    with pytest.raises(NotImplementedError, match="LRP_PREC_FP32"):
        eng.cnn_walk(idx, head, "patternnet")
    eng.set_precision("fp32")
    assert lib.lrp_launch_count() == n0                    # nothing was launched by any refusal so far
    # a fit: no encode since it began, an encode accumulated twice, an end without a batch
    eng.pattern_fit_begin("relu")
    n1 = lib.lrp_launch_count()
    with pytest.raises(RuntimeError, match="lrp_encode_images must run"):
        eng.pattern_fit_batch()
    with pytest.raises(RuntimeError, match="at least once"):
        eng.pattern_fit_end()
    assert lib.lrp_launch_count() == n1
    eng.encode_images(d["Xfit"][:3])
    eng.pattern_fit_batch()
    n2 = lib.lrp_launch_count()
    with pytest.raises(RuntimeError, match="at most once"):
        eng.pattern_fit_batch()
    assert lib.lrp_launch_count() == n2
    eng.pattern_fit_end()
    # patterns are there; a precision round trip dropped the caches: no encode since
    eng.set_precision("bf16x3")
    eng.set_precision("fp32")
    n3 = lib.lrp_launch_count()
    with pytest.raises(RuntimeError, match="lrp_encode_images must run"):
        eng.cnn_walk(idx, head, "patternnet")
    with pytest.raises(ValueError):
        eng.cnn_walk([], head[:0], "patternnet")
    assert lib.lrp_launch_count() == n3
    eng.encode_images(d["X"])
    assert np.isfinite(eng.cnn_walk(idx, head, "patternnet").cpu().numpy()).all()


# ------------------------------------------------------------------------------------------------------- 7. surface
def test_analyzer_and_pattern_computer_equal_the_engine_route():
    from lrp_imagecaptioning_amd import analyzer as A
    from lrp_imagecaptioning_amd.pattern import PatternComputer
    d = PC.walk_draw(3)
    Xi = d["X"][list(d["idx"])]
    spec = A.ImageModelSpec(d["w"], cnn_cfg=PC.FIVE_CFG, img_hw=(PC.HW, PC.HW))
    eng = _vgg_engine(PC.FIVE_CFG, PC.HW, d["w"], 3, 6)
    want_p = {t: eng.pattern_fit(d["Xfit"], t, batch=3) for t in ("relu", "linear")}
    pc = PatternComputer(spec, pattern_type="relu", max_batch=3)
    got = pc.compute(d["Xfit"], batch_size=3)
    assert isinstance(got, list) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, want_p["relu"]))
    both = PatternComputer(spec, pattern_type=("relu", "linear"), max_batch=3).compute(d["Xfit"], batch_size=3)
    assert sorted(both) == ["linear", "relu"]
    for t in both:
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(both[t], want_p[t]))
    for cls, name in ((A.PatternNet, "patternnet"), (A.PatternAttribution, "pattern_attribution")):
        a = cls(spec, max_batch=3)
        a.fit(d["Xfit"], batch_size=3)                     # pattern_type None: 'relu'
        assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a._patterns, want_p["relu"]))
        out = a.analyze([Xi, d["head"]])
        b = cls(spec, patterns=want_p["relu"], max_batch=6)
        assert np.array_equal(_bits(b.analyze([Xi, d["head"]])), _bits(out))
        eng.set_patterns(want_p["relu"])
        eng.encode_images(d["X"])
        want = eng.cnn_walk(list(d["idx"]), d["head"], name).cpu().numpy()
        assert np.array_equal(_bits(out), _bits(want)), name
    with pytest.warns(UserWarning, match="reverse_project_bottleneck_layers"):
        u = A.PatternNet(spec, patterns=want_p["relu"], reverse_project_bottleneck_layers=False, max_batch=6)
    eng.set_pattern_projection(False)
    want = eng.cnn_walk(list(d["idx"]), d["head"], "patternnet").cpu().numpy()
    assert np.array_equal(_bits(u.analyze([Xi, d["head"]])), _bits(want))


@pytest.mark.parametrize("dec", ["adaptive", "gridtd"])
def test_explainer_classes(dec):
    import lrp_imagecaptioning_amd.explainers as EX
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, gridtd_weights
    d = PC.walk_draw(1)
    rs = np.random.RandomState(5)
    H, V, L, D = 32, 50, 16, 64
    w = dict(d["w"])
    w.update((adaptive_weights if dec == "adaptive" else gridtd_weights)(rs, L, D, H, H, V))
    spec = EX.CaptionModelSpec(w, img_encoder="vgg16", hidden_dim=H, embedding_dim=H, L=L, D=D, vocab_size=V, cnn_cfg=PC.FIVE_CFG,
                               img_hw=(PC.HW, PC.HW))
    X, cap = d["X"][:1], [7, 19, 3, 1]
    eng = _vgg_engine(PC.FIVE_CFG, PC.HW, d["w"], 3, 6)
    fitted = eng.pattern_fit(d["Xfit"], "relu", batch=1)
    stem = "ExplainImgCaptioning" + ("AdaptiveAttention" if dec == "adaptive" else "GridTD")
    for suffix, name in (("PatternNet", "patternnet"), ("PatternAttribution", "pattern_attribution")):
        ex = getattr(EX, stem + suffix)(spec, None, None, max_caption_length=6, patterns=d["patterns"])
        ex._forward_beam_search((None, X), cap)
        g = ex._lstm_decoder_backward(2)
        img = ex._explain_CNN(X, g)
        eng.set_patterns(d["patterns"])
        eng.encode_images(X)
        want = eng.cnn_walk([0], g.reshape(1, L, D), name).cpu().numpy()
        assert np.array_equal(_bits(img), _bits(want)), suffix
        np.testing.assert_array_equal(ex._lstm_decoder_backward(2), g)      # the decoder caches were not touched by the CNN half
        ex2 = getattr(EX, stem + suffix)(spec, None, None, max_caption_length=6)
        with pytest.raises(RuntimeError, match="fit_patterns"):
            ex2._explain_CNN(X, g)
        got = ex2.fit_patterns(d["Xfit"])                  # (max_images = 1: one image per batch)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, fitted))


# ------------------------------------------------------------------------------------------------------- 8. VGG16 at 224
def test_vgg16_full_size():
    """One image fitted, two heads.  Thirteen layers of quotients need not meet the small nets' condition: the distances are
    reported next to the float32 restatement's, not barred."""
    rs = np.random.RandomState(len(VGG16_CFG) + 224)
    w = vgg_weights(rs, VGG16_CFG)
    layers = C.vgg_layers(w, VGG16_CFG)
    X = rs.uniform(-120, 130, size=(1, 224, 224, 3)).astype(np.float32)
    head = rs.standard_normal((2, 14, 14, 512)).astype(np.float32)
    eng = _vgg_engine(VGG16_CFG, 224, w, 1, 2)
    pats = eng.pattern_fit(X, "relu")
    assert all(np.isfinite(p).all() for p in pats)
    ref_p = PR.fit(layers, X, "relu")
    print("pattern vgg16 fit: rel_l1 per conv %s" % ["%.2e" % PC.rel_l1(a, b) for a, b in zip(pats, ref_p)])
    eng.encode_images(X)
    X2 = np.repeat(X, 2, axis=0)
    for name, attribution in WALKS:
        out = eng.cnn_walk([0, 0], head, name).cpu().numpy()
        assert np.isfinite(out).all()
        assert np.array_equal(_row_max(out), np.ones(2, np.float32))
        for i in range(2):
            one = eng.cnn_walk([0], head[i:i + 1], name).cpu().numpy()
            assert np.array_equal(_bits(one[0]), _bits(out[i])), (name, i)
        ref = PR.walk(layers, X2, head, pats, attribution, True)
        ref32 = PR.walk(layers, X2, head, pats, attribution, True, dtype=torch.float32)
        print("pattern vgg16 %s: rel_l1 %.3e (float32 restatement %.3e)" % (
            name, max(PC.rel_l1(out[i], ref[i]) for i in range(2)), max(PC.rel_l1(ref32[i], ref[i]) for i in range(2))))
