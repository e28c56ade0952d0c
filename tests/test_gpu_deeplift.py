"""-m gpu: DeepLIFT on the device (lrp_set_deeplift_reference, LRP_WALK_DEEPLIFT, lrp_op_deeplift_conv; analyzer.DeepLIFT and the two
explainer classes) against the restatements of tests/deeplift_ref.py, and the DeepTaylor companion classes.

Whole walk.  The rule is ill-conditioned on ordinary float weights (A / dY with dY a difference of activations), so the parity
draws are DYADIC (deeplift_ref.dyadic_vgg_weights, integer images in [-4, 4], integer references): there the float32 forward
equals the float64 one bit for bit, which every draw asserts on the CPU before it is used, together with noise32 <= 3e-5 — the
float32 restatement's distance from float64.  Bar, the project's: rel_l1 < max(1e-4, 3 x noise32) and gpu_util.band_bar.
The draws whose reference agrees with the images on a region (`patch`: the images are one base picture with their own 6 x 6 patch,
the reference is that picture with another; `block`: a block of pixels equal to the scalar reference) also assert that dropping
the switch moves every float64 map by more than 10 x the tolerance, `patch` that the live dY == 0 share of some layer is >= 5 %.

Operator.  Random float operands; gpu_util.elem_ratio against float64 under gpu_util.elem_bar of torch's float32 evaluation.

Full size.  No parity bar: the literal graph is ill-conditioned at thirteen layers and the dyadic recipe is not exact there;
finite, and B = 1 == B = 2 bit for bit."""
import functools

import numpy as np
import pytest
import torch

import deeplift_ref as DL
import gradient_family_ref as GF
import rule_table_cases as K
from conftest import rel_l1
from gpu_util import band_bar, band_rel_l1, elem_bar, elem_ratio, report
from lrp_imagecaptioning_amd.synthetic import VGG16_CFG, vgg_weights
from oracle import cnn_lrp_ref as C

pytestmark = pytest.mark.gpu
TOL, NOISE_MAX = 1e-4, 3e-5
CFG = [("c1", 3, 16, False), ("c2", 16, 16, True), ("c3", 16, 32, False), ("c4", 32, 32, True), ("c5", 32, 64, False)]   # test_gpu_gradient_family.CFG
SEED = 4
KINDS = ("scalar0", "scalar1", "patch", "block")
IDX = [0, 1, 2, 2, 0, 1]


def _engine(cfg, hw, w, nb, ntok, prec="fp32"):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    h = hw
    for c in cfg:
        h = h // 2 if c[3] else h
    eng = LRPEngine(decoder="adaptive", cnn_cfg=cfg, img_hw=(hw, hw), L=h * h, D=cfg[-1][2], H=8, E=8, V=8, max_images=nb,
                    max_tokens=ntok, max_caption_len=2)
    eng.set_weights(w)
    eng.set_precision(prec)
    return eng


@functools.lru_cache(maxsize=None)
def _case(kind):
    """the five-conv 16 x 16 dyadic net, 3 images, 6 heads crossing images; float64 and float32 restatements for both modes,
    computed once and never written to"""
    rs = np.random.RandomState(SEED + KINDS.index(kind))
    w = DL.dyadic_vgg_weights(rs, CFG)
    layers = C.vgg_layers(w, CFG)
    X = rs.randint(-4, 5, size=(3, 16, 16, 3)).astype(np.float32)
    ref = {"scalar0": 0.0, "scalar1": 1.0, "block": 1.0}.get(kind)
    if kind == "patch":
        base = rs.randint(-4, 5, size=(16, 16, 3)).astype(np.float32)
        X[:] = base
        X[:, 5:11, 5:11] = rs.randint(-4, 5, size=(3, 6, 6, 3))
        ref = base.copy()
        ref[5:11, 5:11] = rs.randint(-4, 5, size=(6, 6, 3))
    if kind == "block":
        X[:, 2:8, 3:9] = 1.0
    head = rs.standard_normal((6, 4, 4, 64)).astype(np.float32)
    refs = {a: DL.deeplift_vgg(layers, X[IDX], head, ref, a) for a in (True, False)}
    refs32 = {a: GF.single_thread_float32(DL.deeplift_vgg, layers, X[IDX], head, ref, a) for a in (True, False)}
    for d in (refs, refs32):
        for v in d.values():
            v.setflags(write=False)
    return dict(w=w, layers=layers, X=X, ref=ref, head=head, refs=refs, refs32=refs32)


def _check_draw(kind, c):
    """what a draw has to be before the device is asked anything"""
    assert DL.forward_is_exact(c["layers"], c["X"])
    assert DL.forward_is_exact(c["layers"], DL._reference(c["ref"], c["X"]).astype(np.float32))
    noise = {a: max(rel_l1(c["refs32"][a][i], c["refs"][a][i]) for i in range(6)) for a in (True, False)}
    assert max(noise.values()) <= NOISE_MAX, noise
    if kind in ("patch", "block"):
        tol = max(TOL, 3 * noise[True])
        moved = min(rel_l1(c["refs"][False][i], c["refs"][True][i]) for i in range(6))
        assert moved > 10 * tol, moved                     # the switch carries a visible share of every map
    if kind == "patch":
        share = DL.deeplift_stats(c["layers"], c["X"], c["ref"])
        assert max(share) >= 0.05, share                   # SafeDivide's dY == 0 branch on live units
    return noise


def _check(name, out, ref, ref32, **kv):
    n = len(out)
    noise32 = max(rel_l1(ref32[i], ref[i]) for i in range(n))
    bar, band32 = band_bar(ref32, ref)
    errs = [rel_l1(out[i], ref[i]) for i in range(n)]
    band = max(band_rel_l1(out[i], ref[i], where=True) for i in range(n))
    report("deeplift_" + name, max_rel_l1=max(errs), noise32=noise32, worst_band=band[0], worst_band_at=band[1],
           f32_restatement_band=band32, band_bar=bar, **kv)
    print("deeplift_%s %s: rel_l1 %.3e noise32 %.3e band %.3e (bar %.3e)" % (name, kv, max(errs), noise32, band[0], bar))
    assert noise32 <= NOISE_MAX, noise32
    assert np.isfinite(out).all()
    assert max(errs) < max(TOL, 3 * noise32), (errs, noise32)
    assert band[0] < bar, (band, bar)


# ------------------------------------------------------------------------------------------------------- 1. whole walk
@pytest.mark.parametrize("approx", [True, False], ids=["mode2", "mode1"])
@pytest.mark.parametrize("kind", KINDS)
def test_walk_matches_the_literal_graph(kind, approx):
    c = _case(kind)
    _check_draw(kind, c)
    eng = _engine(CFG, 16, c["w"], 3, 6)
    eng.set_deeplift_reference(c["ref"], approx)
    eng.encode_images(c["X"])
    out = eng.cnn_walk(IDX, c["head"], "deeplift").cpu().numpy()
    _check("walk", out, c["refs"][approx], c["refs32"][approx], kind=kind, approx=approx)


# ------------------------------------------------------------------------------------------------------- 2. operator
OP_CASES = [(3, 16, False, 9, 11), (16, 16, True, 10, 14), (32, 64, False, 13, 16), (64, 128, True, 16, 12)]


@pytest.mark.parametrize("approx", [True, False], ids=["mode2", "mode1"])
@pytest.mark.parametrize("cin,cout,pool,H,W", OP_CASES)
def test_op_deeplift_conv_against_float64(cin, cout, pool, H, W, approx):
    from lrp_imagecaptioning_amd.engine import op_deeplift_conv
    NB = 2
    rs = np.random.RandomState(cin + cout + H + 7 * int(pool))
    x = rs.standard_normal((NB, H, W, cin)).astype(np.float32)
    xr = rs.standard_normal((H, W, cin)).astype(np.float32)
    x[0, 1:7, 2:8] = xr[1:7, 2:8]                          # exact dX == 0 on a 6 x 6 region: dY == 0 on its 4 x 4 interior
    x[1, :, :, 0] = xr[:, :, 0]                            # ... and on one whole input channel of the other image
    d = 2 if pool else 1
    a = rs.standard_normal((NB, H // d, W // d, cout)).astype(np.float32)
    w = (rs.standard_normal((3, 3, cin, cout)) / np.sqrt(9 * cin)).astype(np.float32)
    b = (0.1 * rs.standard_normal(cout)).astype(np.float32)
    tx, txr, ta = torch.as_tensor(x), torch.as_tensor(xr), torch.as_tensor(a)
    ref, mag = DL.op_deeplift_conv_ref(tx, txr, ta, w, b, pool, approx, torch.float64)
    y, yr = (DL._fused(("conv", w, b), torch.float64)(C._nchw(t.double())) for t in (tx, txr[None]))
    assert int(((y[0] > 0) & (y[0] == yr[0])).sum()) > 0 and int((tx == txr).sum()) >= 6 * 6 * cin   # the forced elements are there
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.backends.mkldnn.flags(enabled=False):
            ref32, _ = DL.op_deeplift_conv_ref(tx, txr, ta, w, b, pool, approx, torch.float32)
    finally:
        torch.set_num_threads(nt)
    out = op_deeplift_conv(tx.cuda(), txr.cuda(), ta.cuda(), w, b, pool=pool, approximate_gradient=approx).cpu()
    assert out.shape == ref.shape and bool(torch.isfinite(out).all())
    r32 = elem_ratio(ref32, ref, mag)
    bar = elem_bar(r32, split=False)
    ratio = elem_ratio(out, ref, mag)
    err = float((out.double() - ref).abs().sum() / ref.abs().sum())
    report("deeplift_op", cin=cin, cout=cout, pool=pool, approx=approx, ratio=ratio, r32=r32, bar=bar, rel_l1=err)
    print("deeplift_op %d->%d pool %d approx %d: ratio %.3e r32 %.3e bar %.3e rel_l1 %.3e" % (cin, cout, pool, approx, ratio, r32, bar, err))
    assert ratio < bar, (ratio, r32, bar)


# ------------------------------------------------------------------------------------------------------- 3. invariance and state
def test_one_image_equals_its_place_in_a_batch():
    c = _case("patch")
    eng = _engine(CFG, 16, c["w"], 3, 6)
    for approx in (True, False):
        eng.set_deeplift_reference(c["ref"], approx)
        eng.encode_images(c["X"])
        batch = eng.cnn_walk(IDX, c["head"], "deeplift").clone()
        for b in range(3):
            eng.encode_images(c["X"][b:b + 1])
            rows = [i for i, v in enumerate(IDX) if v == b]
            one = eng.cnn_walk([0] * len(rows), c["head"][rows], "deeplift")
            assert torch.equal(one, batch[rows]), (approx, b)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_other_walks_do_not_see_the_reference(prec):
    c = _case("patch")
    plain = _engine(CFG, 16, c["w"], 3, 6, prec)
    plain.encode_images(c["X"])
    eng = _engine(CFG, 16, c["w"], 3, 6, prec)
    eng.set_deeplift_reference(c["ref"], True)
    eng.encode_images(c["X"])
    assert torch.equal(eng.get_features(), plain.get_features())
    for walk in ("lrp", "gradient", "input_x_gradient", "guided_backprop", "deconvnet"):
        assert torch.equal(eng.cnn_walk(IDX, c["head"], walk), plain.cnn_walk(IDX, c["head"], walk)), walk
    assert torch.equal(eng.cnn_explain(IDX, c["head"].reshape(6, 16, 64)), plain.cnn_explain(IDX, c["head"].reshape(6, 16, 64)))


def test_workspace_grows_with_the_first_reference_only():
    c = _case("scalar1")
    eng = _engine(CFG, 16, c["w"], 3, 6)
    ws0 = eng.workspace_bytes
    eng.set_deeplift_reference(0, None)                    # off on a handle that never had one: nothing
    eng.encode_images(c["X"])
    eng.cnn_walk(IDX, c["head"], "gradient")
    assert eng.workspace_bytes == ws0
    eng.set_deeplift_reference(1.0, False)                 # one chain: gates and reference activations
    ws1 = eng.workspace_bytes
    assert ws1 > ws0
    eng.set_deeplift_reference(1.0, True)                  # two chains: their ping-pong on top
    ws2 = eng.workspace_bytes
    assert ws2 > ws1
    eng.encode_images(c["X"])
    eng.cnn_walk(IDX, c["head"], "deeplift")
    eng.set_deeplift_reference(1.0, True)                  # the same setting again: nothing, the caches stay
    eng.cnn_walk(IDX, c["head"], "deeplift")
    eng.set_deeplift_reference(0, None)                    # idle afterwards
    eng.set_deeplift_reference(2.0, True)
    assert eng.workspace_bytes == ws2


def test_state_and_unsupported():
    from lrp_imagecaptioning_amd import _capi as CA
    c = _case("scalar1")
    eng = _engine(CFG, 16, c["w"], 3, 6)
    eng.encode_images(c["X"])
    hd = torch.as_tensor(c["head"]).cuda().reshape(6, 16, 64).contiguous()
    out = torch.empty((6, 16, 16, 3), device="cuda")
    idx = (CA.C.c_int32 * 6)(*IDX)

    def walk_rc():
        return eng._lib.lrp_cnn_walk(eng._h, 6, idx, CA.C.c_void_p(hd.data_ptr()), CA.C.c_void_p(out.data_ptr()), 5, eng._stream())

    assert walk_rc() == CA.LRP_ERR_STATE                   # no reference
    with pytest.raises(RuntimeError):
        eng.cnn_walk(IDX, c["head"], "deeplift")
    eng.set_deeplift_reference(1.0, True)
    assert walk_rc() == CA.LRP_ERR_STATE                   # ... and no encode since it was set
    eng.encode_images(c["X"])
    assert walk_rc() == CA.LRP_OK
    first = out.clone()
    eng.set_deeplift_reference(2.0, True)                  # a changed reference drops the caches
    assert walk_rc() == CA.LRP_ERR_STATE
    with pytest.raises(RuntimeError):
        eng.cnn_walk(IDX, c["head"], "deeplift")
    eng.encode_images(c["X"])
    assert walk_rc() == CA.LRP_OK and not torch.equal(out, first)
    eng.set_deeplift_reference(1.0, True)
    eng.encode_images(c["X"])
    assert walk_rc() == CA.LRP_OK and torch.equal(out, first)
    # new weights make the reference's activations stale: the next encode recomputes them
    w2 = DL.dyadic_vgg_weights(np.random.RandomState(99), CFG)
    eng.set_weights(w2)
    eng.encode_images(c["X"])
    fresh = _engine(CFG, 16, w2, 3, 6)
    fresh.set_deeplift_reference(1.0, True)
    fresh.encode_images(c["X"])
    assert torch.equal(eng.cnn_walk(IDX, c["head"], "deeplift"), fresh.cnn_walk(IDX, c["head"], "deeplift"))
    for prec in ("bf16x3", "bf16x3_fast", "f16x2"):        # dY of fp16-pair activations means nothing where it is small
        eng.set_precision(prec)
        eng.encode_images(c["X"])
        assert walk_rc() == CA.LRP_ERR_UNSUPPORTED, prec
        with pytest.raises(NotImplementedError):
            eng.cnn_walk(IDX, c["head"], "deeplift")
    with pytest.raises(ValueError):
        CA.check(eng._lib.lrp_set_deeplift_reference(eng._h, None, 0.0, 3))
    with pytest.raises(TypeError):
        eng.cnn_walk_augmented(c["X"], c["head"][:3].reshape(3, 16, 64), "deeplift", "gaussian", 2)


def test_resnet_handle_refuses():
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import resnet_weights
    stacks, stem, hw = ((4, 2), (8, 2)), 8, 32
    side = hw // 4 // 2
    eng = LRPEngine(decoder="gridtd", img_hw=(hw, hw), L=side * side, D=4 * stacks[-1][0], H=32, E=32, V=50, max_images=1,
                    max_tokens=1, max_caption_len=6, resnet={"stem": stem, "stacks": stacks})
    rs = np.random.RandomState(0)
    eng.set_weights(resnet_weights(rs, stacks, stem=stem, bias_std=0.2))
    eng.set_precision("fp32")
    with pytest.raises(NotImplementedError):
        eng.set_deeplift_reference(0.0, True)
    eng.encode_images(rs.uniform(-120, 130, size=(1, hw, hw, 3)).astype(np.float32))
    with pytest.raises(NotImplementedError):
        eng.cnn_walk([0], rs.standard_normal((1, side * side, 4 * stacks[-1][0])).astype(np.float32), "deeplift")


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_fine_tune_step_does_not_see_a_reference(prec):
    import test_gpu_train as TT
    w, X, cap_in, y, lw, masks = TT._case(3)
    ref = TT._engine(w, len(X))
    ref.set_precision(prec)
    ref.train_begin(lr=1e-3, clipvalue=0.01)
    ref.encode_images(X)
    g_ref, l_ref = ref.train_step(cap_in, y, lw, masks)
    g_ref, l_ref = g_ref.clone(), l_ref.clone()
    eng = TT._engine(w, len(X))
    eng.set_precision(prec)
    eng.set_deeplift_reference(0.25, True)
    eng.train_begin(lr=1e-3, clipvalue=0.01)
    eng.encode_images(X)
    g, l = eng.train_step(cap_in, y, lw, masks)
    assert float(g_ref.abs().sum()) > 0
    assert torch.equal(g, g_ref) and torch.equal(l, l_ref)
    # ... and with the reference set after the step began
    ref.set_deeplift_reference(0.25, True)
    ref.encode_images(X)
    g2, l2 = ref.train_step(cap_in, y, lw, masks)
    assert torch.equal(g2, g_ref) and torch.equal(l2, l_ref)


# ------------------------------------------------------------------------------------------------------- 4. full size
def test_vgg16_full_size_is_finite_and_batch_invariant():
    rs = np.random.RandomState(len(VGG16_CFG) + 224)
    w = vgg_weights(rs, VGG16_CFG, bias_std=0.05)
    X = rs.uniform(-120, 130, size=(2, 224, 224, 3)).astype(np.float32)
    head = rs.standard_normal((2, 14, 14, 512)).astype(np.float32)
    eng = _engine(VGG16_CFG, 224, w, 2, 2)
    eng.set_deeplift_reference(0, True)
    eng.encode_images(X)
    both = eng.cnn_walk([0, 1], head, "deeplift").clone()
    assert bool(torch.isfinite(both).all()) and float(both.abs().sum()) > 0
    for b in range(2):
        eng.encode_images(X[b:b + 1])
        assert torch.equal(eng.cnn_walk([0], head[b:b + 1], "deeplift")[0], both[b]), b


# ------------------------------------------------------------------------------------------------------- 5. classes
def test_analyzer_class_equals_the_engine_route():
    from lrp_imagecaptioning_amd import analyzer as A
    c = _case("patch")
    spec = A.ImageModelSpec(c["w"], cnn_cfg=CFG, img_hw=(16, 16))
    for approx in (True, False):
        d = A.DeepLIFT(spec, reference_inputs=c["ref"], approximate_gradient=approx, max_batch=3)
        got = d.analyze([c["X"], c["head"][:3]])
        e = d._engine
        e.encode_images(c["X"])
        np.testing.assert_array_equal(got, e.cnn_walk([0, 1, 2], c["head"][:3].reshape(3, e.L, e.D), "deeplift").cpu().numpy())
        want = DL.deeplift_vgg(c["layers"], c["X"], c["head"][:3], c["ref"], approx)
        assert max(rel_l1(got[i], want[i]) for i in range(3)) < TOL
    with pytest.raises(TypeError):
        A.GaussianSmoother(d)


@pytest.mark.parametrize("dec", ["adaptive", "gridtd"])
def test_explainer_classes(dec):
    import lrp_imagecaptioning_amd.explainers as EX
    from lrp_imagecaptioning_amd import analyzer as A
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, gridtd_weights
    rs = np.random.RandomState(5)
    H, V, hw, L, D = 32, 50, 16, 16, 64
    w = vgg_weights(rs, CFG, bias_std=0.05)
    w.update((adaptive_weights if dec == "adaptive" else gridtd_weights)(rs, L, D, H, H, V))
    spec = EX.CaptionModelSpec(w, img_encoder="vgg16", hidden_dim=H, embedding_dim=H, L=L, D=D, vocab_size=V, cnn_cfg=CFG, img_hw=(hw, hw))
    X = rs.uniform(-120, 130, size=(1, hw, hw, 3)).astype(np.float32)
    cap = [7, 19, 3, 1]
    name = "ExplainImgCaptioning" + ("AdaptiveAttention" if dec == "adaptive" else "GridTD") + "DeepLIFT"
    ex = getattr(EX, name)(spec, None, None, max_caption_length=6, reference_inputs=20.0)
    ex._forward_beam_search((None, X), cap)
    ds = ex._explain_sentence()
    assert len(ds) == len(ex.caption) - 1 >= 1
    d = np.concatenate(ds)
    img = ex._explain_CNN(X, d)
    assert img.shape == (len(ds),) + X.shape[1:] and np.isfinite(img).all() and np.abs(img).sum() > 0
    # the CNN half is the analyzer class on the same weights: to the bit (one image, any batch of heads)
    an = A.DeepLIFT(A.ImageModelSpec(w, cnn_cfg=CFG, img_hw=(hw, hw)), reference_inputs=20.0, max_batch=len(ds))
    np.testing.assert_array_equal(img, an.analyze([np.repeat(X, len(ds), axis=0), d]))
    # the decoder caches of _forward_beam_search were not touched by the CNN half
    np.testing.assert_array_equal(np.concatenate(ex._explain_sentence()), d)


# ------------------------------------------------------------------------------------------------------- 6. DeepTaylor
@pytest.mark.parametrize("bounded", [False, True])
def test_deeptaylor_classes_under_the_rule_tables_bar(bounded):
    """rule_table_cases' TINY draw with a head that is NOT zero on dead top units (the classes mask it as the output ReLU does);
    bar of test_gpu_rule_table._walk_parity: the float32 restatement within 1e-5, rel_l1 < 1e-4, band under band_bar"""
    from lrp_imagecaptioning_amd import analyzer as A
    cfg, hw, B = K.NETS["tiny"]
    w, X, idx, _, layers = K.net("tiny")
    head = np.random.RandomState(2).standard_normal((B,) + C.forward(layers, X).shape[1:]).astype(np.float32)
    bounds = K.BOUNDS if bounded else None
    ref = DL.deeptaylor_vgg(layers, X, head, bounds)
    ref32 = GF.single_thread_float32(DL.deeptaylor_vgg, layers, X, head, bounds)
    own = max(rel_l1(ref32[i], ref[i]) for i in range(B))
    spec = A.ImageModelSpec(w, cnn_cfg=cfg, img_hw=(hw, hw))
    an = A.BoundedDeepTaylor(spec, low=bounds[0], high=bounds[1], max_batch=B) if bounded else A.DeepTaylor(spec, max_batch=B)
    out = an.analyze([X, head])
    errs = [rel_l1(out[i], ref[i]) for i in range(B)]
    bar, band32 = band_bar(ref32, ref)
    band = max(band_rel_l1(out[i], ref[i], where=True) for i in range(B))
    report("deeptaylor", bounded=bounded, max_rel_l1=max(errs), f32_restatement_rel_l1=own, worst_band=band[0], band_bar=bar)
    print("deeptaylor bounded %d: rel_l1 %.3e (float32 restatement %.3e) band %.3e bar %.3e" % (bounded, max(errs), own, band[0], bar))
    assert own < 1e-5
    assert np.isfinite(out).all()
    assert max(errs) < 1e-4, errs
    assert band[0] < bar, (band, bar)
    unmasked = C.analyze(layers, X, head)
    if not bounded:
        assert min(rel_l1(unmasked[i], ref[i]) for i in range(B)) > 10 * 1e-4      # the mask carries a visible share
