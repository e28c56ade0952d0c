"""-m gpu: Deconvnet (lrp_cnn_walk LRP_WALK_DECONVNET), the augment / reduce operators and SmoothGrad / IntegratedGradients on
the device (LRPEngine.cnn_walk_augmented, analyzer.py, explainers.py) against the restatements of tests/gradient_family_ref.py.

Parity bar, the project's: rel_l1 < max(1e-4, 3 x noise32) and the worst image row / column under gpu_util.band_bar, where
noise32 is the float32 restatement's distance from float64 on the same inputs (single thread, torch's own conv kernels);
`noise32 <= 3e-5` is asserted first, so an ill-conditioned draw fails instead of widening the bar.  The seeds were screened on
the CPU with the restated generator and are named here: VGG_SEED, RESNET_SEEDS, AUG_SEED / NOISE_SEED.

A draw with dead channels (a strongly negative bias in front of a pool) has pool windows whose inputs are all zero.  The other
gradient walks multiply what is routed into such a window by a zero ReLU mask; under Deconvnet it survives and must land on the
window's first cell in scan order.  For those draws the tests first assert, on the CPU, that dropping that share moves the
float64 map by more than 10 x the tolerance: otherwise the case would prove nothing."""
import functools

import numpy as np
import pytest
import torch

import gradient_family_ref as GF
import resnet_grad_ref as RG
from conftest import rel_l1
from gpu_util import band_bar, band_rel_l1, report
from lrp_imagecaptioning_amd.synthetic import RESNET101_STACKS, VGG16_CFG, resnet_weights, vgg_weights
from oracle import cnn_lrp_ref as C

pytestmark = pytest.mark.gpu
TOL, NOISE_MAX = 1e-4, 3e-5
CFG = [("c1", 3, 16, False), ("c2", 16, 16, True), ("c3", 16, 32, False), ("c4", 32, 32, True), ("c5", 32, 64, False)]
VGG_SEED = 21
RESNETS = {"tiny": (((4, 2), (8, 2)), 8, 32),                  # widths % 8 != 0
           "mid": (((8, 2), (16, 3), (32, 2)), 16, 64),
           "stem64": (((32, 2), (64, 2)), 64, 96)}             # 64-channel stem: the fused stem reverse, ragged patches
RESNET_SEEDS = {"tiny": 3, "mid": 3, "stem64": 3}
AUG_SEED, NOISE_SEED = 5, 1234
PRECS = ("fp32", "bf16x3", "f16x2")


def _check(name, out, ref, ref32, **kv):
    n = len(out)
    noise32 = max(rel_l1(ref32[i], ref[i]) for i in range(n))
    bar, band32 = band_bar(ref32, ref)
    errs = [rel_l1(out[i], ref[i]) for i in range(n)]
    band = max(band_rel_l1(out[i], ref[i], where=True) for i in range(n))
    report("gradient_family_" + name, max_rel_l1=max(errs), noise32=noise32, worst_band=band[0], worst_band_at=band[1],
           f32_restatement_band=band32, band_bar=bar, **kv)
    print("gradient_family_%s %s: rel_l1 %.3e noise32 %.3e band %.3e (bar %.3e)" % (name, kv, max(errs), noise32, band[0], bar))
    assert noise32 <= NOISE_MAX, noise32
    assert np.isfinite(out).all()
    assert max(errs) < max(TOL, 3 * noise32), (errs, noise32)
    assert band[0] < bar, (band, bar)


# ------------------------------------------------------------------------------------------------------- 1. Deconvnet, VGG
def _vgg_engine(cfg, hw, w, nb, ntok, prec="fp32"):
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
def _vgg_case(dead):
    """the five-conv 16 x 16 net, 3 images, 6 heads crossing images; dead: two channels of each pooled layer never fire"""
    rs = np.random.RandomState(VGG_SEED)
    w = vgg_weights(rs, CFG, bias_std=0.05)
    if dead:
        for name in ("c2", "c4"):
            w[name + "_b"] = w[name + "_b"].copy()
            w[name + "_b"][[1, 6]] = -1e3
    layers = C.vgg_layers(w, CFG)
    X = rs.uniform(-120, 130, size=(3, 16, 16, 3)).astype(np.float32)
    idx = [0, 1, 2, 2, 0, 1]
    head = rs.standard_normal((6, 4, 4, 64)).astype(np.float32)
    ref = GF.deconvnet_vgg(layers, X[idx], head)
    ref32 = GF.single_thread_float32(GF.deconvnet_vgg, layers, X[idx], head)
    drop = GF.deconvnet_vgg(layers, X[idx], head, drop_zero_windows=True) if dead else None
    return dict(w=w, layers=layers, X=X, idx=idx, head=head, ref=ref, ref32=ref32, drop=drop)


@pytest.mark.parametrize("dead", [False, True])
def test_deconvnet_vgg(dead):
    c = _vgg_case(dead)
    if dead:
        moved = min(rel_l1(c["drop"][i], c["ref"][i]) for i in range(6))
        assert moved > 10 * TOL, moved                     # all-zero windows carry a visible share of every map
    eng = _vgg_engine(CFG, 16, c["w"], 3, 6)
    for prec in PRECS:
        eng.set_precision(prec)
        eng.encode_images(c["X"])
        out = eng.cnn_walk(c["idx"], c["head"], "deconvnet").cpu().numpy()
        _check("vgg", out, c["ref"], c["ref32"], dead=dead, prec=prec)


def test_deconvnet_vgg16_full_size():
    rs = np.random.RandomState(len(VGG16_CFG) + 224)
    w = vgg_weights(rs, VGG16_CFG, bias_std=0.05)
    layers = C.vgg_layers(w, VGG16_CFG)
    X = rs.uniform(-120, 130, size=(1, 224, 224, 3)).astype(np.float32)
    head = rs.standard_normal((1, 14, 14, 512)).astype(np.float32)
    eng = _vgg_engine(VGG16_CFG, 224, w, 1, 1)
    eng.encode_images(X)
    out = eng.cnn_walk([0], head, "deconvnet").cpu().numpy()
    _check("vgg16", out, GF.deconvnet_vgg(layers, X, head), GF.single_thread_float32(GF.deconvnet_vgg, layers, X, head))


# ------------------------------------------------------------------------------------------------------- 2. Deconvnet, ResNet
def _resnet_engine(stacks, stem, hw, B, ntok, w, prec="fp32"):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    side = hw // 4 // (2 ** (len(stacks) - 1))
    eng = LRPEngine(decoder="gridtd", img_hw=(hw, hw), L=side * side, D=4 * stacks[-1][0], H=32, E=32, V=50, max_images=B,
                    max_tokens=ntok, max_caption_len=6, resnet={"stem": stem, "stacks": stacks})
    eng.set_weights(w)
    eng.set_precision(prec)
    return eng, side


@functools.lru_cache(maxsize=None)
def _resnet_case(name):
    """B = 2, heads [0, 1, 1, 0]; stem channel 2 is dead, so all-zero 3 x 3 windows touch the zero padding"""
    stacks, stem, hw = RESNETS[name]
    rs = np.random.RandomState(RESNET_SEEDS[name])
    w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
    w["conv1_bn_beta"] = w["conv1_bn_beta"].copy()
    w["conv1_bn_beta"][2] = -1e4
    spec = RG.resnet_spec(stacks, stem=stem)
    X = rs.uniform(-120, 130, size=(2, hw, hw, 3)).astype(np.float32)
    idx = [0, 1, 1, 0]
    side = hw // 4 // (2 ** (len(stacks) - 1))
    head = rs.standard_normal((4, side, side, 4 * stacks[-1][0])).astype(np.float32)
    ref = GF.deconvnet_resnet(w, spec, X[idx], head)
    ref32 = GF.single_thread_float32(GF.deconvnet_resnet, w, spec, X[idx], head)
    drop = GF.deconvnet_resnet(w, spec, X[idx], head, drop_zero_windows=True)
    return dict(w=w, spec=spec, X=X, idx=idx, head=head, ref=ref, ref32=ref32, drop=drop, stacks=stacks, stem=stem, hw=hw)


@pytest.mark.parametrize("name", sorted(RESNETS))
def test_deconvnet_resnet(name):
    from lrp_imagecaptioning_amd.engine import switches
    c = _resnet_case(name)
    moved = min(rel_l1(c["drop"][i], c["ref"][i]) for i in range(4))
    assert moved > 10 * TOL, moved
    eng, _ = _resnet_engine(c["stacks"], c["stem"], c["hw"], 2, 4, c["w"])
    for prec in PRECS:                                     # no ReLU decision is read: every mode
        eng.set_precision(prec)
        eng.encode_images(c["X"])
        out = eng.cnn_walk(c["idx"], c["head"], "deconvnet").cpu().numpy()
        _check("resnet_" + name, out, c["ref"], c["ref32"], prec=prec)
        if name == "stem64":                               # the two-kernel stem (GEMM + stencil) as well
            with switches(LRP_IMG_FUSED="0"):
                out2 = eng.cnn_walk(c["idx"], c["head"], "deconvnet").cpu().numpy()
            _check("resnet_stem64_two_kernel", out2, c["ref"], c["ref32"], prec=prec)


def test_deconvnet_resnet101_full_size():
    rs = np.random.RandomState(0)
    w = resnet_weights(rs)
    spec = RG.resnet_spec()
    X = rs.uniform(-120, 130, size=(1, 224, 224, 3)).astype(np.float32)
    head = rs.standard_normal((1, 7, 7, 2048)).astype(np.float32)
    eng, _ = _resnet_engine(RESNET101_STACKS, 64, 224, 1, 1, w)
    eng.encode_images(X)
    out = eng.cnn_walk([0], head, "deconvnet").cpu().numpy()
    _check("resnet101", out, GF.deconvnet_resnet(w, spec, X, head), GF.single_thread_float32(GF.deconvnet_resnet, w, spec, X, head))


# ------------------------------------------------------------------------------------------------------- 3. properties
def _property_engines():
    c, r = _vgg_case(True), _resnet_case("mid")
    yield "vgg", _vgg_engine(CFG, 16, c["w"], 3, 6), c["X"], c["head"][:3]
    yield "resnet", _resnet_engine(r["stacks"], r["stem"], r["hw"], 2, 4, r["w"])[0], r["X"], r["head"][:2]


def test_deconvnet_properties():
    for kind, eng, X, h in _property_engines():
        B = len(X)
        idx = list(range(B))
        eng.encode_images(X)
        before = {wk: eng.cnn_walk(idx, h, wk).clone() for wk in ("gradient", "input_x_gradient", "guided_backprop")}
        d = eng.cnn_walk(idx, h, "deconvnet").clone()
        assert torch.equal(eng.cnn_walk(idx, 2 * h, "deconvnet"), 2 * d), kind            # positively homogeneous, exact for 2
        assert (eng.cnn_walk(idx, np.zeros_like(h), "deconvnet") == 0).all(), kind
        for wk, v in before.items():                                                       # the other walks are not disturbed
            assert torch.equal(eng.cnn_walk(idx, h, wk), v), (kind, wk)
        for n in range(B):                                                                 # alone == in the batch, bit for bit
            eng.encode_images(X[n:n + 1])
            assert torch.equal(eng.cnn_walk([0], h[n:n + 1], "deconvnet"), d[n:n + 1]), (kind, n)


def test_deconvnet_is_guided_backprop_when_every_relu_is_on():
    rs = np.random.RandomState(2)
    w = {k: np.abs(v) for k, v in vgg_weights(rs, CFG, bias_std=0.05).items()}
    X = np.abs(rs.uniform(-120, 130, size=(2, 16, 16, 3))).astype(np.float32)
    h = rs.standard_normal((2, 4, 4, 64)).astype(np.float32)
    eng = _vgg_engine(CFG, 16, w, 2, 2)
    eng.encode_images(X)
    d, g = eng.cnn_walk([0, 1], h, "deconvnet").cpu().numpy(), eng.cnn_walk([0, 1], h, "guided_backprop").cpu().numpy()
    assert rel_l1(d, g) < 1e-6
    stacks, stem, hw = RESNETS["tiny"]
    wr = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
    wp = {k: (np.abs(v) if k.endswith(("_conv_W", "_conv_b", "_bn_gamma", "_bn_beta")) else np.zeros_like(v) if k.endswith("_bn_mean") else v)
          for k, v in wr.items()}
    Xr = np.abs(rs.uniform(-120, 130, size=(2, hw, hw, 3))).astype(np.float32)
    er, side = _resnet_engine(stacks, stem, hw, 2, 2, wp)
    hr = rs.standard_normal((2, side, side, 4 * stacks[-1][0])).astype(np.float32)
    er.encode_images(Xr)
    d, g = er.cnn_walk([0, 1], hr, "deconvnet").cpu().numpy(), er.cnn_walk([0, 1], hr, "guided_backprop").cpu().numpy()
    assert rel_l1(d, g) < 1e-6


# ------------------------------------------------------------------------------------------------------- 4. augment_gaussian
def test_op_augment_gaussian():
    from lrp_imagecaptioning_amd.engine import op_augment_gaussian
    rs = np.random.RandomState(0)
    per, sigma, seed = 105, 2.5, (7 << 32) + 11            # 105: a tail group of one value
    x = torch.as_tensor(rs.standard_normal((5, 7, 5, 3)).astype(np.float32)).cuda()
    full = op_augment_gaussian(x, 2, sigma, seed)
    assert full.shape == (10, 7, 5, 3)
    parts = torch.cat([op_augment_gaussian(x, 2, sigma, seed, r0, c) for r0, c in ((0, 3), (3, 3), (6, 3), (9, 1))])
    assert torch.equal(parts, full)
    # the noise of row r is the same whatever B and n are: row 3 is sample 1 of image 1 at n = 2, sample 0 of image 1 at n = 3
    x0 = torch.zeros_like(x)
    a = op_augment_gaussian(x0, 2, sigma, seed)
    b = op_augment_gaussian(x0[:4], 3, sigma, seed)
    assert torch.equal(a, b[:10])
    assert not torch.equal(a, op_augment_gaussian(x0, 2, sigma, seed + 1))
    assert not torch.equal(a, op_augment_gaussian(x0, 2, sigma, seed + (1 << 32)))
    # against the numpy restatement: |z| <= 5.9 and ulp(8) = 9.5e-7, so 1e-5 sigma is about ten ulp of the largest value
    z = GF.gaussian_noise(seed, np.arange(10), per)
    assert np.abs(a.cpu().numpy().reshape(10, per).astype(np.float64) - sigma * z).max() <= 1e-5 * sigma
    want = np.repeat(x.cpu().numpy().reshape(5, per).astype(np.float64), 2, axis=0) + sigma * z
    assert np.abs(full.cpu().numpy().reshape(10, per) - want).max() <= 1e-5 * sigma + 2.0 ** -22     # (+ the sum's own rounding)
    # moments over 2^20 values
    N = 1 << 20
    zs = op_augment_gaussian(torch.zeros((4, N // 16), device="cuda"), 4, 1.0, 99).double().reshape(-1)
    assert zs.numel() == N
    assert abs(float(zs.mean())) <= 5 / np.sqrt(N)
    assert abs(float(zs.var(unbiased=False)) - 1) <= 5 * np.sqrt(2.0 / N)
    p = 0.0026997960632601866                               # P(|z| > 3)
    assert abs(float((zs.abs() > 3).double().mean()) - p) <= 5 * np.sqrt(p * (1 - p) / N)
    assert float(zs.abs().max()) <= 5.9


# ------------------------------------------------------------------------------------------------------- 5. path / reduce
def _ulp_equal(got, want64):
    """got (float32) is want64 rounded to float32, up to one more rounding"""
    w = want64.astype(np.float32)
    return np.all(np.abs(got.astype(np.float64) - want64) <= np.spacing(np.abs(w)).astype(np.float64))


def test_op_augment_path_and_reduce_mean():
    from lrp_imagecaptioning_amd.engine import op_augment_path, op_reduce_accumulate, op_reduce_finish
    rs = np.random.RandomState(1)
    B, n, shape = 5, 2, (7, 5, 3)
    x = rs.standard_normal((B,) + shape).astype(np.float32)
    rt = rs.standard_normal((B,) + shape).astype(np.float32)
    xd = torch.as_tensor(x).cuda()
    chunks = ((0, 3), (3, 3), (6, 3), (9, 1))
    for ref in (0, 0.75, rt):
        for path in ("reference", "standard"):
            got = op_augment_path(xd, n, ref, path)
            want = GF.python_based_augment_path(x, n, np.float32(ref) if np.isscalar(ref) else ref, standard=path == "standard")
            assert want.dtype == np.float32
            if path == "reference":
                np.testing.assert_array_equal(got.cpu().numpy(), want)                      # numpy's own float32 steps
            else:
                want64 = GF.python_based_augment_path(x.astype(np.float64), n, np.float64(ref) if np.isscalar(ref) else ref.astype(np.float64),
                                                      standard=True)
                assert np.abs(got.cpu().numpy() - want64).max() <= 3 * 2.0 ** -24 * np.abs(want64).max() + 1e-7
            parts = torch.cat([op_augment_path(xd, n, ref, path, r0, c) for r0, c in chunks])
            assert torch.equal(parts, got)
    maps = rs.standard_normal((B * n,) + shape).astype(np.float32)
    md = torch.as_tensor(maps).cuda()
    post_np = {None: lambda v: v, "abs": np.abs, "square": np.square}
    for post in (None, "abs", "square"):
        acc = op_reduce_accumulate(md, torch.zeros((B,) + shape, dtype=torch.float64, device="cuda"), n, 0, post)
        acc2 = torch.zeros_like(acc)
        for r0, c in chunks:
            op_reduce_accumulate(md[r0:r0 + c], acc2, n, r0, post)
        assert torch.equal(acc, acc2), post
        m64 = post_np[post](maps.astype(np.float64))
        assert _ulp_equal(op_reduce_finish(acc, n).cpu().numpy(), GF.python_based_reduce_base(m64, n))
        for ref in (0, 0.75, rt):
            r64 = np.float64(ref) if np.isscalar(ref) else ref.astype(np.float64)
            got = op_reduce_finish(acc, n, xd, ref).cpu().numpy()
            assert _ulp_equal(got, GF.python_based_reduce_path(m64, n, x.astype(np.float64), r64)), (post, np.isscalar(ref))


# ------------------------------------------------------------------------------------------------------- 6. SmoothGrad / IG
N_AUG, SIGMA = 5, 8.0


@functools.lru_cache(maxsize=None)
def _aug_net(kind):
    rs = np.random.RandomState(AUG_SEED)
    if kind == "vgg":
        w = vgg_weights(rs, CFG, bias_std=0.05)
        hw, top = 16, (4, 4, 64)
        ref_fn = lambda mode: (lambda S, Hd, dtype=torch.float64: (
            GF.deconvnet_vgg(C.vgg_layers(w, CFG), S, Hd, dtype) if mode == "deconvnet" else
            C.analyze(C.vgg_layers(w, CFG), S, Hd, dtype) if mode == "lrp" else
            C.gradient_analyze(C.vgg_layers(w, CFG), S, Hd, mode, dtype)))
        model = dict(cnn_cfg=CFG, img_hw=(16, 16))
    else:
        stacks, stem, hw = RESNETS["tiny"]
        w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
        spec = RG.resnet_spec(stacks, stem=stem)
        top = (4, 4, 4 * stacks[-1][0])
        ref_fn = lambda mode: (lambda S, Hd, dtype=torch.float64: (
            GF.deconvnet_resnet(w, spec, S, Hd, dtype) if mode == "deconvnet" else RG.gradient_analyze(w, spec, S, Hd, mode, dtype)))
        model = dict(img_hw=(hw, hw), resnet={"stem": stem, "stacks": stacks})
    X = rs.uniform(-120, 130, size=(2, hw, hw, 3)).astype(np.float32)
    head = rs.standard_normal((2,) + top).astype(np.float32)
    return w, model, X, head, ref_fn


def _spec(kind):
    from lrp_imagecaptioning_amd import analyzer as A
    w, model, X, head, ref_fn = _aug_net(kind)
    return A.ImageModelSpec(w, **model)


def _reference_image(X):
    return np.random.RandomState(AUG_SEED + 1).uniform(-60, 60, size=X.shape).astype(np.float32)


def _samples(kind, X, **kw):
    """the sample matrix, downloaded from the augment operator"""
    from lrp_imagecaptioning_amd.engine import op_augment_gaussian, op_augment_path
    xd = torch.as_tensor(X).cuda()
    if kind == "gaussian":
        return op_augment_gaussian(xd, N_AUG, SIGMA, NOISE_SEED).cpu().numpy()
    return op_augment_path(xd, N_AUG, kw.get("reference", 0), kw.get("path", "reference")).cpu().numpy()


def _reduced(ref_fn, mode, S, head, X, post, factor, dtype):
    """the float64 (or float32) restatement on the samples S: per-sample map, post-processing, mean, factor"""
    Hd = np.repeat(head, N_AUG, axis=0)
    maps = ref_fn(mode)(S, Hd, dtype=dtype).astype(np.float64)
    if mode == "input_x_gradient":
        pass                                               # (the restatement multiplied with the sample it was given)
    maps = {None: lambda v: v, "abs": np.abs, "square": np.square}[post](maps)
    out = GF.python_based_reduce_base(maps, N_AUG)
    return out * factor if factor is not None else out


@pytest.mark.parametrize("kind", ["vgg", "resnet"])
def test_smoothgrad_and_integrated_gradients_parity(kind):
    from lrp_imagecaptioning_amd import analyzer as A
    w, model, X, head, ref_fn = _aug_net(kind)
    spec = _spec(kind)
    for post in (None, "abs", "square"):
        S = _samples("gaussian", X)
        ref = _reduced(ref_fn, "gradient", S, head, X, post, None, torch.float64)
        ref32 = GF.single_thread_float32(lambda dtype: _reduced(ref_fn, "gradient", S, head, X, post, None, dtype))
        a3 = A.SmoothGrad(spec, augment_by_n=N_AUG, postprocess=post, noise_scale=SIGMA, seed=NOISE_SEED, max_batch=3)
        out3 = a3.analyze([X, head])                       # ragged chunks 3, 3, 3, 1 that cross the image boundary
        _check("smoothgrad_" + kind, out3, ref, ref32, post=str(post))
        a10 = A.SmoothGrad(spec, augment_by_n=N_AUG, postprocess=post, noise_scale=SIGMA, seed=NOISE_SEED, max_batch=10)
        np.testing.assert_array_equal(a10.analyze([X, head]), out3)
        # (the standard path starts AT the reference: a constant image there would tie every pool window of sample 0)
        for path, rv in (("reference", 0), ("standard", _reference_image(X))):
            S = _samples("path", X, reference=rv, path=path)
            fac = X.astype(np.float64) - rv
            ref = _reduced(ref_fn, "gradient", S, head, X, post, fac, torch.float64)
            ref32 = GF.single_thread_float32(lambda dtype: _reduced(ref_fn, "gradient", S, head, X, post, fac, dtype))
            i3 = A.IntegratedGradients(spec, steps=N_AUG, postprocess=post, reference_inputs=rv, path=path, max_batch=3)
            o3 = i3.analyze([X, head])
            _check("ig_" + kind, o3, ref, ref32, post=str(post), path=path)
            i10 = A.IntegratedGradients(spec, steps=N_AUG, postprocess=post, reference_inputs=rv, path=path, max_batch=10)
            np.testing.assert_array_equal(i10.analyze([X, head]), o3)


@pytest.mark.parametrize("kind", ["vgg", "resnet"])
def test_wrappers_over_other_analyzers(kind):
    from lrp_imagecaptioning_amd import analyzer as A
    w, model, X, head, ref_fn = _aug_net(kind)
    spec = _spec(kind)
    # one step at reference 0 is the input itself: x * gradient(x)
    itg = A.InputTimesGradient(spec).analyze([X, head])
    one = A.PathIntegrator(A.Gradient(spec), steps=1, reference_inputs=0).analyze([X, head])
    assert rel_l1(one, itg) < 1e-6
    S = _samples("gaussian", X)
    subs = [(A.GuidedBackprop, "guided_backprop"), (A.Deconvnet, "deconvnet"), (A.InputTimesGradient, "input_x_gradient")]
    if kind == "vgg":
        subs.append((A.LRPSequentialPresetA, "lrp"))
    for cls, mode in subs:
        hd = head if mode != "lrp" else (head * C.forward(C.vgg_layers(w, CFG), X)).astype(np.float32)
        ref = _reduced(ref_fn, mode, S, hd, X, None, None, torch.float64)
        ref32 = GF.single_thread_float32(lambda dtype: _reduced(ref_fn, mode, S, hd, X, None, None, dtype))
        out = A.GaussianSmoother(cls(spec, max_batch=4), augment_by_n=N_AUG, noise_scale=SIGMA, seed=NOISE_SEED).analyze([X, hd])
        _check("smoother_" + kind, out, ref, ref32, sub=mode)


# ------------------------------------------------------------------------------------------------------- 7. surface
@pytest.mark.parametrize("kind", ["vgg", "resnet"])
def test_analyzer_classes_equal_the_engine_route(kind):
    from lrp_imagecaptioning_amd import analyzer as A
    w, model, X, head, ref_fn = _aug_net(kind)
    spec = _spec(kind)
    d = A.Deconvnet(spec)
    e = d._engine
    got = d.analyze([X, head])
    e.encode_images(X)
    np.testing.assert_array_equal(got, e.cnn_walk([0, 1], head.reshape(2, e.L, e.D), "deconvnet").cpu().numpy())
    sg = A.SmoothGrad(spec, augment_by_n=N_AUG, noise_scale=SIGMA, seed=NOISE_SEED, max_batch=4)
    eng = sg._subanalyzer._engine
    want = eng.cnn_walk_augmented(X, head.reshape(2, eng.L, eng.D), "gradient", "gaussian", N_AUG, noise_scale=SIGMA, seed=NOISE_SEED)
    assert eng.n_images == 0 and eng.captions is None
    np.testing.assert_array_equal(sg.analyze([X, head]), want.cpu().numpy())
    ig = A.analyzers["integrated_gradients"](spec, steps=N_AUG, reference_inputs=20.0, path="standard", max_batch=4)
    eng = ig._subanalyzer._engine
    want = eng.cnn_walk_augmented(X, head.reshape(2, eng.L, eng.D), "gradient", "path", N_AUG, reference=20.0, path="standard")
    np.testing.assert_array_equal(ig.analyze([X, head]), want.cpu().numpy())


@pytest.mark.parametrize("dec", ["adaptive", "gridtd"])
def test_explainer_classes(dec):
    import lrp_imagecaptioning_amd.explainers as EX
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, gridtd_weights
    rs = np.random.RandomState(AUG_SEED)
    H, V, hw, L, D = 32, 50, 16, 16, 64
    w = vgg_weights(rs, CFG, bias_std=0.05)
    w.update((adaptive_weights if dec == "adaptive" else gridtd_weights)(rs, L, D, H, H, V))
    spec = EX.CaptionModelSpec(w, img_encoder="vgg16", hidden_dim=H, embedding_dim=H, L=L, D=D, vocab_size=V, cnn_cfg=CFG, img_hw=(hw, hw))
    X = rs.uniform(-120, 130, size=(1, hw, hw, 3)).astype(np.float32)
    cap = [7, 19, 3, 1]
    layers = C.vgg_layers(w, CFG)
    stem = "ExplainImgCaptioning" + ("AdaptiveAttention" if dec == "adaptive" else "GridTD")
    from lrp_imagecaptioning_amd.engine import op_augment_gaussian, op_augment_path
    xd = torch.as_tensor(X).cuda()
    for suffix, kw in (("Deconvnet", {}), ("SmoothGrad", dict(augment_by_n=N_AUG, noise_scale=SIGMA, seed=NOISE_SEED, max_batch=3)),
                       ("IntegratedGradients", dict(steps=N_AUG, reference_inputs=_reference_image(X), path="standard", max_batch=3))):
        ex = getattr(EX, stem + suffix)(spec, None, None, max_caption_length=6, **kw)
        ex._forward_beam_search((None, X), cap)
        d = ex._lstm_decoder_backward(2)
        img = ex._explain_CNN(X, d)
        assert img.shape == X.shape
        if suffix == "Deconvnet":
            ref = GF.deconvnet_vgg(layers, X, d)
            ref32 = GF.single_thread_float32(GF.deconvnet_vgg, layers, X, d)
        else:
            S = (op_augment_gaussian(xd, N_AUG, SIGMA, NOISE_SEED) if suffix == "SmoothGrad" else
                 op_augment_path(xd, N_AUG, _reference_image(X), "standard")).cpu().numpy()
            fac = None if suffix == "SmoothGrad" else X.astype(np.float64) - _reference_image(X)
            f = lambda dtype: GF.python_based_reduce_base(
                C.gradient_analyze(layers, S, np.repeat(d, N_AUG, axis=0), "gradient", dtype).astype(np.float64), N_AUG) * (1 if fac is None else fac)
            ref, ref32 = f(torch.float64), GF.single_thread_float32(f)
        _check("explainer_" + dec, img, ref, ref32, cls=suffix)
        # the decoder caches of _forward_beam_search were not touched by the CNN half
        np.testing.assert_array_equal(ex._lstm_decoder_backward(2), d)
