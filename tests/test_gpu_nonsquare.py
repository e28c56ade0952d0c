"""-m gpu: every encoder path at H != W.  On a square image a kernel that swaps H and W, tiles_x and tiles_y or Ho and Wo
computes the same values, and outside the VGG LRP walk and lrp_op_conv the suite only ever ran squares: here the ResNet
encoder (stem im2col, the overlapping 3x3/2 pool, the stride-2 subsample / scatter / join kernels, the fused and the
two-kernel stem reverse, the pair-emitting forward, the three gradient walks), the VGG gradient walks, the weight-gradient
GEMMs and the fine-tune step run on H x W images with H != W, against the float64 oracles.

Every heat-map is held to two bounds: the whole-map relative L1 of the corresponding square test, and gpu_util.band_rel_l1
— the worst single image row or column — because on a deep encoder a lost border row moves the whole map by less than 1e-4
(tests/test_band_metric.py).  The band bound is max(1e-4, 10 x what the same oracle evaluated in float32 on the CPU scores
against its float64 evaluation): gpu_util.band_bar.  Measured values: profiles/nonsquare_geometry.txt."""
import functools

import numpy as np
import pytest
import torch

import resnet_grad_ref as RG
from conftest import rel_l1
from gpu_util import NONSQUARE_RESNETS, band_bar, band_rel_l1, report, transpose_spatial
from lrp_imagecaptioning_amd.synthetic import adaptive_weights, gridtd_weights, resnet_weights, vgg_weights
from oracle import cnn_lrp_ref as C
from oracle import resnet_lrp_ref as RN

pytestmark = pytest.mark.gpu
TOL = 1e-4
WALKS = ("gradient", "input_x_gradient", "guided_backprop")


# Seeds of the ResNet LRP cases, chosen on the CPU oracle alone (float32 against float64 evaluation, seeds 0 ... 5): the first
# few seeds include draws on which float32 itself is 2e-4 ... 4e-3 off on one low-mass band (a near-zero denominator of the
# rule); on such a draw the band bound would say little about the arithmetic.  With these the restatement's worst band is
# 1e-5 ... 8e-5 (it moves with the CPU's summation order), so the band bound stays within 1e-4 ... 1e-3.
LRP_SEED = {"stem64": 3, "mid": 3, "tiny": 4, "wide": 2}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _check_maps(name, out, ref, bar, tol=TOL, **info):
    """Both bounds for a batch of (H, W, C) maps; bar = (band bound, the float32 restatement's worst band).  Prints and
    reports every figure before it asserts."""
    errs = [rel_l1(o, r) for o, r in zip(out, ref)]
    bands = [band_rel_l1(o, r, where=True) for o, r in zip(out, ref)]
    worst, where = max(bands)
    rec = dict(info, rel_l1=max(errs), worst_band=worst, f32_restatement_band=bar[1], band_bar=bar[0], worst_band_at=where)
    report(name, **rec)
    print(name, rec)
    assert np.isfinite(np.asarray(out)).all()
    assert max(errs) < tol, (name, info, errs)
    assert worst < bar[0], (name, info, bands, bar)


# ---------------------------------------------------------------------------------------------------------- ResNet
def _resnet_engine(stacks, stem, hw, B, ntok, w):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    down = 4 * 2 ** (len(stacks) - 1)
    th, tw, D = hw[0] // down, hw[1] // down, 4 * stacks[-1][0]
    eng = LRPEngine(decoder="gridtd", img_hw=hw, L=th * tw, D=D, H=32, E=32, V=50, max_images=B, max_tokens=ntok,
                    max_caption_len=6, resnet={"stem": stem, "stacks": stacks})
    eng.set_weights(w)
    return eng, (th, tw, D)


@functools.lru_cache(maxsize=None)
def _lrp_case(name, hw):
    """Inputs and the oracle's results of one geometry, computed once and shared read-only: features, the float64 maps and the
    band bound from the float32 evaluation of the same oracle.  Two images, four maps, heads crossing images (`wide`: one
    image, two maps).  A geometry that is not the table's own is its spatial transpose: the table's case with kernels, images
    and relevance transposed, the oracle evaluated on those."""
    stacks, stem, hw0 = NONSQUARE_RESNETS[name]
    B, idx = (1, (0, 0)) if name == "wide" else (2, (0, 1, 1, 0))
    spec = RN.resnet_spec(stacks, stem=stem)
    ix = list(idx)
    if hw == hw0:
        rs = np.random.RandomState(LRP_SEED[name])
        w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
        X = rs.uniform(-120, 130, size=(B,) + hw + (3,)).astype(np.float32)
        feat = RN.forward(w, spec, X)
        R = (rs.standard_normal((len(ix),) + feat.shape[1:]) * feat[ix]).astype(np.float32)
    else:
        assert hw == hw0[::-1]
        c = _lrp_case(name, hw0)
        w = transpose_spatial(c["w"])
        X, R = (np.ascontiguousarray(np.swapaxes(c[k], 1, 2)) for k in ("X", "R"))
        feat = RN.forward(w, spec, X)
    ref = RN.analyze(w, spec, X[ix], R)
    bar = band_bar(RN.analyze(w, spec, X[ix], R, dtype=torch.float32), ref)
    _frozen(X, feat, R, ref, *w.values())
    return dict(stacks=stacks, stem=stem, hw=hw, B=B, idx=ix, w=w, spec=spec, X=X, feat=feat, R=R, ref=ref, bar=bar)


def _run_lrp(eng, c, top):
    eng.encode_images(c["X"])
    feat = eng.get_features().clone()
    out = eng.cnn_explain(c["idx"], c["R"].reshape(len(c["idx"]), top[0] * top[1], top[2])).clone()
    return feat, out


LRP_CASES = [("stem64", (72, 120)), ("stem64", (120, 72)), ("mid", (48, 80)), ("tiny", (24, 40)), ("wide", (160, 96))]


@pytest.mark.parametrize("prec", ["bf16x3", "fp32"])
@pytest.mark.parametrize("name,hw", LRP_CASES, ids=["%s_%dx%d" % (n, h, w_) for n, (h, w_) in LRP_CASES])
def test_resnet_lrp_matches_oracle(name, hw, prec):
    """stem64: stem map 36 x 60 — 3 x 5 (5 x 3) patches of the fused stem reverse, the last ragged in both directions; top
    map 9 x 15, an odd map behind a stride-2 block.  mid: the two-kernel stem, top map 3 x 5.  tiny: widths % 8 != 0, the
    exact-fp32 fallbacks.  wide: channel widths 256 ... 2048 as in ResNet-101, top map 5 x 3."""
    c = _lrp_case(name, hw)
    eng, top = _resnet_engine(c["stacks"], c["stem"], hw, c["B"], len(c["idx"]), c["w"])
    assert top[:2] == c["feat"].shape[1:3] and top[0] != top[1]
    eng.set_precision(prec)
    feat, out = _run_lrp(eng, c, top)
    e_feat = rel_l1(feat.cpu().numpy().reshape(c["feat"].shape), c["feat"])
    _check_maps("nonsquare_resnet_lrp", out.cpu().numpy(), c["ref"], c["bar"], case="%s %dx%d" % ((name,) + hw), prec=prec,
                feat_rel_l1=e_feat)
    assert e_feat < 1e-5


def test_resnet_two_kernel_stem_matches_oracle():
    """LRP_IMG_FUSED=0 on stem64: the stem's reverse as 1-tap GEMM + rn_stem_stencil_kernel, on the 36 x 60 stem map.  The
    two forms add the same products tap by tap, so their maps can agree to the last bit: that the switch took the other
    route shows in the walk's kernel launches."""
    from lrp_imagecaptioning_amd import _capi
    from lrp_imagecaptioning_amd.engine import switches
    lib = _capi.load()
    c = _lrp_case("stem64", (72, 120))
    eng, top = _resnet_engine(c["stacks"], c["stem"], c["hw"], c["B"], 4, c["w"])
    R = c["R"].reshape(4, top[0] * top[1], top[2])

    def walk():
        n0 = int(lib.lrp_launch_count())
        out = eng.cnn_explain(c["idx"], R).cpu().numpy()
        return out, int(lib.lrp_launch_count()) - n0
    for prec in ("bf16x3", "fp32"):
        eng.set_precision(prec)
        eng.encode_images(c["X"])
        _, fused_launches = walk()
        with switches(LRP_IMG_FUSED=0):
            out, launches = walk()
        _check_maps("nonsquare_resnet_lrp_two_kernel_stem", out, c["ref"], c["bar"], case="stem64 72x120", prec=prec,
                    launches=launches, fused_launches=fused_launches)
        assert launches > fused_launches


def test_resnet_pair_emitting_forward_has_a_fallback_and_is_batch_invariant():
    """stem64 at 72 x 120: LRP_FWD_EMIT=0 (split passes between the convs) within the bounds of the square test (1e-5
    features, 2e-5 maps); each image encoded alone on a max_images=1 handle equals its rows in the batch bit for bit,
    features and maps."""
    from lrp_imagecaptioning_amd.engine import switches
    c = _lrp_case("stem64", (72, 120))
    eng, top = _resnet_engine(c["stacks"], c["stem"], c["hw"], c["B"], 4, c["w"])
    one, _ = _resnet_engine(c["stacks"], c["stem"], c["hw"], 1, 2, c["w"])
    feat, out = _run_lrp(eng, c, top)
    with switches(LRP_FWD_EMIT=0):
        feat0, out0 = _run_lrp(eng, c, top)
    e_fb = rel_l1(feat0.cpu().numpy(), feat.cpu().numpy())
    _check_maps("nonsquare_resnet_emit_fallback", out0.cpu().numpy(), out.cpu().numpy(), c["bar"], tol=2e-5,
                case="stem64 72x120", feat_rel_l1=e_fb)
    assert e_fb < 1e-5
    _check_maps("nonsquare_resnet_emit_fallback_vs_oracle", out0.cpu().numpy(), c["ref"], c["bar"], case="stem64 72x120")
    for n in range(c["B"]):
        rows = [i for i, m in enumerate(c["idx"]) if m == n]
        one.encode_images(c["X"][n:n + 1])
        o1 = one.cnn_explain([0] * len(rows), c["R"][rows].reshape(len(rows), top[0] * top[1], top[2]))
        assert torch.equal(one.get_features()[0], feat[n]), n
        assert torch.equal(o1, out[rows]), n


def test_resnet_transposition_on_the_device():
    """No oracle involved: stem64 on spatially transposed kernels, image and relevance returns the transposed heat-map (fp32
    mode; the summation order differs, so not bit for bit: 1e-5, and the band bound).  Continuous random inputs: no pool
    ties."""
    c, ct = _lrp_case("stem64", (72, 120)), _lrp_case("stem64", (120, 72))
    assert rel_l1(ct["w"]["conv1_conv_W"], c["w"]["conv1_conv_W"]) > 1.0
    eng, top = _resnet_engine(c["stacks"], c["stem"], (72, 120), c["B"], 4, c["w"])
    engt, topt = _resnet_engine(c["stacks"], c["stem"], (120, 72), c["B"], 4, ct["w"])
    assert topt == (top[1], top[0], top[2])
    for e in (eng, engt):
        e.set_precision("fp32")
    feat, out = _run_lrp(eng, c, top)
    featt, outt = _run_lrp(engt, ct, topt)
    f = feat.cpu().numpy().reshape((c["B"],) + top)
    ft = np.swapaxes(featt.cpu().numpy().reshape((c["B"],) + topt), 1, 2)
    e_feat = rel_l1(ft, f)
    _check_maps("nonsquare_resnet_device_transposition", np.swapaxes(outt.cpu().numpy(), 1, 2), out.cpu().numpy(), c["bar"],
                tol=1e-5, case="stem64 72x120 vs 120x72", prec="fp32", feat_rel_l1=e_feat)
    assert e_feat < 1e-5


@functools.lru_cache(maxsize=None)
def _grad_case(name):
    stacks, stem, hw = NONSQUARE_RESNETS[name]
    rs = np.random.RandomState(3)
    w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
    spec = RG.resnet_spec(stacks, stem=stem)
    X = rs.uniform(-120, 130, size=(2,) + hw + (3,)).astype(np.float32)
    down = 4 * 2 ** (len(stacks) - 1)
    idx = [0, 1, 1, 0]
    head = rs.standard_normal((4, hw[0] // down, hw[1] // down, 4 * stacks[-1][0])).astype(np.float32)
    ref, bar = {}, {}
    for walk in WALKS:
        ref[walk] = RG.gradient_analyze(w, spec, X[idx], head, walk)
        bar[walk] = band_bar(RG.gradient_analyze(w, spec, X[idx], head, walk, dtype=torch.float32), ref[walk])
    _frozen(X, head, *ref.values())
    return dict(stacks=stacks, stem=stem, hw=hw, w=w, X=X, idx=idx, head=head, ref=ref, bar=bar)


@pytest.mark.parametrize("name,fused", [("stem64", 1), ("stem64", 0), ("mid", 1)], ids=["stem64", "stem64_two_kernel_stem", "mid"])
def test_resnet_gradient_walks_match_oracle(name, fused):
    """Gradient / Input x Gradient / Guided Backprop (LRP_PREC_FP32) at 72 x 120 and 48 x 80, and the two-kernel stem."""
    from lrp_imagecaptioning_amd.engine import switches
    c = _grad_case(name)
    eng, top = _resnet_engine(c["stacks"], c["stem"], c["hw"], 2, 4, c["w"])
    eng.set_precision("fp32")
    eng.encode_images(c["X"])
    with switches(LRP_IMG_FUSED=fused):
        for walk in WALKS:
            out = eng.cnn_walk(c["idx"], c["head"].reshape(4, top[0] * top[1], top[2]), walk).cpu().numpy()
            _check_maps("nonsquare_resnet_grad", out, c["ref"][walk], c["bar"][walk], case="%s %dx%d" % ((name,) + c["hw"]),
                        walk=walk, fused_stem=fused)


# ------------------------------------------------------------------------------------------------------------- VGG
def _vgg_cases():
    from test_gpu_cnn import RAGGED_CFG
    from test_gpu_gradient import CFG
    return {"small_12x20": (CFG, (12, 20), 3), "ragged_60x80": (RAGGED_CFG, (60, 80), 2)}


@pytest.mark.parametrize("case", ["small_12x20", "ragged_60x80"])
def test_vgg_gradient_walks_match_oracle(case):
    """The VGG gradient walks on a 12 x 20 image (3 images, top map 3 x 5) and on the ragged-tile net at 60 x 80 (top map
    15 x 20), all three walks, exact fp32 forward and the default one, two heads per image."""
    from lrp_imagecaptioning_amd.engine import LRPEngine
    cfg, hw, nb = _vgg_cases()[case]
    rs = np.random.RandomState(0)                          # (float32 on the CPU flips no ReLU / arg-max on these draws: 4e-7)
    w = vgg_weights(rs, cfg, bias_std=0.05)
    layers = C.vgg_layers(w, cfg)
    X = rs.uniform(-120, 130, size=(nb,) + hw + (3,)).astype(np.float32)
    h, ww, c = C.forward(layers, X).shape[1:]
    assert (h, ww) == (hw[0] // 4, hw[1] // 4)
    eng = LRPEngine(decoder="adaptive", cnn_cfg=cfg, img_hw=hw, L=h * ww, D=c, H=8, E=8, V=8, max_images=nb, max_tokens=2 * nb,
                    max_caption_len=2)
    eng.set_weights(w)
    idx = list(range(nb)) + list(range(nb))[::-1]
    head = rs.standard_normal((2 * nb, h, ww, c)).astype(np.float32)
    refs = {walk: C.gradient_analyze(layers, X[idx], head, walk) for walk in WALKS}
    bars = {walk: band_bar(C.gradient_analyze(layers, X[idx], head, walk, dtype=torch.float32), refs[walk]) for walk in WALKS}
    for prec in ("fp32", "bf16x3"):
        eng.set_precision(prec)
        eng.encode_images(X)
        for walk in WALKS:
            out = eng.cnn_walk(idx, head, walk).cpu().numpy()
            _check_maps("nonsquare_vgg_grad", out, refs[walk], bars[walk], case=case, walk=walk, prec=prec)


# ------------------------------------------------------------------------------------------------ weight gradients
WGRAD_SHAPES = [(2, 28, 12, 64, 128), (3, 5, 9, 136, 72), (1, 6, 40, 8, 8)]


def _wgrad64(x, dz, bias=True):
    import torch.nn.functional as F
    Cin, Cout = x.shape[3], dz.shape[3]
    w = torch.zeros((Cout, Cin, 3, 3), dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().permute(0, 3, 1, 2), w, b, padding=1).backward(dz.double().permute(0, 3, 1, 2))
    return w.grad.permute(2, 3, 1, 0).numpy(), b.grad.numpy()              # OIHW -> HWIO


def _wgrad_inputs(NB, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(NB + 31 * H + W)
    x = torch.randn((NB, H, W, Cin), generator=g)
    dz = torch.randn((NB, H, W, Cout), generator=g) * (torch.rand((NB, H, W, Cout), generator=g) > 0.5)
    return x, dz


@pytest.mark.parametrize("NB,H,W,Cin,Cout", WGRAD_SHAPES)
def test_conv_wgrad_at_h_ne_w(NB, H, W, Cin, Cout):
    """lrp_op_conv_wgrad: the im2col gather takes gH and gW separately, and only ever got gH == gW.  Against the float64
    autograd gradient, and against itself on the spatially transposed x, dz: dw with its two tap axes transposed."""
    from lrp_imagecaptioning_amd.engine import op_conv_wgrad
    x, dz = _wgrad_inputs(NB, H, W, Cin, Cout)
    want_w, want_b = _wgrad64(x, dz)
    dw, db = op_conv_wgrad(x.cuda(), dz.cuda())
    dwt, dbt = op_conv_wgrad(x.transpose(1, 2).contiguous().cuda(), dz.transpose(1, 2).contiguous().cuda())
    e_w, e_b = rel_l1(dw.cpu().numpy(), want_w), rel_l1(db.cpu().numpy(), want_b)
    e_t = rel_l1(dwt.transpose(0, 1).cpu().numpy(), dw.cpu().numpy())
    e_tb = rel_l1(dbt.cpu().numpy(), db.cpu().numpy())
    report("nonsquare_wgrad", shape=[NB, H, W, Cin, Cout], dw_rel_l1=e_w, db_rel_l1=e_b, transposed_dw_rel_l1=e_t, transposed_db_rel_l1=e_tb)
    print("nonsquare_wgrad", (NB, H, W, Cin, Cout), e_w, e_b, e_t, e_tb)
    assert e_w < 1e-5 and e_b < 1e-5
    assert e_t < 1e-5 and e_tb < 1e-5
    assert rel_l1(np.swapaxes(want_w, 0, 1), want_w) > 0.5                  # (the taps are not symmetric)


@pytest.mark.parametrize("NB,H,W,Cin,Cout", WGRAD_SHAPES)
def test_conv_wgrad_bf16_at_h_ne_w(NB, H, W, Cin, Cout):
    """lrp_op_conv_wgrad_bf16 with the bars of the square test: 2e-5 against the float64 gradient of the bf16-rounded
    operands, 1e-2 against that of the unrounded ones; the bias gradient stays fp32."""
    from lrp_imagecaptioning_amd.engine import op_conv_wgrad
    x, dz = _wgrad_inputs(NB, H, W, Cin, Cout)
    dw, db = op_conv_wgrad(x.cuda(), dz.cuda(), bf16=True)
    dw = dw.cpu().numpy()
    e_r = rel_l1(dw, _wgrad64(x.bfloat16().float(), dz.bfloat16().float())[0])
    want_w, want_b = _wgrad64(x, dz)
    e_u, e_b = rel_l1(dw, want_w), rel_l1(db.cpu().numpy(), want_b)
    report("nonsquare_wgrad_bf16", shape=[NB, H, W, Cin, Cout], vs_rounded=e_r, vs_unrounded=e_u, db_rel_l1=e_b)
    print("nonsquare_wgrad_bf16", (NB, H, W, Cin, Cout), e_r, e_u, e_b)
    assert np.isfinite(dw).all()
    assert e_r < 2e-5
    assert e_u < 1e-2
    assert e_b < 1e-5


# --------------------------------------------------------------------------------------------------- fine-tune step
@pytest.mark.parametrize("kind", ["adaptive", "gridtd"])
def test_fine_tune_step_on_12x20_images(kind):
    """The fine-tune step (trainer.h walks Ly.H, Ly.W) on 12 x 20 images: two pools -> a 3 x 5 map, L = 15; dropout masks on;
    gradients of every parameter and the losses against oracle/train_ref.py with the bars of tests/test_gpu_train.py."""
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from oracle import train_ref as T
    from test_gpu_train import CFG
    hw, L, D, H, V, B, Tn = (12, 20), 15, 16, 16, 40, 3, 5
    rs = np.random.RandomState(17)
    w = vgg_weights(rs, CFG, bias_std=0.3)
    w.update((adaptive_weights if kind == "adaptive" else gridtd_weights)(rs, L, D, H, H, V))
    X = (rs.uniform(0, 255, size=(B,) + hw + (3,)) - 110).astype(np.float32) / 64
    cap_in = np.concatenate([np.full((B, 1), 1), rs.randint(2, V, size=(B, Tn - 1))], axis=1).astype(np.int32)
    y = rs.randint(0, V, size=(B, Tn)).astype(np.int32)
    y[1, -2:] = -1
    lw = (1 + rs.uniform(0, 1, size=(B, Tn, V)) * (rs.uniform(size=(B, Tn, V)) < 0.2)).astype(np.float32)
    mk = lambda *s: ((rs.uniform(size=s) >= 0.5) * 2.0).astype(np.float32)
    masks = {"image_features": mk(B, L, H), "global": mk(B, H), "output": mk(B, Tn, H), "lstm_in": mk(Tn, 4, B, 2 * H),
             "lstm_rec": mk(Tn, 4, B, H)}
    if kind == "gridtd":
        masks["logits"] = mk(B, Tn, V)
    eng = LRPEngine(decoder=kind, cnn_cfg=CFG, img_hw=hw, L=L, D=D, H=H, E=H, V=V, max_images=4, max_tokens=8, max_caption_len=6)
    eng.set_weights(w)
    layout = eng.train_begin(lr=1e-3, clipvalue=0.01)
    assert set(layout) == set(T.param_names(CFG, kind))
    eng.encode_images(X)
    grads, losses = eng.train_step(cap_in, y, lw, masks)
    total, l1, l2, g, _ = T.loss_and_grads(w, CFG, X, cap_in, y, lw, masks, kind=kind)
    gf = grads.cpu().numpy()
    worst = {nm: rel_l1(gf[off:off + n].reshape(g[nm].shape), g[nm]) for nm, (off, n) in layout.items()}
    report("nonsquare_train_step", decoder=kind, worst_grad_rel_l1=max(worst.values()), worst_grad=max(worst, key=worst.get),
           losses=[float(v) for v in losses.cpu().numpy()[:3]], oracle_losses=[total, l1, l2])
    print("nonsquare_train_step", kind, worst, losses.cpu().numpy()[:3], [total, l1, l2])
    np.testing.assert_allclose(losses.cpu().numpy()[:3], [total, l1, l2], rtol=2e-5)
    assert all(np.abs(v).sum() > 0 for v in g.values())
    bad = {k: v for k, v in worst.items() if not v < 2e-4}
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------- refusals
def test_refusals_stay_refusals():
    """What H != W does not support is refused when asked for, with a message, not computed wrongly later: Guided Grad-CAM
    needs a square image (its upscale is one factor); a ResNet handle whose resolution in front of a stride-2 block is
    odd (36 x 60: 9 x 15) or whose sides are no multiple of 4 (30 x 40) is refused by lrp_create."""
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from test_gpu_gradient import CFG
    rs = np.random.RandomState(1)
    w = vgg_weights(rs, CFG, bias_std=0.05)
    w.update(adaptive_weights(rs, 15, 64, 8, 8, 8))
    eng = LRPEngine(decoder="adaptive", cnn_cfg=CFG, img_hw=(12, 20), L=15, D=64, H=8, E=8, V=8, max_images=1, max_tokens=2,
                    max_caption_len=4)
    eng.set_weights(w)
    eng.encode_images(rs.uniform(-120, 130, size=(1, 12, 20, 3)).astype(np.float32))
    eng.decoder_forward([[3, 5, 1]])
    with pytest.raises(ValueError, match="square image"):
        eng.guided_gradcam([0], [1])
    stacks = ((32, 2), (64, 2))
    kw = dict(decoder="gridtd", D=256, H=32, E=32, V=50, max_images=1, max_tokens=2, max_caption_len=6,
              resnet={"stem": 64, "stacks": stacks})
    with pytest.raises(NotImplementedError, match="odd resolution before a stride-2 block"):
        LRPEngine(img_hw=(36, 60), L=4 * 7, **kw)
    with pytest.raises(NotImplementedError, match="multiples of 4"):
        LRPEngine(img_hw=(30, 40), L=3 * 5, **kw)
