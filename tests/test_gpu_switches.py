"""-m gpu: every A/B switch the library keeps (csrc/common.h `Switches`) against the default path.

VERDICT r3: "~40 LRP_* switches, six swept once, none under a committed test — each untested switch is a dead or wrong code
path waiting for a user."  Round 4 deleted 21 of them (their code paths with them where nothing else reaches those) and
kept 17 as measurement knobs / fall-backs (+ round 4's LRP_POOL_FUSED and LRP_SPARSE_POOL, opt-in then, the default now); three more went later
(LRP_CONV_TILE, LRP_DEC_BATCHED, LRP_DEC_MFMA_FWD: their alternatives were code nothing else reached), then the two that
selected the fp32 forms of the compact pool interface, which leaves 14.  This file runs each of the kept ones — alone, at the setting that leaves the default path — through the engine at a size where the kernels of the benchmark configuration engage and compares every
heat-map with the default run:

  * VGG16 at full size, 8 images x 9 words = 72 heat-maps per call: block1 takes the weights-in-registers kernel with the
    folded image layer and the compact pool interface, block2 the 128 x 128 halo tiles with the in-loop window loader,
    block3 / block4 the 8-wave 256 x 256 tiles (>= 400 workgroups) except their first convs (half as many output columns:
    128 x 128), block5 128 x 128 tiles, block4_conv3 / block3_conv3 the 2:4-sparse kernels; the tile-order table is built
    for 9 tokens per image;
  * the same network on ONE image x 3 words (a B = 1 handle): the small-grid 64 x 64 / 128 x 64 tiles.
Which dense form each of these launches takes is asserted, without a GPU, by tests/test_conv_plan.py.

Expectation per switch: `0.0` = bit-identical (the alternative computes every element through the same chain of operations:
DESIGN 4.1 says so for the tile shapes, the tile order, the compact pool interfaces and the epilogue pass loop), otherwise a
bound on the worst relative L1 over the heat-maps — 1e-6 where only the summation order inside one launch changes, 2e-5
(the batch-invariance bar) where the forward arithmetic changes and a ReLU / arg-max decision may flip.
The switches are read once per process; `engine.switches(...)` sets them and calls lrp_reload_switches (ABI v6)."""
import numpy as np
import pytest
import torch

from gpu_util import report
from lrp_imagecaptioning_amd.synthetic import captions, images

pytestmark = pytest.mark.gpu
B, T, V = 8, 9, 1000

# (switch, value, bound for the batch run, bound for the single-image run); 0.0 = bit-identical
CASES = [
    ("LRP_CONV_HALO", 0, 1e-6, 1e-6),
    ("LRP_CONV_BREG", 0, 1e-6, 1e-6),
    ("LRP_CONV_SMALL", 0, 0.0, 0.0),
    ("LRP_CONV_MID", 0, 0.0, 0.0),
    ("LRP_EPI_FAST", 0, 0.0, 0.0),
    ("LRP_UP2_PW", 0, 0.0, 0.0),
    ("LRP_TILE_ORDER", 0, 0.0, 0.0),
    ("LRP_UP2_COMPACT", 0, 0.0, 0.0),
    ("LRP_IMG_FOLD", 0, 1e-6, 1e-6),
    ("LRP_IMG_FUSED", 0, 1e-6, 1e-6),
    ("LRP_FWD_EMIT", 0, 2e-5, 2e-5),
    ("LRP_FWD_IL", 0, 2e-5, 2e-5),
    ("LRP_POOL_FUSED", 0, 0.0, 0.0),        # max-pool / gate / pooled pairs as a pass behind the conv: the same arithmetic, bit for bit
    ("LRP_SPARSE_POOL", 0, 1e-6, 1e-6),    # block4_conv3 / block3_conv3 on the dense kernels, not the 2:4-sparse matrix cores (other summation order)
]


# LRP_FWD_IL chooses between interleaved and stacked rows of the dual forward matrix when lrp_set_weight packs it (first run of
# this file: flipped after the upload it fed interleaved rows to the stacked-rows epilogue: heat-maps 1e+20 off)
PACKING_SWITCHES = {"LRP_FWD_IL"}


def _rel_l1(a, b):
    num = (a.double() - b.double()).abs().flatten(1).sum(1)
    den = b.double().abs().flatten(1).sum(1)
    return float((num / den).max())


@pytest.fixture(scope="module")
def setup():
    import bench
    from lrp_imagecaptioning_amd.engine import LRPEngine
    w = bench.synth_weights(0, V)
    rs = np.random.RandomState(31)
    X = torch.as_tensor(images(rs, B)).cuda()
    caps = captions(rs, B, T, V)
    big = LRPEngine(decoder="adaptive", V=V, max_images=B, max_tokens=B * T, max_caption_len=T + 1)
    one = LRPEngine(decoder="adaptive", V=V, max_images=1, max_tokens=3, max_caption_len=T + 1)
    for e in (big, one):
        e.set_weights(w)
    idx = [b for b in range(B) for _ in range(T)]
    tpos = [t for _ in range(B) for t in range(1, T + 1)]

    def run():
        big.encode_images(X)
        big.decoder_forward(caps)
        a = big.explain_tokens(idx, tpos)[0].clone()
        one.encode_images(X[3:4])
        one.decoder_forward(caps[3:4])
        b = one.explain_tokens([0, 0, 0], [1, 5, 9])[0].clone()
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
        return a, b

    def reload_weights():
        for e in (big, one):
            e.set_weights(w)
    ref = run()
    again = run()
    assert torch.equal(ref[0], again[0]) and torch.equal(ref[1], again[1])      # the default path is deterministic
    return run, ref, reload_weights


@pytest.mark.parametrize("name,value,tol_batch,tol_one", CASES, ids=["%s=%s" % (c[0], c[1]) for c in CASES])
def test_switch_against_the_default_path(setup, name, value, tol_batch, tol_one):
    from lrp_imagecaptioning_amd import _capi
    from lrp_imagecaptioning_amd.engine import switches
    run, ref, reload_weights = setup
    lib = _capi.load()
    packs = name in PACKING_SWITCHES                       # decides the LAYOUT of an operand copy: set before the weights are uploaded
    with switches(**{name: value}):
        if packs:
            reload_weights()
        n0 = int(lib.lrp_launch_count())
        got = run()
        launches = int(lib.lrp_launch_count()) - n0
    if packs:
        reload_weights()
    e = [_rel_l1(got[k], ref[k]) for k in range(2)]
    same = [bool(torch.equal(got[k], ref[k])) for k in range(2)]
    report("switch_%s_%s" % (name, value), batch_rel_l1=e[0], single_image_rel_l1=e[1], batch_bit_identical=same[0],
           single_image_bit_identical=same[1], launches=launches)
    for k, tol in enumerate((tol_batch, tol_one)):
        if tol == 0.0:
            assert same[k], (name, value, "batch" if k == 0 else "single image", e[k])
        else:
            assert e[k] < tol, (name, value, "batch" if k == 0 else "single image", e[k])
    # and the default path is back afterwards
    back = run()
    assert torch.equal(back[0], ref[0]) and torch.equal(back[1], ref[1])


def test_fused_pool_with_a_ragged_image_stack():
    """The pool in the conv epilogue (ConvArgs::pool_gc) on FIVE images: the stack of block4's 28-row maps is 140 rows = 17.5
    tiles of 8 rows — tiles that straddle two images and a last one that runs past the stack — and 5 x 10 heat-maps later every
    bit equals the pass-behind-the-conv form, and the walk through the EXPANDED pool interfaces (LRP_UP2_COMPACT=0, LRP_UP2_PW=0:
    every pooled layer's full-resolution gate, rebuilt on demand from the compact one by Encoder::full_gate) does too."""
    import bench
    from lrp_imagecaptioning_amd.engine import LRPEngine, switches
    Bq, Tq = 5, 4
    w = bench.synth_weights(0, V)
    rs = np.random.RandomState(77)
    X = torch.as_tensor(images(rs, Bq)).cuda()
    caps = captions(rs, Bq, Tq, V)
    eng = LRPEngine(decoder="adaptive", V=V, max_images=Bq, max_tokens=Bq * Tq, max_caption_len=Tq + 1)
    eng.set_weights(w)
    idx = [b for b in range(Bq) for _ in range(Tq)]
    tpos = [t for _ in range(Bq) for t in range(1, Tq + 1)]

    def run():
        eng.encode_images(X)
        eng.decoder_forward(caps)
        hm = eng.explain_tokens(idx, tpos)[0].clone()
        feat = eng.get_features()
        R = (feat[[0, 4]] * 0.5).contiguous()
        given = eng.cnn_explain([0, 4], R).clone()         # (the CNN half alone, on a given relevance)
        return hm, given
    a = run()
    with switches(LRP_POOL_FUSED=0):
        b = run()
    with switches(LRP_UP2_COMPACT=0, LRP_UP2_PW=0):        # expanded interfaces: every pooled layer's full-resolution gate is read
        c = run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
