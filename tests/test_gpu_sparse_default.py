"""-m gpu: the 2:4-sparse consumers of the pooled boundaries (csrc/conv_sparse.h) as the DEFAULT path of the walk.

Sparse and dense kernels sum in different orders, so the choice between them may depend on the layer only, never on how many
tokens or images a call explains; and the sparse kernel has two tile forms — 256 windows x 256 columns on 8 waves for the grids
of the batch engine, 64 windows x 128 columns on 4 waves for small grids — which must agree to the bit, because a picture's
heat-map must not depend on the batch it is explained in (tests/test_gpu_real_images.py asserts that on photographs).  Here:

  1. operator level: the small form against the large form on one stack (both forced, every row), and the launcher's own
     choice on a few tokens of that stack against the large form's rows — every parity class, tiles that span tokens, ragged
     last tiles, Wp < 14, two column tiles, N = 256 and N = 512;
  2. end to end: VGG16 at full size, 8 images x 9 words against each image on a B = 1 handle, default settings: torch.equal;
  3. the default IS the sparse path: equal to LRP_SPARSE_POOL=1, different from LRP_SPARSE_POOL=0 and within 1e-6 relative L1
     of it (the bound tests/test_gpu_switches.py uses for a changed summation order), batch engine and single-image engine;
  4. the expanded interface of all four pooled boundaries stays under test: with LRP_SPARSE_POOL=0, LRP_UP2_COMPACT=0 and
     LRP_UP2_PW=0 are bit-identical to LRP_SPARSE_POOL=0 alone on five images (a ragged image stack)."""
import numpy as np
import pytest
import torch

from gpu_util import report
from lrp_imagecaptioning_amd.synthetic import captions, images

pytestmark = pytest.mark.gpu
V = 1000
FORCE_LARGE, FORCE_SMALL = 1 | (2 << 8), 1 | (4 << 8)      # lrp_op_conv_pool_sparse's reps: one launch, the form whatever the grid

# NB, Hp, Wp, Cin (output columns N), Cout (K side), tokens of the sub-stack.  The launcher takes the small form up to
# SMALL_BLOCKS workgroups of the large one, 4 classes x ceil(NB Hp / 18) x ceil(Wp / 14) x N / 256: every full stack below is
# beyond that (its own choice is the large form), every sub-stack below it.  SMALL_BLOCKS repeats CONV_SPARSE_SMALL_BLOCKS of
# csrc/conv_sparse.h and moves with it; the forced forms compare the two kernels whatever the constant is.
SMALL_BLOCKS = 96
CASES = [
    (90, 14, 14, 256, 32, 3),      # block4_conv3's geometry: 4-row small tiles span the 14-row tokens, ragged last tile
    (24, 28, 28, 256, 48, 2),      # block3_conv3's geometry: two column tiles, three chunks
    (170, 7, 5, 256, 16, 5),       # Wp < 14, Hp odd
    (100, 3, 17, 512, 64, 3),      # N = 512 (four 128-column small tiles per class), ragged second column tile
]


def _large_blocks(NB, Hp, Wp, N):
    return 4 * ((NB * Hp + 17) // 18) * ((Wp + 13) // 14) * (N // 256)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_small_form_equals_large_form(case):
    from lrp_imagecaptioning_amd.engine import op_conv_pool_sparse
    NB, Hp, Wp, Cin, Cout, k = case
    assert _large_blocks(NB, Hp, Wp, Cin) > SMALL_BLOCKS >= _large_blocks(k, Hp, Wp, Cin)
    rs = np.random.RandomState(sum(case))
    sc = torch.as_tensor(rs.standard_normal((NB, Hp, Wp, Cout)).astype(np.float32)).cuda()
    pos = torch.as_tensor(rs.randint(0, 4, size=(NB, Hp, Wp, Cout)).astype(np.uint8)).cuda()
    w = np.abs(rs.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cout)).astype(np.float32)
    w[rs.uniform(size=w.shape) < 0.3] = 0.0
    gate = torch.as_tensor(rs.uniform(0, 1, size=(NB, 2 * Hp, 2 * Wp, Cin)).astype(np.float32)).cuda()
    large = op_conv_pool_sparse(sc, pos, w, gate, reps=FORCE_LARGE)
    auto = op_conv_pool_sparse(sc, pos, w, gate)
    small = op_conv_pool_sparse(sc, pos, w, gate, reps=FORCE_SMALL)
    assert bool(torch.isfinite(large).all()) and float(large.abs().sum()) > 0
    assert torch.equal(auto, large)
    assert torch.equal(small, large)
    # the launcher's own choice on a few tokens: from the start of the stack and from its middle (other tile alignment)
    for s0 in (0, NB // 2):
        sub = op_conv_pool_sparse(sc[s0:s0 + k], pos[s0:s0 + k], w, gate[s0:s0 + k])
        assert torch.equal(sub, large[s0:s0 + k]), s0
        sub_l = op_conv_pool_sparse(sc[s0:s0 + k], pos[s0:s0 + k], w, gate[s0:s0 + k], reps=FORCE_LARGE)
        assert torch.equal(sub_l, large[s0:s0 + k]), s0
    report("sparse_small_vs_large_%s" % "x".join(map(str, case)), bit_identical=True)


def _rel_l1(a, b):
    num = (a.double() - b.double()).abs().flatten(1).sum(1)
    den = b.double().abs().flatten(1).sum(1)
    return float((num / den).max())


@pytest.fixture(scope="module")
def engines():
    import bench
    from lrp_imagecaptioning_amd.engine import LRPEngine
    B, T = 8, 9
    w = bench.synth_weights(0, V)
    rs = np.random.RandomState(31)
    X = torch.as_tensor(images(rs, B)).cuda()
    caps = captions(rs, B, T, V)
    big = LRPEngine(decoder="adaptive", V=V, max_images=B, max_tokens=B * T, max_caption_len=T + 1)
    one = LRPEngine(decoder="adaptive", V=V, max_images=1, max_tokens=T, max_caption_len=T + 1)
    for e in (big, one):
        e.set_weights(w)
    idx = [b for b in range(B) for _ in range(T)]
    tpos = [t for _ in range(B) for t in range(1, T + 1)]

    def run_big():
        big.encode_images(X)
        big.decoder_forward(caps)
        return big.explain_tokens(idx, tpos)[0].clone()

    def run_one(i):
        one.encode_images(X[i:i + 1])
        one.decoder_forward(caps[i:i + 1])
        return one.explain_tokens([0] * T, list(range(1, T + 1)))[0].clone()
    return B, T, run_big, run_one


def test_batch_equals_single_image_bit_for_bit(engines):
    B, T, run_big, run_one = engines
    batch = run_big()
    assert bool(torch.isfinite(batch).all())
    for i in range(B):
        alone = run_one(i)
        assert torch.equal(batch[i * T:(i + 1) * T], alone), i
    report("sparse_default_b8_vs_b1", bit_identical=True, images=B, words=T)


def test_the_default_takes_the_sparse_path(engines):
    from lrp_imagecaptioning_amd.engine import switches
    B, T, run_big, run_one = engines
    runs = {"batch": run_big, "single": lambda: run_one(3)}
    for name, run in runs.items():
        ref = run()
        with switches(LRP_SPARSE_POOL=1):
            on = run()
        with switches(LRP_SPARSE_POOL=0):
            off = run()
        e = _rel_l1(ref, off)
        print("sparse default vs LRP_SPARSE_POOL=0, %s engine: worst relative L1 %.3g" % (name, e))
        report("sparse_default_vs_dense_" + name, rel_l1=e)
        assert torch.equal(ref, on), name
        assert not torch.equal(ref, off), name
        assert e < 1e-6, (name, e)
        assert torch.equal(run(), ref), name              # and the default is back afterwards


def test_expanded_interfaces_with_dense_consumers_on_a_ragged_stack():
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
        return hm, eng.cnn_explain([0, 4], R).clone()
    with switches(LRP_SPARSE_POOL=0):
        a = run()
    with switches(LRP_SPARSE_POOL=0, LRP_UP2_COMPACT=0, LRP_UP2_PW=0):
        b = run()
    assert bool(torch.isfinite(a[0]).all())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
