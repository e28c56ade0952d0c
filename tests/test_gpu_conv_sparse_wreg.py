"""-m gpu: the weights-in-registers loop of the 2:4-sparse pooled consumer's large form (csrc/conv_sparse.h, conv_sparse_kernel
<SparseTileLarge, WREG>) against the LDS-stage loop it replaces (LRP_CONV_SPARSE_WREG=0).  Both issue, per output element, the
same chain of smfmacs — chunk-major, six k-steps per 16 channels, lo x hi, hi x lo, hi x hi on one accumulator, then gate
multiply and split — so every comparison here is torch.equal.

Operator level (lrp_op_conv_pool_sparse): the launcher's own choice, the forced large form (the one the switch changes) and the
forced small form (which it does not), operands as in tests/test_gpu_conv_sparse.py.

Engine level: VGG16 at full size, 2 images x 3 words: heat-maps and one cnn_explain with the switch 0 and 1, and the default
against LRP_CONV_SPARSE_WREG=1.  Six tokens are a small grid, which the launcher gives to the small form; the same comparison
under LRP_CONV_SMALL=0 puts both sparse launches of the walk on the large form."""
import numpy as np
import pytest
import torch

from gpu_util import report
from lrp_imagecaptioning_amd.synthetic import captions, images

pytestmark = pytest.mark.gpu
V = 1000
FORMS = {"auto": 1, "large": 1 | (2 << 8), "small": 1 | (4 << 8)}     # lrp_op_conv_pool_sparse's reps: one launch, the form forced

CASES = [  # NB, Hp, Wp, Cin (output columns N), Cout (K side)
    (5, 7, 5, 256, 16),       # one chunk: the weight prefetch runs past the last step inside the first chunk; Wp < 14, Hp odd
    (3, 14, 14, 256, 32),     # two chunks, tiles span tokens
    (2, 28, 28, 256, 48),     # three chunks, two column tiles
    (1, 3, 17, 512, 64),      # two N tiles, ragged second column tile
    (2, 14, 14, 256, 272),    # seventeen chunks: an odd count over many hand-overs, both A buffers end in either parity
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_operator_is_bit_identical_to_the_lds_stage_loop(case):
    from lrp_imagecaptioning_amd.engine import op_conv_pool_sparse, switches
    NB, Hp, Wp, Cin, Cout = case
    rs = np.random.RandomState(sum(case))
    sc = torch.as_tensor(rs.standard_normal((NB, Hp, Wp, Cout)).astype(np.float32)).cuda()
    pos = torch.as_tensor(rs.randint(0, 4, size=(NB, Hp, Wp, Cout)).astype(np.uint8)).cuda()
    w = np.abs(rs.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cout)).astype(np.float32)     # w+ >= 0 like the walk's
    w[rs.uniform(size=w.shape) < 0.3] = 0.0
    gate = torch.as_tensor(rs.uniform(0, 1, size=(NB, 2 * Hp, 2 * Wp, Cin)).astype(np.float32)).cuda()
    outs = {}
    for on in (0, 1):
        with switches(LRP_CONV_SPARSE_WREG=on):
            for form, reps in FORMS.items():
                outs[on, form] = op_conv_pool_sparse(sc, pos, w, gate, reps=reps).clone()
    for form in FORMS:
        a, b = outs[1, form], outs[0, form]
        assert bool(torch.isfinite(a).all()) and float(a.abs().sum()) > 0, form
        assert torch.equal(a, b), (form, float((a - b).abs().max()))
    assert torch.equal(outs[1, "large"], outs[1, "small"])
    report("conv_sparse_wreg_%s" % "x".join(map(str, case)), bit_identical=True)


@pytest.fixture(scope="module")
def engine():
    import bench
    from lrp_imagecaptioning_amd.engine import LRPEngine
    B, T = 2, 3
    rs = np.random.RandomState(5)
    X = torch.as_tensor(images(rs, B)).cuda()
    caps = captions(rs, B, T, V)
    eng = LRPEngine(decoder="adaptive", V=V, max_images=B, max_tokens=B * T, max_caption_len=T + 1)
    eng.set_weights(bench.synth_weights(0, V))
    idx = [b for b in range(B) for _ in range(T)]
    tpos = [t for _ in range(B) for t in range(1, T + 1)]

    def run():
        eng.encode_images(X)
        eng.decoder_forward(caps)
        hm = eng.explain_tokens(idx, tpos)[0].clone()
        R = (eng.get_features()[[0, 1]] * 0.5).contiguous()
        return hm, eng.cnn_explain([0, 1], R).clone()
    return run


@pytest.mark.parametrize("small", [1, 0], ids=["launcher's choice", "large form"])
def test_engine_is_bit_identical_with_the_switch_off_and_on(engine, small):
    from lrp_imagecaptioning_amd.engine import switches
    with switches(LRP_CONV_SMALL=small):
        ref = engine()
        with switches(LRP_CONV_SMALL=small, LRP_CONV_SPARSE_WREG=1):
            on = engine()
        with switches(LRP_CONV_SMALL=small, LRP_CONV_SPARSE_WREG=0):
            off = engine()
        back = engine()
    for r in ref:
        assert bool(torch.isfinite(r).all()) and float(r.abs().sum()) > 0
    for what, r, a, b, c in zip(("heat-maps", "cnn_explain"), ref, on, off, back):
        assert torch.equal(a, b), (what, float((a - b).abs().max()))
        assert torch.equal(r, a), what                    # the default is LRP_CONV_SPARSE_WREG=1 ...
        assert torch.equal(c, r), what                    # ... and still is after the with block
    report("conv_sparse_wreg_engine_small%d" % small, bit_identical=True)
