"""-m gpu: the implicit-GEMM conv kernel (lrp_op_conv through the C ABI) against float64 torch-CPU convolutions under a
whole-tensor relative L1: ragged M tails, Cin not a multiple of 32, 1x1 mode and both LRP epilogues (gate multiply, gate multiply
through a 2x2 pool).  These stacks of a few small images are small grids: under default switches the launch plan puts most of them
on the 64 x 64 tiles (the form each case takes is noted beside it and written into its report line).  Every form of the kernel,
one launch at a time and per output element, is tests/test_gpu_conv_forms.py over the table of tests/conv_cases.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases
from conftest import rel_l1
from gpu_util import report

pytestmark = pytest.mark.gpu


def _planned(case, taps, mode, split):
    """the form lrp_op_conv takes for this launch under the switches in force, e.g. 'SMALL 64x64' (conv_cases.op_plan)"""
    return conv_cases.plan_name(conv_cases.op_plan(conv_cases.Case(*case[:5], taps, mode, split, {}, "", (), "")))


def _ref_conv(x, w, b, taps, relu):
    xt = torch.as_tensor(x, dtype=torch.float64).permute(0, 3, 1, 2)
    wt = torch.as_tensor(w, dtype=torch.float64).permute(3, 2, 0, 1)
    y = F.conv2d(xt, wt, torch.as_tensor(b, dtype=torch.float64), padding=1 if taps == 9 else 0)
    if relu:
        y = F.relu(y)
    return y.permute(0, 2, 3, 1).numpy()


def _ref_convT(s, w, taps):
    st = torch.as_tensor(s, dtype=torch.float64).permute(0, 3, 1, 2)
    wt = torch.as_tensor(w, dtype=torch.float64).permute(3, 2, 0, 1)      # (Cout,Cin,kh,kw)
    y = F.conv_transpose2d(st, wt, padding=1 if taps == 9 else 0)
    return y.permute(0, 2, 3, 1).numpy()


FWD_CASES = [  # NB, H, W, Cin, Cout, taps
    (2, 8, 8, 32, 128, 9),      # SMALL 64x64: two M tiles, two N tiles, exact
    (1, 14, 14, 64, 256, 9),    # SMALL 64x64: four N tiles, ragged M (196)
    (3, 7, 5, 8, 64, 9),        # SMALL 64x64: Cin < 32, odd sizes
    (2, 6, 6, 16, 16, 9),       # PLAIN 128x32, tiny
    (1, 9, 9, 36, 40, 9),       # SMALL 64x64: Cin, Cout not multiples of 32
    (1, 1, 300, 64, 96, 1),     # SMALL 64x64: 1x1 mode (dense layer), ragged M
    (2, 16, 16, 128, 192, 9),   # SMALL 64x64: N = 192, three N tiles
]


@pytest.mark.parametrize("case", FWD_CASES)
@pytest.mark.parametrize("mode", [0, 1])
def test_conv_forward(case, mode):
    from lrp_imagecaptioning_amd.engine import op_conv
    NB, H, W, Cin, Cout, taps = case
    rs = np.random.RandomState(hash(case) % 1000)
    k = 3 if taps == 9 else 1
    x = rs.standard_normal((NB, H, W, Cin)).astype(np.float32)
    w = (rs.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(np.float32)
    b = rs.standard_normal(Cout).astype(np.float32)
    out = op_conv(torch.as_tensor(x).cuda(), w, b, None, mode, taps).cpu().numpy()
    ref = _ref_conv(x, w, b, taps, relu=(mode == 0))
    err = rel_l1(out, ref)
    report("conv_fwd", case=list(case), mode=mode, plan=_planned(case, taps, mode, False), rel_l1=err)
    assert out.shape == ref.shape
    assert err < 2e-6, err


BWD_CASES = [  # NB, H, W, Cin(out channels of the LRP step), Cout(channels of S)
    (2, 8, 8, 128, 64),
    (1, 14, 14, 256, 128),
    (3, 6, 6, 64, 32),
    (2, 6, 6, 16, 24),
    (5, 4, 4, 8, 8),
]


@pytest.mark.parametrize("case", BWD_CASES)
@pytest.mark.parametrize("mode", [2, 3])
def test_conv_lrp_backward(case, mode):
    """out = convT(S, w) * gate   (mode 3: through a 2x2 max-pool, gate at 2x resolution)."""
    from lrp_imagecaptioning_amd.engine import op_conv
    NB, H, W, Cin, Cout = case
    rs = np.random.RandomState(sum(case))
    s = rs.standard_normal((NB, H, W, Cout)).astype(np.float32)
    w = np.abs(rs.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32)
    up = 2 if mode == 3 else 1
    gate = rs.uniform(0, 1, size=(NB, up * H, up * W, Cin)).astype(np.float32)
    out = op_conv(torch.as_tensor(s).cuda(), w, None, torch.as_tensor(gate).cuda(), mode, 9).cpu().numpy()
    c = _ref_convT(s, w, 9)
    if mode == 3:
        c = c.repeat(2, axis=1).repeat(2, axis=2)
    ref = c * gate
    err = rel_l1(out, ref)
    report("conv_bwd", case=list(case), mode=mode, plan=_planned(case, 9, mode, False), rel_l1=err)
    assert out.shape == ref.shape
    assert err < 2e-6, err


def test_identity_weight_asymmetric():
    """A = I check with an asymmetric operand (catches a transposed C/D map)."""
    from lrp_imagecaptioning_amd.engine import op_conv
    C = 64
    x = np.arange(2 * 4 * 4 * C, dtype=np.float32).reshape(2, 4, 4, C) / 100.0
    w = np.zeros((3, 3, C, C), dtype=np.float32)
    w[1, 1] = np.eye(C)
    w[1, 1, 3, 5] = 2.0                     # asymmetric: out[..,5] += 2*x[..,3]
    out = op_conv(torch.as_tensor(x).cuda(), w, np.zeros(C, np.float32), None, 1, 9).cpu().numpy()
    ref = x.copy()
    ref[..., 5] += 2.0 * x[..., 3]
    np.testing.assert_allclose(out, ref, rtol=1e-6, atol=1e-6)


# ---- split-bf16 path (LRP_CONV_HALO: 0 never, 1 auto, 2 always the resident-image kernels).  Forward, all but two of these
# small grids take SMALL 64x64 at every setting; backward they take BREG 128x64 (N = 40 ... 64 output columns; SMALL under
# LRP_CONV_HALO=0), SMALL (N = 72) or PLAIN 128x32 (N <= 32).  The resident-image geometries that the shapes were once chosen for — tiles that span images, W = 33,
# widths below 14, the power-of-two pitch — are the cases of tests/conv_cases.py with the small-grid rules switched off.
SPLIT_CASES = [  # NB, H, W, Cin, Cout   (forward: Cin -> Cout; backward: S has Cout channels, out has Cin)
    (3, 14, 14, 64, 128),     # fwd SMALL; bwd BREG 128x64 tw 14 th 9: tiles span image boundaries in the stack
    (2, 28, 28, 40, 64),      # fwd SMALL; bwd BREG: N = 40 < 64, two column tiles
    (1, 56, 56, 8, 128),      # fwd SMALL; bwd PLAIN 128x32 (N = 8)
    (2, 7, 5, 72, 64),        # fwd SMALL; bwd SMALL (N = 72)
    (1, 9, 33, 16, 128),      # fwd SMALL; bwd PLAIN 128x32 (N = 16)
    (2, 16, 16, 64, 64),      # fwd SMALL; bwd BREG tw 8 under LRP_CONV_HALO=2, SMALL otherwise
    (33, 56, 56, 8, 256),     # fwd HALO 256x256, the 8-wave tile (>= 400 blocks), tw 14 th 18; bwd PLAIN 128x32
    (140, 14, 14, 16, 256),   # fwd HALO 128x128 tw 14 th 9 (218 x 2 tiles: below the 8-wave tile's 400 blocks); bwd PLAIN 128x32
    (3, 28, 28, 64, 64),      # backward: N = 64, two channel chunks -> weights-in-registers kernel (one group)
    (2, 14, 28, 64, 128),     # backward: N = 64, four chunks = two groups of the resident image
    (2, 14, 14, 56, 96),      # backward: N = 56 (< 64), three chunks: the last group holds one chunk
]


@pytest.fixture(params=["0", "1", "2"])
def halo_mode(request):
    from lrp_imagecaptioning_amd.engine import switches
    with switches(LRP_CONV_HALO=request.param):
        yield request.param


@pytest.mark.parametrize("case", SPLIT_CASES)
def test_split_bf16_forward(case, halo_mode):
    from lrp_imagecaptioning_amd.engine import op_conv
    NB, H, W, Cin, Cout = case
    rs = np.random.RandomState(sum(case))
    x = rs.standard_normal((NB, H, W, Cin)).astype(np.float32)
    w = (rs.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32)
    b = rs.standard_normal(Cout).astype(np.float32)
    out = op_conv(torch.as_tensor(x).cuda(), w, b, None, 1, 9, split_bf16=True).cpu().numpy()
    err = rel_l1(out, _ref_conv(x, w, b, 9, relu=False))
    report("conv_split_fwd", case=list(case), halo=halo_mode, plan=_planned(case, 9, 1, True), rel_l1=err)
    assert err < 2e-5, err


@pytest.mark.parametrize("case", SPLIT_CASES)
@pytest.mark.parametrize("mode", [2, 3])
def test_split_bf16_lrp_backward(case, mode, halo_mode):
    from lrp_imagecaptioning_amd.engine import op_conv
    NB, H, W, Cin, Cout = case
    if mode == 3 and NB * H * W > 50000:
        NB = max(1, NB // 4)          # the 2x-resolution gate of the pool mode is 4x the pixels
    rs = np.random.RandomState(sum(case) + mode)
    s = rs.standard_normal((NB, H, W, Cout)).astype(np.float32)
    w = np.abs(rs.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32)
    up = 2 if mode == 3 else 1
    gate = rs.uniform(0, 1, size=(NB, up * H, up * W, Cin)).astype(np.float32)
    out = op_conv(torch.as_tensor(s).cuda(), w, None, torch.as_tensor(gate).cuda(), mode, 9, split_bf16=True).cpu().numpy()
    c = _ref_convT(s, w, 9)
    if mode == 3:
        c = c.repeat(2, axis=1).repeat(2, axis=2)
    err = rel_l1(out, c * gate)
    report("conv_split_bwd", case=list(case), mode=mode, halo=halo_mode, plan=_planned((NB,) + tuple(case[1:]), 9, mode, True), rel_l1=err)
    assert err < 2e-5, err


# ---- small grids take 64 x 64 tiles with a 4-stage k pipeline (LRP_CONV_SMALL, conv_igemm.h): every output element sees the
# same chain of MFMAs in the same k order as with the large tiles, so the two must agree BIT FOR BIT — that is what keeps a
# single image's heat-maps identical to the same image explained inside a batch of 32
SMALL_CASES = [  # NB, H, W, Cin, Cout
    (1, 14, 14, 512, 512),    # block5 of one image: 2 x 4 large tiles, K = 4608
    (10, 14, 14, 256, 128),   # ten words: 16 x 1 large tiles
    (1, 28, 28, 72, 64),      # N = 64 tile family, Cin not a multiple of 32
    (2, 7, 5, 40, 192),       # ragged M, N = 192
    (10, 28, 28, 256, 256),   # split: 62 x 2 large tiles = 124 <= 128, still the 64 x 64 tiles; fp32: PLAIN 128x64 (62 x 4, the halved
                              # fp32 tile) under either setting.  The 128 x 64 tiles of the grids in between: tests/conv_cases.py
]


@pytest.mark.parametrize("case", SMALL_CASES)
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_small_tiles_are_bit_identical_to_large_tiles(case, split, mode):
    from lrp_imagecaptioning_amd.engine import op_conv
    NB, H, W, Cin, Cout = case
    rs = np.random.RandomState(sum(case) + mode)
    if mode == 1:
        x = rs.standard_normal((NB, H, W, Cin)).astype(np.float32)
        w = (rs.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32)
        args = (torch.as_tensor(x).cuda(), w, rs.standard_normal(Cout).astype(np.float32), None, 1, 9)
    else:
        s = rs.standard_normal((NB, H, W, Cout)).astype(np.float32)
        w = np.abs(rs.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32)
        up = 2 if mode == 3 else 1
        gate = rs.uniform(0, 1, size=(NB, up * H, up * W, Cin)).astype(np.float32)
        args = (torch.as_tensor(s).cuda(), w, None, torch.as_tensor(gate).cuda(), mode, 9)
    outs = {}
    from lrp_imagecaptioning_amd.engine import switches
    for small in ("1", "0"):
        with switches(LRP_CONV_SMALL=small, LRP_CONV_MID=small):   # the 128 x 64 tiles of the grids in between follow the same switch here
            outs[small] = op_conv(*args, split_bf16=split).clone()
    assert torch.equal(outs["1"], outs["0"]), float((outs["1"] - outs["0"]).abs().max())
