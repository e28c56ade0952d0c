"""Pin gpu_util.elem_ratio / elem_bar on the CPU, and with them the blind spot they close: at operator level a whole-tensor
relative L1 cannot see one wrong pixel.  Three defects are seeded into the float64 reference of one case of tests/conv_cases.py —
the split-bf16 forward conv on the 8-wave tile, (33, 56, 56, 8, 256): 103 488 pixels of 256 outputs — and each must exceed the
element bar that tests/test_gpu_conv_forms.py holds the kernels to; the two that touch one pixel stay under the 2e-5 the
whole-tensor assertions of tests/test_gpu_conv_op.py allow.  Nothing here needs a GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l1
from gpu_util import elem_bar, elem_ratio

NB, H, W, CIN, COUT = 33, 56, 56, 8, 256
TOL = 2e-5                                                   # the whole-tensor bar of the split-bf16 operator tests
PIX = (17, 30, 41)                                           # the pixel (image, y, x) the one-pixel defects sit on: interior


def _conv(x, w, b=None):
    """x (NB, H, W, Cin), w (3, 3, Cin, Cout) HWIO -> (NB, H, W, Cout), 3x3 'same', in the dtype of x"""
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, padding=1).permute(0, 2, 3, 1)


def _bf16(t):
    return t.float().bfloat16().double()


@pytest.fixture(scope="module")
def graph():
    rs = np.random.RandomState(NB + H + W + CIN + COUT)
    x = torch.as_tensor(rs.standard_normal((NB, H, W, CIN)).astype(np.float32))
    w = torch.as_tensor((rs.standard_normal((3, 3, CIN, COUT)) / np.sqrt(9 * CIN)).astype(np.float32))
    b = torch.as_tensor(rs.standard_normal(COUT).astype(np.float32))
    ref = _conv(x.double(), w.double(), b.double())
    mag = _conv(x.double().abs(), w.double().abs(), b.double().abs())
    r32 = elem_ratio(_conv(x, w, b), ref, mag)
    return x.double(), w.double(), ref, mag, r32


def test_identical_results_score_zero_and_massless_elements_must_be_zero():
    ref = np.array([[1.0, -2.0], [0.0, 4.0]])
    mag = np.array([[2.0, 2.0], [0.0, 8.0]])
    assert elem_ratio(ref, ref, mag) == 0.0
    out = ref.copy()
    out[1, 1] += 0.5
    assert elem_ratio(out, ref, mag) == 0.5 / 8.0
    out[1, 0] = 1e-30                                        # no mass went into it: anything but zero is wrong
    assert elem_ratio(out, ref, mag) == float("inf")
    t = [torch.as_tensor(a) for a in (out, ref, mag)]
    assert elem_ratio(*t) == float("inf")
    t[0][1, 0] = 0.0
    assert elem_ratio(*t) == 0.5 / 8.0
    with pytest.raises(ValueError):
        elem_ratio(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((3, 2)))


def test_the_bars_come_from_the_reference():
    assert elem_bar(0.0, False) == 2.0 ** -22 and elem_bar(1e-7, False) == 1e-6
    assert elem_bar(0.0, True) == 2.0 ** -16 + 2.0 ** -22 and elem_bar(2e-7, True) == 2.0 ** -16 + 2e-6


def test_float32_and_the_ideal_three_term_split_sit_under_the_bar(graph):
    x, w, ref, mag, r32 = graph
    assert 0.0 < r32 < 2.0 ** -22 * 4                       # a float32 sum of K = 72 products: a few ulp of its mass
    assert r32 < elem_bar(r32, False)
    xh, wh = _bf16(x), _bf16(w)
    xl, wl = _bf16(x - xh), _bf16(w - wh)
    split = _conv(xh, wh) + _conv(xh, wl) + _conv(xl, wh) + (ref - _conv(x, w))       # (the bias, exactly)
    r = elem_ratio(split, ref, mag)
    assert 0.0 < r < 2.0 ** -16 < elem_bar(r32, True), (r, r32)


def test_one_tap_dropped_on_one_pixel_passes_the_whole_tensor_bar_and_fails_the_element_bar(graph):
    x, w, ref, mag, r32 = graph
    n, y, c = PIX
    out = ref.clone()
    out[n, y, c] -= x[n, y - 1, c + 1] @ w[0, 2]            # the tap (ky, kx) = (0, 2) reads the pixel above and to the right
    assert rel_l1(out.numpy(), ref.numpy()) < TOL            # the blind spot, pinned
    assert elem_ratio(out, ref, mag) > 100 * elem_bar(r32, True)


def test_two_channels_swapped_on_one_pixel_pass_the_whole_tensor_bar_and_fail_the_element_bar(graph):
    x, w, ref, mag, r32 = graph
    n, y, c = PIX
    out = ref.clone()
    out[n, y, c, 5], out[n, y, c, 6] = ref[n, y, c, 6], ref[n, y, c, 5]
    assert rel_l1(out.numpy(), ref.numpy()) < TOL / 10
    assert elem_ratio(out, ref, mag) > 100 * elem_bar(r32, True)


def test_hi_only_weights_in_one_chunk_of_one_tile_fail_the_element_bar(graph):
    """the lo half of the weights lost for one 32-channel chunk (here: the layer's 8 channels) on the 128 rows of one M tile:
    2^-9 per product at worst.  The whole tensor sees 128 of 103 488 rows of it."""
    x, w, ref, mag, r32 = graph
    lost = _conv(x, w - _bf16(w)).reshape(-1, COUT)
    out = ref.clone().reshape(-1, COUT)
    rows = slice(128 * 400, 128 * 401)
    out[rows] -= lost[rows]
    out = out.reshape(ref.shape)
    assert rel_l1(out.numpy(), ref.numpy()) < TOL
    assert elem_ratio(out, ref, mag) > 10 * elem_bar(r32, True)


def test_the_split_bar_is_for_k_of_72_and_more():
    """2^-16 is the dropped lo*lo' term; with the rounding of the two lo halves the three-term product's worst case is 2^-15,
    and a sum of few products comes close to it somewhere among millions of outputs: at K = 8 the IDEAL split, in float64,
    is above the bar that the same arithmetic keeps with room to spare from K = 72 on (conv_cases.MIN_SPLIT_K)."""
    def ideal(K):
        rs = np.random.RandomState(K)
        x = torch.as_tensor(rs.standard_normal((NB * H * W, K))).float().double()
        w = torch.as_tensor(rs.standard_normal((K, COUT)) / np.sqrt(K)).float().double()
        ref, mag = x @ w, x.abs() @ w.abs()
        xh, wh = _bf16(x), _bf16(w)
        r32 = elem_ratio(x.float() @ w.float(), ref, mag)
        return elem_ratio(xh @ wh + xh @ _bf16(w - wh) + _bf16(x - xh) @ wh, ref, mag), elem_bar(r32, True)
    r, bar = ideal(8)
    assert bar < r < 2.0 ** -15, (r, bar)
    r, bar = ideal(72)
    assert r < bar / 2, (r, bar)
