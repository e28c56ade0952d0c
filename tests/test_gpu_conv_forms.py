"""-m gpu: every kernel form that lrp_op_conv can take (tests/conv_cases.py; tests/test_conv_op_coverage.py proves the table
complete on the CPU) and the conv's neighbours — lrp_op_conv_pool_sparse, lrp_op_conv_wgrad[_bf16], lrp_op_sgemm — against a float64
torch evaluation of the same operation, in two ways:

(a) EXACT operands: the result is representable whatever the summation order, so the comparison is torch.equal with the float64
    result cast to float32.  Recipe A: in = m / 1024 with integer |m| <= 512, integer weights ({0..3} backward, {-3..3} forward),
    integer bias in [-8, 8], gates in {0, 0.5, 1, 2}; recipe B: the 1/1024 grid on the weights and the integers on the input.
    m / 1024 has at most 10 significant bits: bf16 hi + lo hold it exactly, the integer side has no lo half (so the dropped lo*lo'
    term is zero), every product of 8-bit parts is exact in fp32, every partial sum is a multiple of 2^-10 below 2^14, and a gate
    that is a power of two multiplies exactly.  The condition is asserted from the reference: max mag x 1024 < 2^24.  A misrouted
    tap, channel, separator row or tile edge, or a dropped hi*lo' / lo*hi' term, is a hard mismatch in A or B; a zero gate must
    give an exact zero.
(b) RANDOM operands (those of tests/test_gpu_conv_op.py), a bound per output element: gpu_util.elem_ratio against
    mag = |gate| x (|in| conv |w|) (+ |bias|), under gpu_util.elem_bar of r32 = the same ratio of torch's float32 evaluation of
    the graph on the CPU.  r32 is taken on the first images of a large stack only: the maximum over a part is at most the
    maximum over the whole, so the bar is never wider for it.

Each case leaves its form, ratio, r32 and bar through gpu_util.report (profiles/conv_forms_parity.txt is that record)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases as T
from gpu_util import elem_bar, elem_ratio, report

pytestmark = pytest.mark.gpu

OPERANDS = ("exact_a", "exact_b", "random")
GATES = (0.0, 0.5, 1.0, 2.0)


def _grid(rs, shape, lo=-512):
    return (rs.randint(lo, 513, size=shape) / 1024.0).astype(np.float32)


def _gate(shape, seed, exact):
    """on the device (the pooled 8-wave case has 105 M gate elements).  random: uniform [0, 1) with one in eight exactly zero"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if exact:
        return torch.tensor(GATES, device="cuda")[torch.randint(0, 4, shape, device="cuda", generator=g)]
    u = torch.rand(shape, device="cuda", generator=g)
    return u * (torch.rand(shape, device="cuda", generator=g) >= 0.125)


def _operands(c, kind):
    """-> x (NB, H, W, channels of the input) device, w HWIO numpy, bias numpy | None, gate device | None"""
    inC, _ = T.launch_dims(c)
    k = 3 if c.taps == 9 else 1
    bwd = c.mode >= 2
    seed = sum(c[:8]) + 7 * OPERANDS.index(kind)
    rs = np.random.RandomState(seed)
    xs, ws = (c.NB, c.H, c.W, inC), (k, k, c.Cin, c.Cout)
    if kind == "exact_a":
        x, w = _grid(rs, xs), rs.randint(0 if bwd else -3, 4, size=ws).astype(np.float32)
    elif kind == "exact_b":
        x, w = rs.randint(-3, 4, size=xs).astype(np.float32), _grid(rs, ws, 0 if bwd else -512)
    else:
        x = rs.standard_normal(xs).astype(np.float32)
        w = (rs.standard_normal(ws) / np.sqrt(k * k * c.Cin)).astype(np.float32)
        w = np.abs(w) if bwd else w
    if bwd:
        up = 2 if c.mode == 3 else 1
        return torch.as_tensor(x).cuda(), w, None, _gate((c.NB, up * c.H, up * c.W, c.Cin), seed, kind != "random")
    b = rs.randint(-8, 9, size=c.Cout).astype(np.float32) if kind != "random" else rs.standard_normal(c.Cout).astype(np.float32)
    return torch.as_tensor(x).cuda(), w, b, None


def _graph(c, x, w, b, gate, relu=True):
    """the operation of lrp_op_conv in the dtype and on the device of its (torch) operands; w HWIO"""
    pad = 1 if c.taps == 9 else 0
    xt, wt = x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1)
    if c.mode < 2:
        y = F.conv2d(xt, wt, b, padding=pad)
        return (F.relu(y) if c.mode == 0 and relu else y).permute(0, 2, 3, 1)
    y = F.conv_transpose2d(xt, wt, padding=pad).permute(0, 2, 3, 1)        # wt: (channels of S, output columns, k, k)
    if c.mode == 3:
        y = y.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return y * gate


def _eval(c, x, w, b, gate, dtype, dev, n=None, mass=True):
    """(result, mass) of the first n images (None: all) in `dtype` on `dev`; mass = the graph of the absolute values, no relu"""
    xs, gs = x[:n].to(dev, dtype), None if gate is None else gate[:n].to(dev, dtype)
    wt, bt = torch.as_tensor(w).to(dev, dtype), None if b is None else torch.as_tensor(b).to(dev, dtype)
    res = _graph(c, xs, wt, bt, gs)
    if not mass:
        return res, None
    return res, _graph(c, xs.abs(), wt.abs(), None if bt is None else bt.abs(), None if gs is None else gs.abs(), relu=False)


def _r32_images(c):
    """how many images the float32 CPU restatement evaluates: about 4 G multiply-adds and 16 M outputs at the most"""
    inC, N = T.launch_dims(c)
    macs = c.H * c.W * c.taps * inC * N
    outs = c.H * c.W * N * (4 if c.mode == 3 else 1)
    return max(1, min(c.NB, int(4e9 // macs), (1 << 24) // outs))


def _mismatch(out, want):
    bad = (out != want).nonzero()
    return "%d of %d elements differ, first at %s: %r != %r" % (len(bad), out.numel(), bad[0].tolist(),
                                                                 float(out[tuple(bad[0])]), float(want[tuple(bad[0])]))


@pytest.mark.parametrize("kind", OPERANDS)
@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_conv_form_against_float64(case, kind):
    from lrp_imagecaptioning_amd.engine import op_conv, switches
    c = case
    x, w, b, gate = _operands(c, kind)
    with switches(**c.switches):
        p = T.op_plan(c)
        assert p["ok"] == 1 and (T.FORM_NAMES[p["form"]], (p["BM"], p["BN"])) == (c.form, tuple(c.tile)), (T.plan_name(p), c)
        out = op_conv(x, w, b, gate, c.mode, c.taps, split_bf16=c.split)
    ref, mag = _eval(c, x, w, b, gate, torch.float64, "cuda")
    assert out.shape == ref.shape and bool(torch.isfinite(out).all())
    if kind != "random":
        assert float(mag.max()) * 1024 < 2 ** 24                          # what the exactness rests on
        want = ref.float()
        assert float(ref.abs().max()) > 0
        assert bool((want.double() == ref).all())
        same = torch.equal(out, want)
        report("conv_forms", case=T.case_id(c), plan=T.plan_name(p), operands=kind, exact=bool(same))
        assert same, _mismatch(out, want)
        if gate is not None:
            assert bool((gate == 0).any()) and bool((out[gate == 0] == 0).all())
        return
    n32 = _r32_images(c)
    r32 = elem_ratio(_eval(c, x, w, b, gate, torch.float32, "cpu", n32, mass=False)[0].cuda(), ref[:n32], mag[:n32])
    bar = elem_bar(r32, c.split)
    ratio = elem_ratio(out, ref, mag)
    err = float((out.double() - ref).abs().sum() / ref.abs().sum())
    report("conv_forms", case=T.case_id(c), plan=T.plan_name(p), operands=kind, ratio=ratio, r32=r32, bar=bar, rel_l1=err)
    print("%s: %s ratio %.3e r32 %.3e bar %.3e rel_l1 %.3e" % (T.case_id(c), T.plan_name(p), ratio, r32, bar, err))
    assert err < (2e-5 if c.split else 2e-6), err                         # the whole-tensor bars of tests/test_gpu_conv_op.py
    assert ratio < bar, (ratio, r32, bar)


# ---------------------------------------------------------------- the 2:4-sparse consumer of a pooled boundary (csrc/conv_sparse.h)
SPARSE_CASES = [  # NB, Hp, Wp, Cin (output columns N), Cout (K side): those of tests/test_gpu_conv_sparse.py
    (3, 14, 14, 256, 32), (2, 28, 28, 256, 48), (5, 7, 5, 256, 16), (1, 3, 17, 512, 64), (40, 14, 14, 512, 512)]
SPARSE_FORMS = {"choice": 1, "large": 1 | (2 << 8), "small": 1 | (4 << 8)}     # lrp_op_conv_pool_sparse's reps: one launch, the form forced


def _expand(sc, pos):
    NB, Hp, Wp, C = sc.shape
    S = torch.zeros((NB, 2 * Hp, 2 * Wp, C), dtype=sc.dtype, device=sc.device)
    for q in range(4):
        S[:, (q >> 1)::2, (q & 1)::2, :] = torch.where(pos == q, sc, torch.zeros_like(sc))
    return S


def _sparse_graph(S, w, gate):
    return F.conv_transpose2d(S.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1) * gate


@pytest.mark.parametrize("kind", OPERANDS)
@pytest.mark.parametrize("case", SPARSE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_sparse_consumer_against_float64(case, kind):
    """out = gate x conv_transpose(S, w), S the pooled relevance expanded to its windows' positions; one reference for the
    launcher's choice and both forced forms.  exact_a: the 1/1024 grid on sc, integers on w; exact_b: the reverse."""
    from lrp_imagecaptioning_amd.engine import op_conv_pool_sparse
    NB, Hp, Wp, Cin, Cout = case
    seed = sum(case) + 7 * OPERANDS.index(kind)
    rs = np.random.RandomState(seed)
    scs, ws = (NB, Hp, Wp, Cout), (3, 3, Cin, Cout)
    if kind == "exact_a":
        sc, w = _grid(rs, scs), rs.randint(0, 4, size=ws).astype(np.float32)
    elif kind == "exact_b":
        sc, w = rs.randint(-3, 4, size=scs).astype(np.float32), _grid(rs, ws, 0)
    else:
        sc = rs.standard_normal(scs).astype(np.float32)
        w = np.abs(rs.standard_normal(ws) / np.sqrt(9 * Cout)).astype(np.float32)
    w[rs.uniform(size=ws) < 0.3] = 0.0
    sc = torch.as_tensor(sc).cuda()
    pos = torch.as_tensor(rs.randint(0, 4, size=scs).astype(np.uint8)).cuda()
    gate = _gate((NB, 2 * Hp, 2 * Wp, Cin), seed, kind != "random")
    S, wt = _expand(sc, pos), torch.as_tensor(w).cuda()
    ref = _sparse_graph(S.double(), wt.double(), gate.double())
    mag = _sparse_graph(S.double().abs(), wt.double().abs(), gate.double())
    if kind == "random":
        n32 = max(1, min(NB, int(4e9 // (4 * Hp * Wp * 9 * Cin * Cout))))
        r32 = elem_ratio(_sparse_graph(S[:n32].cpu(), wt.cpu(), gate[:n32].cpu()).cuda(), ref[:n32], mag[:n32])
        bar = elem_bar(r32, True)
    else:
        assert float(mag.max()) * 1024 < 2 ** 24
        want = ref.float()
        assert bool((want.double() == ref).all()) and float(ref.abs().max()) > 0
    for form, reps in SPARSE_FORMS.items():
        out = op_conv_pool_sparse(sc, pos, w, gate, reps=reps)
        if kind != "random":
            same = torch.equal(out, want)
            report("conv_forms_sparse", case=list(case), form=form, operands=kind, exact=bool(same))
            assert same, (form, _mismatch(out, want))
            assert bool((out[gate == 0] == 0).all())
            continue
        ratio = elem_ratio(out, ref, mag)
        err = float((out.double() - ref).abs().sum() / ref.abs().sum())
        report("conv_forms_sparse", case=list(case), form=form, operands=kind, ratio=ratio, r32=r32, bar=bar, rel_l1=err)
        print("sparse %s %s: ratio %.3e r32 %.3e bar %.3e rel_l1 %.3e" % (case, form, ratio, r32, bar, err))
        assert err < 2e-5, (form, err)
        assert ratio < bar, (form, ratio, r32, bar)


# ---------------------------------------------------------------- the fine-tune step's products (csrc/train_gemm.h, train_gemm_bf16.h)
WGRAD_CASES = [(3, 14, 14, 136, 72), (1, 5, 5, 8, 8), (2, 6, 10, 24, 40)]        # NB, H, W, Cin, Cout; the last: H != W


def _wgrad(x, dz):
    """torch's own weight / bias gradient of the 3x3 'same' conv in the dtype of x -> (dw HWIO, db)"""
    Cin, Cout = x.shape[3], dz.shape[3]
    w = torch.zeros((Cout, Cin, 3, 3), dtype=x.dtype, requires_grad=True)
    b = torch.zeros(Cout, dtype=x.dtype, requires_grad=True)
    F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1).backward(dz.permute(0, 3, 1, 2))
    return w.grad.permute(2, 3, 1, 0).contiguous(), b.grad


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_wgrad_against_float64(case, bf16):
    """Exact: integers in {-3..3} x {-2..2} (8 significant bits at the most, so the bf16 rounding is exact, and every sum stays
    below 6 K < 2^24).  Random: element bound against the float64 gradient — of the bf16-rounded operands for the bf16 kernel,
    whose products are then exact in fp32 as well, so the fp32 bar holds for both."""
    from lrp_imagecaptioning_amd.engine import op_conv_wgrad
    NB, H, W, Cin, Cout = case
    g = torch.Generator().manual_seed(sum(case))
    assert 6 * NB * H * W < 2 ** 24
    x = torch.randint(-3, 4, (NB, H, W, Cin), generator=g).float()
    dz = torch.randint(-2, 3, (NB, H, W, Cout), generator=g).float()
    dw, db = op_conv_wgrad(x.cuda(), dz.cuda(), bf16=bf16)
    want_w, want_b = _wgrad(x.double(), dz.double())
    assert float(want_w.abs().max()) > 0
    assert torch.equal(dw.cpu(), want_w.float()), _mismatch(dw.cpu(), want_w.float())
    assert torch.equal(db.cpu(), want_b.float())

    x = torch.randn((NB, H, W, Cin), generator=g)
    dz = torch.randn((NB, H, W, Cout), generator=g) * (torch.rand((NB, H, W, Cout), generator=g) > 0.5)
    if bf16:
        x, dz = x.bfloat16().float(), dz.bfloat16().float()
    dw, db = op_conv_wgrad(x.cuda(), dz.cuda(), bf16=bf16)
    want_w, want_b = _wgrad(x.double(), dz.double())
    mag_w, mag_b = _wgrad(x.double().abs(), dz.double().abs())
    w32, b32 = _wgrad(x, dz)
    r32, r32b = elem_ratio(w32, want_w, mag_w), elem_ratio(b32, want_b, mag_b)
    ratio, ratio_b = elem_ratio(dw.cpu(), want_w, mag_w), elem_ratio(db.cpu(), want_b, mag_b)
    report("conv_forms_wgrad", case=list(case), bf16=bf16, ratio=ratio, r32=r32, bar=elem_bar(r32, False), ratio_db=ratio_b, r32_db=r32b)
    print("wgrad %s bf16=%s: ratio %.3e r32 %.3e bar %.3e | db %.3e r32 %.3e" % (case, bf16, ratio, r32, elem_bar(r32, False), ratio_b, r32b))
    assert ratio < elem_bar(r32, False), (ratio, r32)
    assert ratio_b < elem_bar(r32b, False), (ratio_b, r32b)


SGEMM_CASES = [  # (M, N, K, transA, transB): the small ones of tests/test_gpu_train.py
    (32, 2048, 512, False, False), (32, 512, 2048, False, True), (136, 72, 5000, True, False), (64, 64, 100000, True, False),
    (3, 64, 70000, True, False), (1, 1, 1, False, False), (129, 257, 33, False, True)]


@pytest.mark.parametrize("M,N,K,ta,tb", SGEMM_CASES)
def test_sgemm_on_integers_is_exact(M, N, K, ta, tb):
    """integers in {-3..3}: every sum stays below 9 K + 8 < 2^24, so the product is exact whatever the order — with the K split
    (a workspace), without it, and accumulating into C.  Then random operands under the fp32 element bar."""
    from lrp_imagecaptioning_amd.engine import op_sgemm
    assert 9 * K + 8 < 2 ** 24
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N)
    pad = 8                                                 # views into wider buffers, as the step's operands are

    def views(make):
        A = make((K, M + pad) if ta else (M, K + pad))[:, :(M if ta else K)]
        B = make((N, K + pad) if tb else (K, N + pad))[:, :(K if tb else N)]
        return A, B, (A.double().t() if ta else A.double()), (B.double().t() if tb else B.double())
    A, B, Ad, Bd = views(lambda s: torch.randint(-3, 4, s, device="cuda", generator=g).float())
    C0 = torch.randint(-8, 9, (M, N), device="cuda", generator=g).float()
    want = Ad @ Bd
    for split in (True, False):
        got = op_sgemm(A, B, ta, tb, split=split)
        assert torch.equal(got, want.float()), (split, _mismatch(got, want.float()))
        got = op_sgemm(A, B, ta, tb, C_init=C0.clone(), split=split)
        assert torch.equal(got, (want + C0.double()).float()), (split, "accumulate")

    A, B, Ad, Bd = views(lambda s: torch.randn(s, device="cuda", generator=g))
    C0 = torch.randn((M, N), device="cuda", generator=g)
    want, mag = Ad @ Bd + C0.double(), Ad.abs() @ Bd.abs() + C0.double().abs()
    a32, b32 = (A.cpu().t() if ta else A.cpu()), (B.cpu().t() if tb else B.cpu())
    r32 = elem_ratio((a32 @ b32 + C0.cpu()).cuda(), want, mag)
    ratio = elem_ratio(op_sgemm(A, B, ta, tb, C_init=C0.clone()), want, mag)
    report("conv_forms_sgemm", case=[M, N, K, ta, tb], ratio=ratio, r32=r32, bar=elem_bar(r32, False))
    print("sgemm %s: ratio %.3e r32 %.3e bar %.3e" % ((M, N, K, ta, tb), ratio, r32, elem_bar(r32, False)))
    assert ratio < elem_bar(r32, False), (ratio, r32)
