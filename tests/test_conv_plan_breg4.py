"""The launch plan's FORM_BREG4 / FORM_BREG4_POOL (csrc/conv_plan.h conv_plan, through lrp_conv_plan): the launches on the 4-wave
128 x 128 resident-image tile whose N is a multiple of the tile — the dense split-bf16 EPI_MUL launches of the reverse walk and
the interleaved fp16-pair dual forward — take their weights from registers when a fragment-major copy of the weights exists.
Tile and geometry stay those of FORM_HALO / FORM_POOL.  Host arithmetic only — no GPU."""
import pytest

from lrp_imagecaptioning_amd import _capi as K
from lrp_imagecaptioning_amd.build import build_library
from lrp_imagecaptioning_amd.engine import conv_plan, switches
from lrp_imagecaptioning_amd.synthetic import VGG16_CFG

HALO, POOL, BREG4, BREG4_POOL = K.LRP_FORM_HALO, K.LRP_FORM_POOL, K.LRP_FORM_BREG4, K.LRP_FORM_BREG4_POOL
MUL, DUAL, BF, H2, FP32 = K.LRP_EPI_MUL, K.LRP_EPI_FWD_DUAL, K.LRP_OPND_BF16X3, K.LRP_OPND_F16X2, K.LRP_OPND_FP32
FRAG, UP2, IL, GC = K.LRP_PLAN_FRAG, K.LRP_PLAN_UP2_SRC, K.LRP_PLAN_DUAL_IL, K.LRP_PLAN_POOL_GC
GEOM = ("BM", "BN", "threads", "tw", "th", "hrows", "m_tiles", "n_tiles")
WALK = ("block3_conv1", "block2_conv2")
FWD = [c for c in VGG16_CFG[1:]]                        # the 12 dual convs behind the image layer
B = 32


@pytest.fixture(scope="module", autouse=True)
def _library():
    build_library()


def _layer(name):
    H = 224
    for n, cin, cout, pool in VGG16_CFG:
        if n == name:
            return H, cin, cout, pool
        H = H // 2 if pool else H
    raise KeyError(name)


def _walk(tokens, name, flags=0, prec=BF, taps=9):
    H, cin, cout, _ = _layer(name)
    return conv_plan(MUL, prec, tokens, H, H, cin, cout, taps=taps, flags=flags)


def _fwd(name, flags=0, terms=7, nb=B, prec=H2):
    H, cin, cout, _ = _layer(name)
    return conv_plan(DUAL, prec, nb, H, H, 2 * cout, cin, terms=terms, split=cout, flags=flags)


def test_constants():
    assert (K.LRP_FORM_BREG4, K.LRP_FORM_BREG4_POOL) == (7, 8)


@pytest.mark.parametrize("name", WALK)
def test_vgg16_walk_takes_the_form_with_todays_geometry(name):
    today = _walk(320, name)
    assert today["ok"] == 1 and today["form"] == HALO and (today["BM"], today["BN"], today["threads"]) == (128, 128, 256), today
    p = _walk(320, name, FRAG)
    assert p["ok"] == 1 and p["form"] == BREG4, p
    assert [p[k] for k in GEOM] == [today[k] for k in GEOM], (p, today)


def test_block2_conv2_takes_it_with_the_compact_pool_interface():
    today = _walk(320, "block2_conv2", UP2)
    assert today["ok"] == 1 and today["form"] == HALO, today
    p = _walk(320, "block2_conv2", FRAG | UP2)
    assert p["ok"] == 1 and p["form"] == BREG4, p
    assert [p[k] for k in GEOM] == [today[k] for k in GEOM], (p, today)


@pytest.mark.parametrize("terms", [7, 23])
@pytest.mark.parametrize("name", [c[0] for c in FWD])
def test_vgg16_dual_forward_takes_the_form_with_todays_geometry(name, terms):
    today = _fwd(name, IL, terms)
    assert today["ok"] == 1 and today["form"] == HALO and (today["BM"], today["BN"]) == (128, 128), today
    p = _fwd(name, FRAG | IL, terms)
    assert p["ok"] == 1 and p["form"] == BREG4, p
    assert [p[k] for k in GEOM] == [today[k] for k in GEOM], (p, today)
    if _layer(name)[3]:
        today = _fwd(name, IL | GC, terms)
        assert today["ok"] == 1 and today["form"] == POOL, today
        p = _fwd(name, FRAG | IL | GC, terms)
        assert p["ok"] == 1 and p["form"] == BREG4_POOL, p
        assert [p[k] for k in GEOM] == [today[k] for k in GEOM], (p, today)


def test_four_pooled_layers():
    assert sum(1 for c in FWD if c[3]) == 4


@pytest.mark.parametrize("name", WALK)
def test_walk_answers_that_stay(name):
    H, cin, cout, _ = _layer(name)
    assert _walk(320, name)["form"] == HALO                                   # without the copy
    with switches(LRP_CONV_BREG4=0):
        assert _walk(320, name, FRAG) == _walk(320, name)
        assert _walk(320, name, FRAG | UP2) == _walk(320, name, UP2)
    for extra in (K.LRP_PLAN_JOIN, K.LRP_PLAN_IMG_PART):
        with switches(LRP_CONV_BREG4=0):
            today = _walk(320, name, FRAG | extra)
        assert _walk(320, name, FRAG | extra) == today, extra
    with switches(LRP_CONV_BREG4=0):
        today = [_walk(320, name, FRAG, prec=FP32), conv_plan(MUL, BF, 320, H, H, 136, cout, flags=FRAG), _walk(320, name, FRAG, taps=1),
                 _walk(3, name, FRAG), _walk(320, name, FRAG, prec=H2), conv_plan(K.LRP_EPI_MUL_UP2, BF, 320, H, H, cin, cout, flags=FRAG)]
    now = [_walk(320, name, FRAG, prec=FP32), conv_plan(MUL, BF, 320, H, H, 136, cout, flags=FRAG), _walk(320, name, FRAG, taps=1),
           _walk(3, name, FRAG), _walk(320, name, FRAG, prec=H2), conv_plan(K.LRP_EPI_MUL_UP2, BF, 320, H, H, cin, cout, flags=FRAG)]
    if today[3]["form"] == HALO and today[3]["BM"] == 128 and today[3]["BN"] == 128:
        # three tokens of 112 x 112 maps are 304 tiles: above the small-grid rules, so today's answer is itself the pipelined
        # 128 x 128 resident-image launch, which is exactly what the form replaces — everything but `form` stays
        assert name == "block2_conv2" and now[3] == dict(today[3], form=BREG4), (now[3], today[3])
        now[3] = today[3]
    assert now == today
    assert all(p["form"] not in (BREG4, BREG4_POOL) for p in now), now
    assert _walk(3, "block3_conv1", FRAG)["form"] == K.LRP_FORM_SMALL
    assert _walk(320, name, FRAG)["form"] == BREG4                           # and back


@pytest.mark.parametrize("name", [c[0] for c in FWD])
def test_forward_answers_that_stay(name):
    H, cin, cout, pool = _layer(name)
    assert _fwd(name, IL)["form"] == HALO
    asks = [lambda: _fwd(name, FRAG),                                         # stacked rows
            lambda: _fwd(name, FRAG | IL, prec=FP32),
            lambda: conv_plan(DUAL, H2, B, H, H, 2 * 68, cin, split=68, flags=FRAG),          # N = 136 (stacked: 68 is no multiple of 32)
            lambda: conv_plan(DUAL, H2, B, H, H, 2 * cout, cin, taps=1, split=cout, flags=FRAG | IL),
            lambda: _fwd(name, FRAG | IL, nb=1)]                            # one image: the small-grid tiles below 56 x 56
    with switches(LRP_CONV_BREG4=0):
        off = _fwd(name, FRAG | IL), _fwd(name, FRAG | IL | GC), _fwd(name, FRAG | IL, 23)
        today = [f() for f in asks]
    assert off == (_fwd(name, IL), _fwd(name, IL | GC), _fwd(name, IL, 23))
    now = [f() for f in asks]
    n = 5 if H <= 28 else 4
    assert now[:n] == today[:n]
    assert all(p["form"] not in (BREG4, BREG4_POOL) for p in now[:n]), now


def test_breg8_switch_changes_no_128_row_answer():
    asks = [lambda n=n, f=f: _walk(320, n, f) for n in WALK for f in (0, FRAG, FRAG | UP2)]
    asks += [lambda c=c, f=f, t=t: _fwd(c[0], f, t) for c in FWD for f in (IL, FRAG | IL) for t in (7, 23)]
    asks += [lambda: conv_plan(MUL, BF, 120, 28, 28, 256, 40, flags=FRAG)]
    on = [f() for f in asks]
    with switches(LRP_CONV_BREG8=0):
        off = [f() for f in asks]
    assert on == off
    assert all(p["BM"] == 128 for p in on)


def test_256_row_and_narrow_answers_do_not_change():
    asks = [lambda: _walk(320, "block4_conv2", FRAG), lambda: _walk(320, "block2_conv1", FRAG), lambda: _walk(320, "block1_conv2", FRAG),
            lambda: _walk(320, "block1_conv2", FRAG | K.LRP_PLAN_IMG_PART | UP2)]
    on = [f() for f in asks]
    with switches(LRP_CONV_BREG4=0):
        off = [f() for f in asks]
    assert on == off
    assert on[0]["form"] == K.LRP_FORM_BREG8 and on[1]["form"] == K.LRP_FORM_BREG
