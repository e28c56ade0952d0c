#!/usr/bin/env python3
"""Do two builds of liblrp_hip.so plan every convolution alike?  No GPU needed.

  conv_plan_sweep.py A.so B.so [--jobs J]

loads both libraries through ctypes, asks lrp_conv_plan (include/lrp_hip.h) of each the same questions and asserts that all
eleven output words are equal.  The grid: 7 epilogues x 3 operand formats x terms {5, 7, 23}; every subset of the eight
LRP_PLAN_* flags the plan does not refuse for that (epilogue, format) whatever the shape — the refused subsets are asked too, on
one batch size, and must be refused by both —; NB {1, 3, 8, 72, 90}; H = W {7, 14, 17, 28, 56, 112, 224} and 28 x 20; N and Cin
{8, 24, 40, 54, 64, 72, 128, 136, 256, 512}; taps {1, 9}; split = N / 2 for the dual forward.  Once under the default
switches and once under each of SWITCHES (set the way engine.switches sets them: environment + lrp_reload_switches).

Record of the commit that split conv_igemm.h by role against its parent: conv_table_ab.txt."""
import ctypes
import itertools
import multiprocessing
import os
import sys

EPIS, PRECS, TERMS = range(7), range(3), (5, 7, 23)
RELU, BIAS, MUL, UP2, DUAL, STORE, IMG = EPIS
FP32, BF16X3, F16X2 = PRECS
FRAG, JOIN, DUAL_IL, GMASK, UP2_SRC, IMG_PART, POOL_GC, DUAL_MUL = (1 << i for i in range(8))
NBS = (1, 3, 8, 72, 90)
HWS = [(h, h) for h in (7, 14, 17, 28, 56, 112, 224)] + [(28, 20)]
CHANNELS = (8, 24, 40, 54, 64, 72, 128, 136, 256, 512)
SWITCHES = [{}] + [{k: v} for k, v in (("LRP_CONV_HALO", 0), ("LRP_CONV_HALO", 2), ("LRP_CONV_BREG", 0), ("LRP_CONV_BREG8", 0),
                                       ("LRP_CONV_BREG4", 0), ("LRP_CONV_SMALL", 0), ("LRP_CONV_MID", 0), ("LRP_POOL_FUSED", 0),
                                       ("LRP_UP2_PW", 0))]


def refused_whatever_the_shape(epi, prec, flags):
    """include/lrp_hip.h on the LRP_PLAN_* requests: what each may ride on"""
    mul = epi in (MUL, UP2)
    asked = flags & (UP2_SRC | IMG_PART | POOL_GC)
    if flags & GMASK and (epi != MUL or prec != FP32 or asked or flags & DUAL_MUL):
        return True
    if flags & DUAL_MUL and (not mul or prec == F16X2 or asked or flags & (FRAG | JOIN)):
        return True
    if flags & (UP2_SRC | IMG_PART) and not mul:
        return True
    if flags & POOL_GC and (epi != DUAL or prec != F16X2 or not flags & DUAL_IL or flags & (UP2_SRC | IMG_PART)):
        return True
    return False


def sweep(job):
    a_path, b_path, env = job
    for k in [k for k in os.environ if k.startswith("LRP_")]:      # (a pool worker may have run another setting before)
        del os.environ[k]
    for k, v in env.items():
        os.environ[k] = str(v)
    libs = [ctypes.CDLL(p) for p in (a_path, b_path)]
    for lib in libs:
        assert lib.lrp_reload_switches() == 0
    fa, fb = (lib.lrp_conv_plan for lib in libs)
    oa, ob = (ctypes.c_int32 * 11)(), (ctypes.c_int32 * 11)()
    asks = ok = 0
    for epi, prec, terms, flags in itertools.product(EPIS, PRECS, TERMS, range(256)):
        trivial = refused_whatever_the_shape(epi, prec, flags)
        for NB in ((8,) if trivial else NBS):
            for (H, W), N, Cin, taps in itertools.product(HWS, CHANNELS, CHANNELS, (1, 9)):
                split = N // 2 if epi == DUAL else 0
                ra = fa(epi, prec, terms, NB, H, W, N, Cin, taps, split, flags, oa)
                rb = fb(epi, prec, terms, NB, H, W, N, Cin, taps, split, flags, ob)
                if ra != 0 or rb != 0 or oa[:] != ob[:]:
                    raise AssertionError("%s: epi %d prec %d terms %d flags %#x NB %d %dx%d N %d Cin %d taps %d: %d %s | %d %s" % (
                        env, epi, prec, terms, flags, NB, H, W, N, Cin, taps, ra, oa[:], rb, ob[:]))
                assert not (trivial and oa[0]), ("not refused", env, epi, prec, terms, flags, NB, H, W, N, Cin, taps)
                asks += 1
                ok += oa[0]
    return env, asks, ok


if __name__ == "__main__":
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else 8
    a_path, b_path = (os.path.abspath(p) for p in sys.argv[1:3])
    with multiprocessing.get_context("spawn").Pool(jobs) as pool:     # (processes: a setting is the environment of its worker)
        rows = pool.map(sweep, [(a_path, b_path, env) for env in SWITCHES], chunksize=1)
    for env, asks, ok in rows:
        print("  %-18s %9d asks, %9d answered ok, %9d refused: all eleven words equal" % (
            " ".join("%s=%s" % kv for kv in env.items()) or "default switches", asks, ok, asks - ok))
    print("%d asks under %d switch settings: the two builds answer all eleven words alike" % (sum(r[1] for r in rows), len(rows)))
