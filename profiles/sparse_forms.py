#!/usr/bin/env python3
"""Per-launch time of the two tile forms of conv_sparse_kernel (csrc/conv_sparse.h: 256 windows x 256 columns on 8 waves, 64
windows x 128 columns on 4 waves) at small token counts, operator level, each form forced through the measurement bits of
lrp_op_conv_pool_sparse's `reps`.  The time of a launch = (101 launches - 1 launch) / 100, best of three.  Where the large form
overtakes the small one is the constant CONV_SPARSE_SMALL_BLOCKS.
Usage (GPU box): python profiles/sparse_forms.py"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lrp_imagecaptioning_amd.engine import op_conv_pool_sparse  # noqa: E402

SHAPES = {"block4_conv3": (14, 14, 512, 512), "block3_conv3": (28, 28, 256, 256)}
for name, (Hp, Wp, Cin, Cout) in SHAPES.items():
    for NB in (1, 3, 5, 10, 15, 20, 30, 40, 60, 90):
        rs = np.random.RandomState(0)
        g = torch.Generator(device="cuda").manual_seed(1)
        sc = torch.randn((NB, Hp, Wp, Cout), device="cuda", generator=g)
        pos = torch.randint(0, 4, (NB, Hp, Wp, Cout), device="cuda", generator=g, dtype=torch.uint8)
        w = np.abs(rs.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cout)).astype(np.float32)
        gate = torch.rand((NB, 2 * Hp, 2 * Wp, Cin), device="cuda", generator=g)
        res = {}
        for form, bit in (("large", 2), ("small", 4)):
            op_conv_pool_sparse(sc, pos, w, gate, reps=3 | (bit << 8))
            best = 1e9
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                op_conv_pool_sparse(sc, pos, w, gate, reps=1 | (bit << 8))
                t1 = time.perf_counter()
                op_conv_pool_sparse(sc, pos, w, gate, reps=101 | (bit << 8))
                t2 = time.perf_counter()
                best = min(best, ((t2 - t1) - (t1 - t0)) / 100 * 1e6)
            res[form] = best
        blocks = 4 * ((NB * Hp + 17) // 18) * ((Wp + 13) // 14) * (Cin // 256)
        print("%s NB=%d large-form workgroups %d: large %.1f us, small %.1f us" % (name, NB, blocks, res["large"], res["small"]), flush=True)
