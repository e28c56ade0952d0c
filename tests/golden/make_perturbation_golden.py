#!/usr/bin/env python3
"""Generate tests/golden/perturbation_*.npz by running the REFERENCE's own Perturbation class
(innvestigate/tools/perturbate.py) on seeded inputs.

Tooling like make_golden.py, whose stub finder it reuses: the reference module is imported from where it lies, and only
its numeric inputs and outputs are written.  Each fixture holds x and the analysis (n, H, W, C) float32, the reference's
aggregate_regions and compute_region_ordering results, and perturbate_on_batch for every (function, k, value range).
An output is stored as its difference against x (against clip(x) when a value range is set and k >= 1): the flat indices
whose bits differ and the values there (tests/perturbation_ref.py golden_output decodes it) — lossless, and a few tens of
kB per file instead of 36 full copies of x.

Two properties of the inputs are asserted here because the tests rely on them:
  * the region means are well separated (a per-region constant from a permutation plus noise of amplitude 0.1): the smallest
    gap between the reference's own sorted region means is >= 1e-3 of their largest magnitude, so neither float32 rounding
    nor the unspecified order of quicksort ties can move a rank;
  * sample 0 lies inside the value range.  The reference clips the WHOLE batch inside its loop as soon as one region is
    perturbed (PT:142-146), so every region but the first perturbed one of the batch is computed from clipped data; that
    one region depends on what else is in the batch.  With sample 0 inside the range the clip does not change it and the
    fixture holds no such order-dependent value; samples 1 and 2 reach far outside the range.

Usage:  python tests/golden/make_perturbation_golden.py [--ref /root/reference]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402  (the stub finder for keras & co.)
from perturbation_ref import FUNCTIONS, RANGES, geometry  # noqa: E402

CASES = [  # name, seed, H, W, C, region
    ("perturbation_18x27_r9", 0, 18, 27, 3, (9, 9)),
    ("perturbation_20x29_r9", 1, 20, 29, 3, (9, 9)),
    ("perturbation_23x23_r4x6", 2, 23, 23, 3, (4, 6)),
    ("perturbation_20x29_r9_c1", 3, 20, 29, 1, (9, 9)),
]
N = 3


def make_inputs(seed, H, W, C, region):
    rs = np.random.RandomState(seed)
    Hr, Wr, bh, bw = geometry(H, W, region)
    nreg = Hr * Wr
    reg = ((np.arange(H) + bh) // region[0])[:, None] * Wr + ((np.arange(W) + bw) // region[1])[None, :]
    analysis = np.empty((N, H, W, C), dtype=np.float32)
    for i in range(N):
        const = (rs.permutation(nreg) - nreg // 2).astype(np.float64)
        analysis[i] = (const[reg][..., None] + 0.1 * rs.uniform(-1, 1, size=(H, W, C))).astype(np.float32)
    x = rs.randn(N, H, W, C).astype(np.float32)
    x[0] = rs.uniform(-0.45, 0.45, size=(H, W, C)).astype(np.float32)
    return x, analysis, nreg


def run_case(P, seed, H, W, C, region):
    x, analysis, nreg = make_inputs(seed, H, W, C, region)
    ks = np.array([0, 1, 2.5, 5, nreg, nreg + 3], dtype=np.float64)
    out = {"x": x, "analysis": analysis, "region": np.array(region, dtype=np.int32), "ks": ks}
    # the reference's intermediate results, by its own methods in the order perturbate_on_batch calls them
    p = P.Perturbation("zeros", region_shape=region)
    a = np.moveaxis(analysis, 3, 1)
    a = p.reduce_function(a, axis=1, keepdims=True)
    if not np.all(np.array(a.shape[2:]) % region == 0):
        a, _ = p.pad(a)
    agg = p.aggregate_regions(a)
    ranks = p.compute_region_ordering(agg)
    s = np.sort(agg.reshape(N, -1).astype(np.float64), axis=-1)
    gap = (np.diff(s, axis=-1).min(axis=-1) / np.abs(s).max(axis=-1)).min()
    assert gap >= 1e-3, gap
    out["aggregated"] = agg.reshape(N, -1)
    out["ranks"] = ranks.reshape(N, -1).astype(np.int32)
    for ri, rng in enumerate(RANGES):
        if rng is not None:
            assert np.abs(x[0]).max() < min(-rng[0], rng[1]) and np.abs(x[1:]).max() > 2 * max(-rng[0], rng[1])
        for fn in FUNCTIONS:
            for ki, k in enumerate(ks):
                kk = int(k) if float(k).is_integer() else float(k)
                p = P.Perturbation(fn, num_perturbed_regions=kk, region_shape=region, value_range=rng)
                y = p.perturbate_on_batch(x.copy(), analysis.copy())
                assert y.dtype == np.float32 and y.shape == x.shape
                base = np.clip(x, np.float32(rng[0]), np.float32(rng[1])) if (rng is not None and k >= 1) else x
                idx = np.flatnonzero(y.reshape(-1).view(np.uint32) != base.reshape(-1).view(np.uint32))
                key = "%s_k%d_r%d" % (fn, ki, ri)
                out["idx_" + key] = idx.astype(np.int32)
                out["val_" + key] = y.reshape(-1)[idx]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    sys.meta_path.insert(0, make_golden._StubFinder())
    sys.path.insert(0, args.ref)
    import innvestigate.tools.perturbate as P
    for name, seed, H, W, C, region in CASES:
        out = run_case(P, seed, H, W, C, region)
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, **out)
        print("%-28s regions=%d  size=%.1f KB" % (name, out["ranks"].shape[1], os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
