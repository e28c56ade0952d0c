"""Helpers shared by the -m gpu parity tests."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "gpurun_out")


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def band_errors(out, ref):
    """Per image row and per image column of one (H, W, C) map: sum|out-ref| over the band / sum|ref| over the band, in
    float64 -> (rows (H,), columns (W,)).  A band whose reference mass is exactly zero scores 0 if `out` is exactly zero
    there and inf otherwise."""
    a = np.asarray(out, dtype=np.float64)
    b = np.asarray(ref, dtype=np.float64)
    if a.shape != b.shape or a.ndim != 3:
        raise ValueError("band_errors takes two (H, W, C) maps of one shape")
    res = []
    for axes in ((1, 2), (0, 2)):
        num, den, mass = np.abs(a - b).sum(axis=axes), np.abs(b).sum(axis=axes), np.abs(a).sum(axis=axes)
        e = num / np.where(den > 0, den, 1.0)
        res.append(np.where(den > 0, e, np.where(mass > 0, np.inf, 0.0)))
    return res[0], res[1]


def band_rel_l1(out, ref, where=False):
    """The largest band_errors value over every image row and every image column: what a whole-map rel_l1 cannot see, a
    dropped, duplicated or misplaced border row (about 1.0 on that band, a few 1e-5 of the map's mass on a deep encoder).
    where=True -> (value, "row i" | "col j") of the worst band."""
    rows, cols = band_errors(out, ref)
    i, j = int(np.argmax(rows)), int(np.argmax(cols))
    v, w = (float(rows[i]), "row %d" % i) if rows[i] >= cols[j] else (float(cols[j]), "col %d" % j)
    return (v, w) if where else v


def band_bar(ref32, ref, floor=1e-4, factor=10.0):
    """The bound of band_rel_l1 for an engine result: max(floor, factor x the worst band of the SAME oracle evaluated in
    float32 against its float64 evaluation), over the maps of a batch.  Measured against the reference, never against
    the engine; the factor covers arithmetic that is not the float32 restatement's (split-bf16 products, another summation
    order, fp16-pair activations); a broken band scores about 1.0.  -> (bar, float32 restatement's worst band)"""
    e32 = max(band_rel_l1(a, b) for a, b in zip(ref32, ref))
    return max(floor, factor * e32), e32


def elem_ratio(out, ref, mag):
    """max |out - ref| / mag over the elements of one operator result, in float64: `mag` is the mass each element was summed
    from (|gate| x (|in| conv |w|), plus |bias|), so the ratio is an error per unit of what went into THAT element, and one wrong
    pixel among millions scores what it would score alone — the whole-tensor rel_l1 divides it by the tensor.  An element without
    mass must be exactly zero: the result is inf if one is not.  numpy arrays or torch tensors (of one device)."""
    if hasattr(out, "detach"):
        import torch
        d, m = (out.double() - ref.double()).abs(), mag.double()
        if tuple(d.shape) != tuple(m.shape):
            raise ValueError("elem_ratio takes three arrays of one shape")
        if bool(((m <= 0) & (d > 0)).any()):
            return float("inf")
        return float((d / torch.where(m > 0, m, torch.ones_like(m))).max()) if d.numel() else 0.0
    d = np.abs(np.asarray(out, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    m = np.asarray(mag, dtype=np.float64)
    if d.shape != m.shape:
        raise ValueError("elem_ratio takes three arrays of one shape")
    if ((m <= 0) & (d > 0)).any():
        return float("inf")
    return float((d / np.where(m > 0, m, 1.0)).max()) if d.size else 0.0


def elem_bar(r32, split):
    """The bound of elem_ratio for an operator result, from the reference alone: `r32` is elem_ratio of torch's float32
    evaluation of the same graph.  fp32 operator: max(2^-22, 10 r32) — 10 for a float32 sum in another order (as band_bar),
    2^-22 = four ulp for the epilogue's roundings when K is tiny.  Split-bf16 operator: 2^-16 more, the worst case per product
    of the three-term split (csrc/conv_igemm.h header)."""
    return (2.0 ** -16 if split else 0.0) + max(2.0 ** -22, 10.0 * r32)


def transpose_spatial(w):
    """A weight dict with every 4-d (kh, kw, cin, cout) kernel transposed in its two spatial axes: the network that maps the
    transposed image to the transposed result."""
    return {k: (np.ascontiguousarray(np.swapaxes(v, 0, 1)) if np.ndim(v) == 4 else v) for k, v in w.items()}


# the ResNet geometries of the H != W tests: name -> (stacks, stem, (H, W)); sides are multiples of 4 and the resolution in
# front of every stride-2 block is even (csrc/resnet_encoder.h init)
NONSQUARE_RESNETS = {
    "stem64": (((32, 2), (64, 2)), 64, (72, 120)),          # stem map 36 x 60, top map 9 x 15
    "mid": (((8, 2), (16, 3), (32, 2)), 16, (48, 80)),      # top map 3 x 5
    "tiny": (((4, 2), (8, 2)), 8, (24, 40)),                # widths % 8 != 0
    "wide": (((64, 1), (128, 1), (256, 2), (512, 1)), 64, (160, 96)),   # ResNet-101's channel widths, top map 5 x 3
}


def report(name, **kv):
    """Append a json line to gpurun_out/parity.jsonl so one GPU call leaves a full record."""
    try:
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, "parity.jsonl"), "a") as f:
            kv["name"] = name
            f.write(json.dumps({k: (float(v) if isinstance(v, (np.floating, float)) else v) for k, v in kv.items()}) + "\n")
    except Exception:
        pass
