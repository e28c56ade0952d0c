#!/usr/bin/env python3
"""Caption search with the beam bookkeeping on the host (`beam.search`, the default) and on the device
(lrp_decoder_beam_search, `_beam_search(on_device=True)`) on an MI355X: what profiles/beam_device.txt records.

VGG16 captioner at the bench's decoder size (L 196, D 512, H = E = 512, V 10000), beam 3, 20 steps:
  adaptive  1 image                      (3 rows)
  adaptive  32 images on max_images=96   (96 rows, one group)
  grid-TD   32 images on max_images=96
For each, two figures per path, in ms per search (median [min .. max] of REPS wall-clock repetitions after WARMUP, the device idle
before and after each) and captions/s:
  search   features resident: gen_begin, the 20 steps, the captions on the host as Python lists
  call     the whole `_beam_search((None, images))`: float32 images from the host, encoder forward, feature fan-out, search
The two paths alternate repetition by repetition in one process, so that clock and thermal drift fall on both alike; the
captions of the two paths are compared before anything is timed.

Usage (GPU box, repository root): python profiles/beam_device_bench.py [--reps N]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPS, BEAM, STEPS, V = 3, 25, 3, 20, 10000


def _explainer(kind, max_images):
    """An explainer of the reference's class around an engine with a small token budget (nothing is explained here)."""
    import numpy as np
    import lrp_imagecaptioning_amd.explainers as EX
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, gridtd_weights, vgg_weights
    rs = np.random.RandomState(0)
    w = vgg_weights(rs)
    w.update((adaptive_weights if kind == "adaptive" else gridtd_weights)(rs, 196, 512, 512, 512, V))
    cls = EX.ExplainImgCaptioningAdaptiveAttention if kind == "adaptive" else EX.ExplainImgCaptioningGridTDModel
    ex = object.__new__(cls)
    ex._preprocessor = EX.CaptionPreprocessorStub()
    ex._max_caption_length = STEPS
    ex._engine = LRPEngine(decoder=kind, V=V, max_images=max_images, max_tokens=4, max_caption_len=STEPS + 1)
    ex._engine.set_weights(w)
    ex._state_cache, ex.caption = {}, None
    return ex


def _search_only(ex, feat, n_images, on_device):
    """The body of `_beam_search` behind the encoder: features (n_images * BEAM slots) are on the device already."""
    from lrp_imagecaptioning_amd import beam
    eng = ex._engine
    eng.set_features(feat)
    eng.gen_begin(n_images * BEAM)
    if on_device:
        return eng.beam_search_lists(n_images, BEAM, STEPS, 1)

    def step(s, parent, word):
        ids, logp = eng.log_softmax_topk(eng.gen_step(s, parent, word), BEAM)
        return ids.cpu().numpy(), logp.cpu().numpy()
    return beam.search(step, n_images, BEAM, STEPS, 1)


def _alternate(fns, reps):
    import torch
    times = [[] for _ in fns]
    for r in range(WARMUP + reps):
        for i, f in enumerate(fns):
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if r >= WARMUP:
                times[i].append((time.perf_counter() - t) * 1e3)
    return times


def _line(label, ms, n_images):
    med = statistics.median(ms)
    return "  %-14s %8.2f ms [%7.2f .. %7.2f]  %8.0f captions/s" % (label, med, min(ms), max(ms), n_images / med * 1e3)


def case(kind, n_images, max_images, reps):
    import numpy as np
    from lrp_imagecaptioning_amd.synthetic import images
    ex = _explainer(kind, max_images)
    X = images(np.random.RandomState(1), n_images)
    ex._engine.encode_images(X)
    feat = ex._engine.get_features()[:n_images].repeat_interleave(BEAM, dim=0).contiguous()
    host, dev = _search_only(ex, feat, n_images, False), _search_only(ex, feat, n_images, True)
    assert host == dev, "the two paths disagree"
    whole = ex._beam_search((None, X), beam_size=BEAM, on_device=True)
    assert (whole if n_images > 1 else [whole]) == dev
    lens = sorted(len(c[0]) for c in dev)
    print("%s, %d image(s) on max_images=%d, beam %d, %d steps, %d repetitions; captions equal on both paths (lengths %d .. %d)"
          % (kind, n_images, max_images, BEAM, STEPS, reps, lens[0], lens[-1]), flush=True)
    t = _alternate([lambda: _search_only(ex, feat, n_images, False), lambda: _search_only(ex, feat, n_images, True)], reps)
    print(_line("search host", t[0], n_images))
    print(_line("search device", t[1], n_images))
    print("  search device / host: x%.2f of the time" % (statistics.median(t[1]) / statistics.median(t[0])), flush=True)
    t = _alternate([lambda: ex._beam_search((None, X), beam_size=BEAM, on_device=False),
                    lambda: ex._beam_search((None, X), beam_size=BEAM, on_device=True)], reps)
    print(_line("call host", t[0], n_images))
    print(_line("call device", t[1], n_images))
    print("  call device / host: x%.2f of the time" % (statistics.median(t[1]) / statistics.median(t[0])), flush=True)


def main():
    import torch
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else REPS
    assert reps >= 20, "medians of fewer than 20 repetitions are not reported"
    print("device: %s" % torch.cuda.get_device_name(0))
    for kind, n_images, max_images in (("adaptive", 1, 3), ("adaptive", 32, 96), ("gridtd", 32, 96)):
        case(kind, n_images, max_images, reps)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
