"""Perturbation ("pixel-flipping") analysis (the reference's innvestigate/tools/perturbate.py, cited PT:): rank the regions
of an image by the relevance a heat-map gives them, replace the top-k regions, run the model again and record how far the
score of the explained word falls.  The faster the curve falls, the more faithful the explanation.

    Perturbation                 PT:25-191   regions of a batch of images replaced by the ranks of a batch of analyses
    CaptionPerturbationAnalysis  PT:194-397  the curve for every (image, word) unit of a set of captioned images

Everything between the heat-maps and the scores stays on the device (lrp_perturb_ranks, lrp_perturb_apply,
lrp_perturb_word_scores; csrc/perturb_kernels.h): no heat-map and no perturbed image crosses PCIe.

Kept from the reference, bug for bug: with the default channels='first' only channel 0 of the image is perturbed (the
mask has a channel axis of length 1 and PT:135-139 index x with that channel; B after the BGR preprocessing).
channels='all' perturbs every channel.

Differences from the reference:
  * exact ties between region scores go to the lower region index (PT:82 sorts with quicksort and leaves them open);
    scores are accumulated in float64 in a fixed order;
  * the reference clips the whole batch inside its loop as soon as one region is perturbed (PT:142-146), so what it
    perturbs afterwards is the clipped tensor, except for the very first perturbed region of the batch, which depends on
    what else the batch holds.  Here every unit stands alone: with a value range a unit with at least one perturbed region
    is clipped, perturbed and clipped again; a unit without one is not clipped;
  * a region shape that divides exactly one axis raises ValueError (the reference pads that axis by a whole region and
    dies on its own assert, PT:107);
  * 'gaussian' draws N(0, 0.3) from a torch.Generator instead of numpy's global state;
  * `recompute_analysis` (PT:215) is not offered: the reference cannot run it either — with recompute_analysis=True
    `analysis_generator` is never set (PT:227-239) and compute_perturbation_analysis fails at PT:384.
"""
import numpy as np
import torch

from . import engine as _eng

_FUNCTIONS = {"zeros": "zeros", "gaussian": "noise", "mean": "mean", "invert": "invert"}


def _reduction(f, what):
    if isinstance(f, str):
        if f not in ("mean", "max"):
            raise ValueError("%s '%s' not known." % (what, f))
        return f
    if f is np.mean:
        return "mean"
    if f is np.max or f is getattr(np, "amax", None):
        return "max"
    raise NotImplementedError("%s must be 'mean', 'max', np.mean or np.max" % what)


def random_ranks(n, nreg, seed):
    """(n, nreg) int32: one permutation per unit from np.random.RandomState(seed), the baseline order."""
    rs = np.random.RandomState(seed)
    return np.stack([rs.permutation(nreg) for _ in range(n)]).astype(np.int32).reshape(n, nreg)


class Perturbation(object):
    """PT:25-191 on the device.  perturbation_function 'zeros' | 'mean' | 'invert' | 'gaussian' (or np.zeros_like / np.mean);
    reduce_function / aggregation_function 'mean' | 'max' (or np.mean / np.max); generator: the torch.Generator of
    'gaussian' (default: torch's global one for the device)."""

    def __init__(self, perturbation_function, num_perturbed_regions=0, region_shape=(9, 9), reduce_function="mean",
                 aggregation_function="mean", pad_mode="reflect", in_place=False, value_range=None, channels="first",
                 generator=None):
        if isinstance(perturbation_function, str):
            if perturbation_function not in _FUNCTIONS:
                raise ValueError("Perturbation function type '{}' not known.".format(perturbation_function))    # PT:57
            self.perturbation_function = perturbation_function
        elif perturbation_function is np.zeros_like:
            self.perturbation_function = "zeros"
        elif perturbation_function is np.mean:
            self.perturbation_function = "mean"
        elif callable(perturbation_function):
            raise NotImplementedError("a perturbation function runs on the device: 'zeros', 'mean', 'invert' or 'gaussian'")
        else:
            raise TypeError("Cannot handle perturbation function of type {}.".format(type(perturbation_function)))  # PT:61
        self.reduce_function = _reduction(reduce_function, "reduce_function")
        self.aggregation_function = _reduction(aggregation_function, "aggregation_function")
        if pad_mode != "reflect":
            raise NotImplementedError("pad_mode 'reflect' is the one the device kernels index")
        if channels not in ("first", "all"):
            raise ValueError("channels must be 'first' (the reference: channel 0 only) or 'all'")
        if len(region_shape) != 2 or int(region_shape[0]) < 1 or int(region_shape[1]) < 1:
            raise ValueError("region_shape must be two positive ints")
        if value_range is not None and not (len(value_range) == 2 and value_range[0] <= value_range[1]):
            raise ValueError("value_range must be (min_val, max_val)")
        self.num_perturbed_regions = num_perturbed_regions
        self.region_shape = (int(region_shape[0]), int(region_shape[1]))
        self.pad_mode = pad_mode
        self.in_place = in_place
        self.value_range = value_range
        self.channels = channels
        self.generator = generator

    # ---------------------------------------------------------------- device steps (tensors in, tensors out)
    def ranks_device(self, analysis, negate=False):
        """analysis (n, H, W, C) float32 / float64 device tensor -> (n, nreg) int32 ranks."""
        return _eng.perturb_ranks(analysis, self.region_shape, self.reduce_function, self.aggregation_function, negate=negate)

    def apply_device(self, x, img_idx, ranks, k):
        """x (B, H, W, C) float32 device tensor, unit u = image img_idx[u] with the regions of rank <= k[u] - 1 replaced."""
        mode = _FUNCTIONS[self.perturbation_function]
        noise = None
        if mode == "noise":
            shape = (ranks.shape[0],) + tuple(x.shape[1:])
            gdev = self.generator.device if self.generator is not None else x.device
            noise = torch.empty(shape, dtype=torch.float32, device=gdev).normal_(0.0, 0.3, generator=self.generator).to(x.device)
        return _eng.perturb_apply(x, img_idx, ranks, k, self.region_shape, mode=mode, noise=noise,
                                  all_channels=self.channels == "all", value_range=self.value_range)

    # ---------------------------------------------------------------- the reference's surface
    @staticmethod
    def _to_device(a, keep64=False):
        """numpy array or GPU tensor -> float32 GPU tensor (float64 stays float64 with keep64; other dtypes are converted)."""
        if not torch.is_tensor(a):
            a = torch.as_tensor(np.ascontiguousarray(a)).to("cuda")
        elif not a.is_cuda:
            raise ValueError("tensors must live on the GPU (numpy arrays are copied there)")
        if a.dtype == torch.float32 or (keep64 and a.dtype == torch.float64):
            return a
        return a.to(torch.float64 if keep64 else torch.float32)

    def _check(self, shape):
        if len(shape) != 4:
            raise ValueError("expected (n, H, W, C) arrays")
        return _eng.perturb_geometry(shape[1], shape[2], self.region_shape)

    def region_ranks(self, analysis):
        """PT:167-177 for a batch of analyses (n, H, W, C): (n, nreg) int32 ranks in row-major region order, 0 = the highest
        score; a numpy array for a numpy array, a device tensor for a device tensor."""
        self._check(tuple(analysis.shape))
        r = self.ranks_device(self._to_device(analysis, keep64=True))
        return r if torch.is_tensor(analysis) else r.cpu().numpy()

    def perturbate_on_batch(self, x, analysis):
        """PT:150-191: x, analysis (n, H, W, C) channels-last, numpy arrays or device tensors -> the perturbed batch, of the
        kind x was (float32).  The num_perturbed_regions highest ranking regions of each sample are replaced."""
        if tuple(analysis.shape) != tuple(x.shape):
            raise ValueError("analysis %s and x %s differ in shape" % (tuple(analysis.shape), tuple(x.shape)))      # PT:164
        self._check(tuple(x.shape))
        xd = self._to_device(x)
        ranks = self.ranks_device(self._to_device(analysis, keep64=True).to(xd.device))
        n = xd.shape[0]
        out = self.apply_device(xd, torch.arange(n, dtype=torch.int32, device=xd.device), ranks,
                                float(self.num_perturbed_regions))
        if torch.is_tensor(x):
            if self.in_place:
                x.copy_(out)
            return out
        out = out.cpu().numpy()
        if self.in_place:
            x[...] = out
        return out


class CaptionPerturbationAnalysis(object):
    """PT:194-397 for a captioning model: the perturbation curve of every (image, word) unit.

    explainer: any of the explainer classes (LRP, gradient, gradient x input, Guided Grad-CAM, occlusion, RISE; either decoder); its
    heat-map of a word ranks the regions.  order 'relevance' (most relevant first), 'least_relevant' (the scores negated)
    or 'random' (a host-drawn permutation per unit from `seed`: the baseline the curve is read against; nothing is
    explained).  Step 0 is the unperturbed image; step s perturbs 1 + (s - 1) * regions_per_step regions (PT:377-385;
    regions_per_step may be a float), always starting from the original image.

    No `recompute_analysis`: the reference cannot run it (see the module docstring).  Afterwards the engine's cached
    forward belongs to the last chunk of perturbed images, not to any image of the caller's."""

    def __init__(self, explainer, perturbation, steps=1, regions_per_step=1, order="relevance", seed=0):
        if order not in ("relevance", "least_relevant", "random"):
            raise ValueError("order must be 'relevance', 'least_relevant' or 'random'")
        if int(steps) != steps or steps < 0:
            raise ValueError("steps must be a non-negative int")
        self.explainer = explainer
        self.perturbation = perturbation
        self.steps = int(steps)
        self.regions_per_step = regions_per_step
        self.order = order
        self.seed = seed

    def _heatmaps(self, ii, ts, images=None, captions=None):
        """(n, H, W, 3) heat-maps of the units (slot, t) of the engine's current forward, on the device.  images, captions: what
        that forward was made from (read by the occlusion / RISE explainers only, which run forwards of their own)."""
        from .explainers import _GradientMixin, _GuidedGradcamMixin, _SaliencyMixin
        ex = self.explainer
        eng = ex._engine
        if isinstance(ex, _SaliencyMixin):
            # occlusion / RISE need the chunk's images and captions, not the cached forward (which their own chunks replace:
            # step 0 has been read by now, and the next chunk encodes again)
            words = [[t for i, t in zip(ii, ts) if i == b] for b in range(len(captions))]
            res = ex.explain_images(images, captions, words)
            row = {u: j for j, u in enumerate(res["units"])}
            sel = torch.as_tensor([row[(i, t)] for i, t in zip(ii, ts)], device=eng.device)
            return res["maps"][sel].unsqueeze(-1).expand(-1, -1, -1, 3).contiguous()
        if isinstance(ex, _GuidedGradcamMixin):
            return eng.guided_gradcam(ii, ts)
        if isinstance(ex, _GradientMixin):
            d, _ = eng.decoder_gradient(ii, ts, want_r_words=False)
            return eng.cnn_walk(ii, d, ex._walk)
        return eng.explain_tokens(ii, ts)[0]

    def compute_perturbation_analysis(self, images, captions=None, words=None):
        """images (B, H, W, 3) preprocessed; captions: one id list per image (None: beam search); words: per image the
        positions t >= 1 to explain (None: every word before EOS).  Returns a dict:
            units   [(image, t)]
            logp    (steps + 1, n_units) float64: log-probability of the unit's word at every step (row 0: unperturbed)
            logit   (steps + 1, n_units) float64: its logit
            scores  the reference's list of steps + 1 means (PT:374-397): here the mean word probability per step
            aopc    (n_units,) the mean over the steps of p_0 - p_s (zeros without a step)
        The units are explained in chunks of max_images images / max_tokens words and ranked once; every perturbed unit is
        one image slot of a chunk of max_images, teacher-forced with its own caption.  Only the (steps + 1, n_units)
        scalars come back to the host."""
        images = np.asarray(images, dtype=np.float32)
        ex, pert = self.explainer, self.perturbation
        eng = ex._engine
        B = len(images)
        Hr, Wr, _, _ = _eng.perturb_geometry(images.shape[1], images.shape[2], pert.region_shape)
        if captions is None:
            res = ex._beam_search((None, images))
            captions = [res[0]] if B == 1 else [r[0] for r in res]
        captions = [list(map(int, c)) for c in captions]
        if len(captions) != B or (words is not None and len(words) != B):
            raise ValueError("one caption (and one list of word positions) per image")
        units = []
        for b in range(B):
            for t in (range(1, len(captions[b])) if words is None else words[b]):
                if t < 1 or t > len(captions[b]):
                    raise NotImplementedError("index out of range of captions")          # E:538-539
                units.append((b, int(t)))
        n = len(units)
        if n == 0:
            raise ValueError("no word to explain")
        dev = eng.device
        x_dev = torch.as_tensor(images).to(dev)
        i32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32)).to(dev)
        img_of = i32([b for b, _ in units])
        t_of = i32([t for _, t in units])
        col_of = i32([captions[b][t - 1] - 1 for b, t in units])
        logit = torch.empty((self.steps + 1, n), dtype=torch.float64, device=dev)
        logp = torch.empty((self.steps + 1, n), dtype=torch.float64, device=dev)

        # step 0 and the ranks: the unperturbed forward of max_images images at a time
        ranks = torch.empty((n, Hr * Wr), dtype=torch.int32, device=dev)
        if self.order == "random":
            ranks.copy_(torch.as_tensor(random_ranks(n, Hr * Wr, self.seed)))
        u0 = 0
        for lo in range(0, B, eng.max_images):
            hi = min(B, lo + eng.max_images)
            mine = [(b - lo, t) for b, t in units if lo <= b < hi]
            if not mine:
                continue
            u1 = u0 + len(mine)
            eng.encode_images(x_dev[lo:hi])
            eng.decoder_forward(captions[lo:hi])
            logit[0, u0:u1], logp[0, u0:u1] = _eng.perturb_word_scores(eng, img_of[u0:u1] - lo, t_of[u0:u1], col_of[u0:u1])
            if self.order != "random":
                for c0 in range(0, len(mine), eng.max_tokens):
                    chunk = mine[c0:c0 + eng.max_tokens]
                    R = self._heatmaps([u[0] for u in chunk], [u[1] for u in chunk], x_dev[lo:hi], captions[lo:hi])
                    ranks[u0 + c0:u0 + c0 + len(chunk)] = pert.ranks_device(R, negate=self.order == "least_relevant")
            u0 = u1

        # steps 1 ..: one perturbed image per slot
        for s in range(1, self.steps + 1):
            k = 1 + (s - 1) * self.regions_per_step
            for c0 in range(0, n, eng.max_images):
                c1 = min(n, c0 + eng.max_images)
                eng.encode_images(pert.apply_device(x_dev, img_of[c0:c1], ranks[c0:c1], float(k)))
                eng.decoder_forward([captions[b] for b, _ in units[c0:c1]])
                slots = torch.arange(c1 - c0, dtype=torch.int32, device=dev)
                logit[s, c0:c1], logp[s, c0:c1] = _eng.perturb_word_scores(eng, slots, t_of[c0:c1], col_of[c0:c1])
        ex.caption = None                                    # the engine's caches now hold the last chunk
        ex._state_cache = {}
        logp_h, logit_h = logp.cpu().numpy(), logit.cpu().numpy()
        p = np.exp(logp_h)
        aopc = (p[:1] - p[1:]).mean(axis=0) if self.steps else np.zeros(n)
        return {"units": units, "logp": logp_h, "logit": logit_h, "scores": [float(v) for v in p.mean(axis=1)], "aopc": aopc}
