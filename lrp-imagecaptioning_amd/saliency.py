"""Occlusion sensitivity (Zeiler & Fergus, ECCV 2014) and RISE (Petsiuk, Das & Saenko, BMVC 2018) as word saliencies of a
captioning model.  Neither reads a gradient or the model's structure: they are the control the backward-walking explainers are
compared against.

    OcclusionSaliency   slide a window over the image, replace it by `fill`, record how far the word's score falls; a pixel's
                        saliency is the mean fall over the windows that cover it
    RISESaliency        score n_masks randomly masked copies of the image; a pixel's saliency is the mean of the scores weighted
                        by the pixel's mask value, divided by p
    LIMESaliency        (Ribeiro, Singh & Guestrin, KDD 2016) switch the segments of the image on and off at random; a pixel's
                        saliency is its segment's coefficient in a kernel-weighted ridge regression of the score on the switches
    KernelSHAPSaliency  (Lundberg & Lee, NeurIPS 2017) the same regression under the Shapley kernel and the efficiency constraint:
                        the segments' Shapley values, sampled or (up to 12 segments) exact
    GradientCAMSaliency (Grad-CAM, Grad-CAM++, XGrad-CAM, LayerCAM, HiResCAM) a map over the positions of the encoder output from the
                        gradient of the word's logit there, expanded to the image; no masked forward
    ScoreCAMSaliency    (Wang et al., CVPR-W 2020) mask the image by each feature channel's own upsampled map; a channel's weight
                        in the CAM is the word's score under its mask
    AblationCAMSaliency (Desai & Ramaswamy, WACV 2020) zero one channel of the encoder output at a time; a channel's weight is the
                        relative fall of the word's score (decoder forwards only)

A masked image is one image slot of the engine: per chunk of max_images slots (any mix of images and masks) the apply operator
makes the rows (lrp_op_occlude / lrp_op_rise_apply), `encode_images` and one teacher-forced `decoder_forward` with each slot's
own caption score every word of every slot at once, `lrp_perturb_word_scores` reads the scores in place and they are scattered
into the images' score matrices on the device.  After the last chunk one map kernel per group of images (lrp_op_occlusion_map /
lrp_op_rise_map) folds the matrices into the maps.  No masked image, score matrix or map crosses PCIe.

The RISE masks are a function of (seed, key, k) alone (include/lrp_hip.h): `keys` names the images (default: their position in
the call), so an image keeps its masks wherever it stands in a batch.  The mask is the bilinear upsample of an (s + 1)^2 grid by
exactly (ceil(H / s), ceil(W / s)) pixels per cell, cropped at a random shift; RISE itself resizes an s x s grid by a non-integer
factor, and the two agree in distribution away from the border.

Afterwards the engine's cached forward belongs to the last chunk of masked images: the explainer's cached caption is dropped."""
import numpy as np
import torch

from . import engine as _eng

SCORES = ("prob", "logp", "logit")
_TILE = 8          # RISE_TT of csrc/saliency_kernels.h, the words per thread of the RISE map kernel: T is padded to a multiple
                   # with zero columns, which cost no pass there (another value stays correct; only the padding loses its point)


def _check_common(fill, score):
    if score not in SCORES:
        raise ValueError("score must be 'prob', 'logp' or 'logit'")
    f = np.asarray(fill, dtype=np.float64).reshape(-1)
    if f.size not in (1, 3) or not np.isfinite(f).all():      # (three: every image of the engine has three channels)
        raise ValueError("fill must be a finite scalar or one value per channel")


class _WordSaliency(object):
    def __init__(self, explainer, fill, score):
        self.explainer = explainer
        self.fill = fill
        self.score = score

    # ---------------------------------------------------------------- what a method adds
    def _rows(self):
        """masked rows per image, the unmasked row 0 not counted"""
        raise NotImplementedError()

    def _prepare(self, x_dev, image_ids):
        pass

    def _apply(self, x_dev, img, k, grid_row, plain):
        """img, k (n) int32 device tensors -> (n, H, W, C) rows: masked where k >= 0, the image itself at the slots listed in
        `plain` (host ints: the slots with k = -1)"""
        raise NotImplementedError()

    def _maps(self, S, H, W):
        """S (n_img, 1 + rows, T) float64 -> (n_img, T, H, W) float32"""
        raise NotImplementedError()

    def _set_segments(self, x_dev, segments):
        """the caller's label map, before anything runs (the segment methods alone take one)"""
        if segments is not None:
            raise ValueError("%s takes no segments" % type(self).__name__)

    def _extras(self, active, n_words, B):
        """what a method adds to the result dict, after _maps"""
        return {}

    def _check_images(self, x_dev):
        """what a method demands of the (B, H, W, 3) images, before anything runs"""
        pass

    def _enter(self, eng, rows):
        """how a chunk's rows enter the engine: masked images through the encoder (the CAM family's ablated feature rows
        replace its output instead)"""
        eng.encode_images(rows)

    # ---------------------------------------------------------------- the driver
    def _units(self, images, captions, words, segments):
        """the arguments of `explain`, checked -> (x_dev, B, H, W, captions, units, words_of, active)"""
        ex = self.explainer
        eng = ex._engine
        x_dev = eng._dev(images)
        if x_dev.dim() != 4:
            raise ValueError("expected (B, H, W, 3) images")
        B, H, W = int(x_dev.shape[0]), int(x_dev.shape[1]), int(x_dev.shape[2])
        self._check_images(x_dev)
        self._set_segments(x_dev, segments)
        if captions is None:
            res = ex._beam_search((None, x_dev.cpu().numpy()))
            captions = [res[0]] if B == 1 else [r[0] for r in res]
        captions = [list(map(int, c)) for c in captions]
        if len(captions) != B or (words is not None and len(words) != B):
            raise ValueError("one caption (and one list of word positions) per image")
        units, words_of = [], []
        for b in range(B):
            ts = [int(t) for t in (range(1, len(captions[b])) if words is None else words[b])]
            for t in ts:
                if t < 1 or t > len(captions[b]):
                    raise NotImplementedError("index out of range of captions")          # E:538-539
                units.append((b, t))
            words_of.append(ts)
        if not units:
            raise ValueError("no word to explain")
        return x_dev, B, H, W, captions, units, words_of, [b for b in range(B) if words_of[b]]

    def explain(self, images, captions=None, words=None, segments=None):
        """images (B, H, W, 3) preprocessed (numpy or device tensor); captions: one id list per image (None: beam search); words:
        per image the positions t >= 1 to explain (None: every word before EOS), as in
        CaptionPerturbationAnalysis.compute_perturbation_analysis.  Returns a dict:
            units    [(image, t)]
            maps     (n_units, H, W) float32 device tensor
            scores0  (n_units,) float64 device tensor: the word's score on the unmasked image
            scores   per image (None without a word) the (1 + rows, n_words) float64 device score matrix the maps were folded
                     from: row 0 the unmasked image, row 1 + k window / mask k
        segments (LIME and KernelSHAP alone): a (B, H, W) int label map from any segmenter, every label of [0, d) in every image
        (None: the regular grid of `cells`); their result also holds
            coefficients  per image the (n_words, d) float64 device tensor of the fit
            intercept     per image (n_words,): LIME's intercept, KernelSHAP's base score (every segment filled)
            segments      the (B, H, W) int32 label map used
            status        (B,) int32, 0: the fit went through (anything else raises ValueError)"""
        ex = self.explainer
        eng = ex._engine
        dev = eng.device
        x_dev, B, H, W, captions, units, words_of, active = self._units(images, captions, words, segments)
        self._prepare(x_dev, active)
        R = 1 + self._rows()                                   # row 0: the unmasked image (k = -1)
        Tp = -(-max(len(words_of[b]) for b in active) // _TILE) * _TILE
        S = torch.zeros((len(active), R, Tp), dtype=torch.float64, device=dev)

        # every job (image, row) and every unit (job, word) of the run, built once and uploaded once
        nw = np.array([len(words_of[b]) for b in active], dtype=np.int64)
        job_ai = np.repeat(np.arange(len(active), dtype=np.int64), R)
        job_row = np.tile(np.arange(R, dtype=np.int64), len(active))
        job_nw = nw[job_ai]
        ustart = np.concatenate([[0], np.cumsum(job_nw)])
        unit_job = np.repeat(np.arange(len(job_ai), dtype=np.int64), job_nw)
        unit_w = np.arange(ustart[-1], dtype=np.int64) - ustart[unit_job]
        t_flat = np.concatenate([np.asarray(words_of[b], dtype=np.int64) for b in active])
        col_flat = np.concatenate([np.asarray([captions[b][t - 1] - 1 for t in words_of[b]], dtype=np.int64) for b in active])
        woff = np.concatenate([[0], np.cumsum(nw)])
        src = woff[job_ai[unit_job]] + unit_w                  # the unit's word in the flat per-image word lists
        up = lambda a, dt=torch.int32: torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
        active_np = np.asarray(active, dtype=np.int64)
        job_img_d, job_k_d = up(active_np[job_ai]), up(job_row - 1)
        job_grid_d = up(job_ai * (R - 1) + np.maximum(job_row - 1, 0), torch.int64)
        unit_job_d, unit_t_d, unit_col_d = up(unit_job), up(t_flat[src]), up(col_flat[src])
        dest_d = up((job_ai[unit_job] * R + job_row[unit_job]) * Tp + unit_w, torch.int64)
        flat = S.view(-1)

        M = eng.max_images
        for c0 in range(0, len(job_ai), M):
            c1 = min(len(job_ai), c0 + M)
            rows = self._apply(x_dev, job_img_d[c0:c1], job_k_d[c0:c1], job_grid_d[c0:c1],
                               [j - c0 for j in range(c0, c1) if job_row[j] == 0])
            self._enter(eng, rows)
            eng.decoder_forward([captions[active[a]] for a in job_ai[c0:c1]])
            u0, u1 = int(ustart[c0]), int(ustart[c1])
            logit, logp = _eng.perturb_word_scores(eng, unit_job_d[u0:u1] - c0, unit_t_d[u0:u1], unit_col_d[u0:u1])
            flat.index_copy_(0, dest_d[u0:u1], logit if self.score == "logit" else (logp if self.score == "logp" else logp.exp()))
        ex.caption = None                                      # the engine's caches now hold the last chunk
        ex._state_cache = {}

        maps = self._maps(S, H, W)
        per_image = [None] * B
        for a, b in enumerate(active):
            per_image[b] = S[a, :, :int(nw[a])]
        res = {"units": units,
               "maps": torch.cat([maps[a, :int(nw[a])] for a in range(len(active))]),
               "scores0": torch.cat([S[a, 0, :int(nw[a])] for a in range(len(active))]),
               "scores": per_image}
        res.update(self._extras(active, nw, B))
        return res


class OcclusionSaliency(_WordSaliency):
    """window (ph, pw) or an int; stride likewise (None: the window); fill: a scalar or one value per channel (preprocessed
    units: 0 is the dataset mean); score 'prob' (exp(logp)), 'logp' or 'logit'."""

    @staticmethod
    def check_arguments(window=None, stride=None, fill=0.0, score="prob"):
        if window is None:
            raise ValueError("occlusion needs a window")
        ph, pw = _eng._pair(window, "window")
        sh, sw = (ph, pw) if stride is None else _eng._pair(stride, "stride")
        if not (1 <= sh <= ph and 1 <= sw <= pw):
            raise ValueError("occlusion needs 1 <= stride <= window on both axes: window (%d, %d), stride (%d, %d)" % (ph, pw, sh, sw))
        _check_common(fill, score)
        return (ph, pw), (sh, sw)

    def __init__(self, explainer, window, stride=None, fill=0.0, score="prob"):
        self.window, self.stride = self.check_arguments(window, stride, fill, score)
        super(OcclusionSaliency, self).__init__(explainer, fill, score)
        H, W = explainer._model.img_hw
        self._grid = _eng.occlusion_geometry(H, W, self.window, self.stride)

    def _rows(self):
        return self._grid[0] * self._grid[1]

    def _apply(self, x_dev, img, k, grid_row, plain):
        return _eng.op_occlude(x_dev, img, k, self.window, self.stride, self.fill)      # (k = -1 copies the image)

    def _maps(self, S, H, W):
        return _eng.op_occlusion_map(S, H, W, self.window, self.stride)


class RISESaliency(_WordSaliency):
    """n_masks masks per image from an (s + 1)^2 grid of cells that are 1 with probability p; seed: the 64-bit Philox key;
    keys: one uint32 identity per image of a call (default: its position), so an image's masks do not depend on its batch."""

    @staticmethod
    def check_arguments(n_masks=None, s=8, p=0.5, seed=0, fill=0.0, score="prob", keys=None):
        if n_masks is None or int(n_masks) != n_masks or n_masks < 1:
            raise ValueError("n_masks must be a positive int")
        if int(s) != s or not 1 <= s <= _eng.RISE_MAX_S:
            raise NotImplementedError("RISE grid s=%s outside [1,%d]" % (s, _eng.RISE_MAX_S))
        if not 0.0 < float(p) <= 1.0:
            raise ValueError("RISE needs 0 < p <= 1")
        if int(seed) != seed or not 0 <= seed < 2 ** 64:
            raise ValueError("seed must be an int in [0, 2^64)")
        if keys is not None and any(int(k) != k or not 0 <= k < 2 ** 32 for k in keys):
            raise ValueError("keys must be ints in [0, 2^32)")
        _check_common(fill, score)

    def __init__(self, explainer, n_masks, s=8, p=0.5, seed=0, fill=0.0, score="prob", keys=None):
        self.check_arguments(n_masks, s, p, seed, fill, score, keys)
        super(RISESaliency, self).__init__(explainer, fill, score)
        self.n_masks, self.s, self.p, self.seed = int(n_masks), int(s), float(p), int(seed)
        self.keys = None if keys is None else [int(k) for k in keys]

    def _rows(self):
        return self.n_masks

    def _prepare(self, x_dev, image_ids):
        if self.keys is not None and len(self.keys) != x_dev.shape[0]:
            raise ValueError("one key per image")
        keys = np.asarray([b if self.keys is None else self.keys[b] for b in image_ids], dtype=np.int64)
        K = self.n_masks
        H, W = int(x_dev.shape[1]), int(x_dev.shape[2])
        self.grids, self.shifts = _eng.op_rise_grids(np.repeat(keys, K), np.tile(np.arange(K, dtype=np.int64), len(keys)), self.s,
                                                     self.p, self.seed, H, W, device=x_dev.device)

    def _apply(self, x_dev, img, k, grid_row, plain):
        rows = _eng.op_rise_apply(x_dev, img, self.grids[grid_row], self.shifts[grid_row], self.s, self.fill)
        if plain:                                              # the operator has no unmasked row: one per image is copied in
            sel = torch.as_tensor(plain, device=x_dev.device)
            rows[sel] = x_dev[img[sel].long()]
        return rows

    def _maps(self, S, H, W):
        n_img, K = S.shape[0], self.n_masks
        return _eng.op_rise_map(S[:, 1:], self.grids.view(n_img, K, -1), self.shifts.view(n_img, K, 2), H, W, self.s, self.p)


# ---------------------------------------------------------------------------------------------------------------
# LIME and KernelSHAP: the mask is a binary choice over d segments, the scores are folded by a weighted linear regression
# (csrc/segment_kernels.h).  The same driver: only the hooks differ.
# ---------------------------------------------------------------------------------------------------------------
shapley_size_thresholds = _eng.shapley_size_thresholds
SHAP_ENUM_MAX_D = 12


def grid_segments(H, W, cells):
    """(H, W) int32 labels of a regular grid of `cells` (an int or (cells_y, cells_x)): cell boundaries at floor(i H / cells_y)
    and floor(j W / cells_x), label = i cells_x + j."""
    cy, cx = _eng._pair(cells, "cells")
    if cy < 1 or cx < 1:
        raise ValueError("cells must be positive")
    row = np.searchsorted(np.arange(cy + 1, dtype=np.int64) * H // cy, np.arange(H), side="right") - 1
    col = np.searchsorted(np.arange(cx + 1, dtype=np.int64) * W // cx, np.arange(W), side="right") - 1
    return (row[:, None] * cx + col[None, :]).astype(np.int32)


def _full_bits(d):
    """the four words of the subset that holds every one of d segments, as int32"""
    words = [(1 << min(max(d - 32 * w, 0), 32)) - 1 for w in range(4)]
    return np.array(words, dtype=np.uint32).view(np.int32)


def lime_weights(d, kernel_width):
    """wtab[m], m = 0 .. d: LIME's exponential kernel sqrt(exp(-D^2 / kernel_width^2)) on the cosine distance D = 1 - sqrt(m / d)
    of a subset of m segments to the all-ones vector (the empty subset has distance 1)."""
    m = np.arange(d + 1, dtype=np.float64)
    return np.sqrt(np.exp(-(1.0 - np.sqrt(m / d)) ** 2 / float(kernel_width) ** 2))


def shapley_weights(d):
    """wtab[m] = (d - 1) / (C(d, m) m (d - m)) on 1 <= m <= d - 1, 0 at the ends: the Shapley kernel of Lundberg & Lee, theorem 2"""
    from math import comb
    w = np.zeros(d + 1, dtype=np.float64)
    for m in range(1, d):
        w[m] = (d - 1.0) / (float(comb(d, m)) * m * (d - m))
    return w


def _check_segment_common(cells, ridge, seed, keys, fill, score):
    cy, cx = _eng._pair(cells, "cells")
    if cy < 1 or cx < 1:
        raise ValueError("cells must be positive")
    _eng._seg_count(cy * cx)                                   # NotImplementedError outside [2, SEG_MAX_D]
    if not (np.isfinite(ridge) and float(ridge) >= 0.0):
        raise ValueError("ridge must be finite and >= 0")
    if int(seed) != seed or not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be an int in [0, 2^64)")
    if keys is not None and any(int(k) != k or not 0 <= k < 2 ** 32 for k in keys):
        raise ValueError("keys must be ints in [0, 2^32)")
    _check_common(fill, score)
    return cy * cx


class _SegmentSaliency(_WordSaliency):
    """what LIME and KernelSHAP share: the label map, its check, the keys of the draws and the extra keys of the result"""

    def __init__(self, explainer, cells, ridge, seed, fill, score, keys):
        super(_SegmentSaliency, self).__init__(explainer, fill, score)
        self.cells, self.ridge, self.seed = _eng._pair(cells, "cells"), float(ridge), int(seed)
        self.keys = None if keys is None else [int(k) for k in keys]

    def _check_d(self, d):
        _eng._seg_count(d)

    def _set_segments(self, x_dev, segments):
        B, H, W = int(x_dev.shape[0]), int(x_dev.shape[1]), int(x_dev.shape[2])
        dev = x_dev.device
        if segments is None:
            lab = torch.as_tensor(grid_segments(H, W, self.cells)).to(dev).unsqueeze(0).expand(B, H, W).contiguous()
            d = self.cells[0] * self.cells[1]
        else:
            lab = segments if torch.is_tensor(segments) else torch.as_tensor(np.asarray(segments))
            if tuple(lab.shape) != (B, H, W) or lab.dtype.is_floating_point or lab.dtype == torch.bool:
                raise ValueError("segments must be a (B, H, W) = (%d, %d, %d) int label map" % (B, H, W))
            lab = lab.to(dev)
            lo, hi = int(lab.min()), int(lab.max())
            if lo < 0:
                raise ValueError("segment labels must be >= 0")
            d = hi + 1                                         # one d per call
            lab = lab.to(torch.int32).contiguous()
        self._check_d(d)
        # every label must occur in every image: an image's regression then has the same d columns whatever its batch mates are
        present = torch.zeros((B, d), dtype=torch.bool, device=dev).scatter_(1, lab.view(B, -1).long(), True)
        missing = (~present).nonzero()
        if missing.numel():
            b, l = (int(v) for v in missing[0])
            raise ValueError("image %d has no pixel of segment %d: every label in [0, %d) must occur in every image" % (b, l, d))
        self.labels, self.d = lab, d

    def _draw_keys(self, x_dev, image_ids):
        if self.keys is not None and len(self.keys) != x_dev.shape[0]:
            raise ValueError("one key per image")
        return np.asarray([b if self.keys is None else self.keys[b] for b in image_ids], dtype=np.int64)

    def _fold(self, phi, icpt, status, active):
        """keep the fit for _extras, refuse a singular one, gather the maps"""
        bad = status.nonzero()
        if bad.numel():
            raise ValueError("image %d: the regression's normal equations are singular; use more samples or a ridge"
                             % active[int(bad[0])])
        self._fit = (phi, icpt, status)
        return _eng.op_segment_map(phi, self.labels[torch.as_tensor(active, device=phi.device)], self.d)

    def _extras(self, active, n_words, B):
        phi, icpt, status = self._fit
        coef, inter = [None] * B, [None] * B
        st = torch.zeros((B,), dtype=torch.int32, device=phi.device)
        st[torch.as_tensor(active, device=phi.device)] = status
        for a, b in enumerate(active):
            coef[b], inter[b] = phi[a, :int(n_words[a])], icpt[a, :int(n_words[a])]
        return {"coefficients": coef, "intercept": inter, "segments": self.labels, "status": st}


class LIMESaliency(_SegmentSaliency):
    """LIME (Ribeiro, Singh & Guestrin 2016) on image segments: row 0 is the image itself and joins the fit as the all-ones sample
    (as LIME's first sample does), rows 1 .. n_samples switch each segment on with probability p (off: `fill`).  A weighted ridge
    regression of the word's score on the binary vectors, free intercept, the row weight LIME's exponential kernel of width
    kernel_width on the cosine distance to the all-ones vector; a pixel's saliency is its segment's coefficient.  cells: the
    regular grid used when `explain` gets no label map.  LIME's feature selection is not built: every segment enters the fit."""

    @staticmethod
    def check_arguments(n_samples=None, cells=7, p=0.5, kernel_width=0.25, ridge=1.0, seed=0, fill=0.0, score="prob", keys=None):
        if n_samples is None or int(n_samples) != n_samples or n_samples < 1:
            raise ValueError("n_samples must be a positive int")
        if not 0.0 < float(p) <= 1.0:
            raise ValueError("LIME needs 0 < p <= 1")
        if not (np.isfinite(kernel_width) and float(kernel_width) > 0.0):
            raise ValueError("kernel_width must be finite and > 0")
        return _check_segment_common(cells, ridge, seed, keys, fill, score)

    def __init__(self, explainer, n_samples, cells=7, p=0.5, kernel_width=0.25, ridge=1.0, seed=0, fill=0.0, score="prob", keys=None):
        self.check_arguments(n_samples, cells, p, kernel_width, ridge, seed, fill, score, keys)
        super(LIMESaliency, self).__init__(explainer, cells, ridge, seed, fill, score, keys)
        self.n_samples, self.p, self.kernel_width = int(n_samples), float(p), float(kernel_width)

    def _rows(self):
        return self.n_samples

    def _prepare(self, x_dev, image_ids):
        keys, K = self._draw_keys(x_dev, image_ids), self.n_samples
        self._active = list(image_ids)
        self.bits = _eng.op_segment_draws(np.repeat(keys, K), np.tile(np.arange(K, dtype=np.int64), len(keys)), self.d, "bernoulli",
                                          self.p, self.seed, device=x_dev.device)
        self._full = torch.as_tensor(_full_bits(self.d)).to(x_dev.device)

    def _apply(self, x_dev, img, k, grid_row, plain):
        bits = self.bits[grid_row]
        if plain:                                              # every segment on: the operator returns the image's bits
            bits[torch.as_tensor(plain, device=x_dev.device)] = self._full
        return _eng.op_segment_apply(x_dev, img, bits, self.labels, self.d, self.fill)

    def _maps(self, S, H, W):
        n_img = S.shape[0]
        bits = torch.cat([self._full.view(1, 1, 4).expand(n_img, 1, 4), self.bits.view(n_img, self.n_samples, 4)], dim=1)
        phi, icpt, status = _eng.op_segment_fit(bits, lime_weights(self.d, self.kernel_width), S, self.d, self.ridge)
        return self._fold(phi, icpt, status, self._active)


class KernelSHAPSaliency(_SegmentSaliency):
    """KernelSHAP (Lundberg & Lee 2017) on image segments: row 0 is the image (`total`), row 1 the image with every segment
    filled (`base`); the regression explains score - base under the constraint sum(phi) = total - base, which is eliminated as
    the shap package does.  n_samples an even int >= 2 d: antithetic pairs of subsets drawn from the Shapley kernel's size
    distribution, unit weights.  n_samples None: every one of the 2^d - 2 proper subsets in ascending integer order under the
    Shapley kernel's weights, which gives the exact Shapley values of the d segments (d <= 12).  `intercept` is the base score."""

    @staticmethod
    def _check_samples(n_samples, d):
        if n_samples is None:
            if d > SHAP_ENUM_MAX_D:
                raise NotImplementedError("enumerating the subsets of d=%d segments: n_samples=None is for d <= %d" % (d, SHAP_ENUM_MAX_D))
        elif int(n_samples) != n_samples or n_samples % 2 or n_samples < 2 * d:
            raise ValueError("n_samples must be an even int >= 2 d = %d (antithetic pairs; fewer leave the fit singular)" % (2 * d))

    @staticmethod
    def check_arguments(n_samples=None, cells=4, ridge=0.0, seed=0, fill=0.0, score="prob", keys=None):
        d = _check_segment_common(cells, ridge, seed, keys, fill, score)
        KernelSHAPSaliency._check_samples(n_samples, d)
        return d

    def __init__(self, explainer, n_samples=None, cells=4, ridge=0.0, seed=0, fill=0.0, score="prob", keys=None):
        self.check_arguments(n_samples, cells, ridge, seed, fill, score, keys)
        super(KernelSHAPSaliency, self).__init__(explainer, cells, ridge, seed, fill, score, keys)
        self.n_samples = None if n_samples is None else int(n_samples)

    def _check_d(self, d):                                     # (again with the d of the caller's label map)
        _eng._seg_count(d)
        self._check_samples(self.n_samples, d)

    def _n(self):
        return 2 ** self.d - 2 if self.n_samples is None else self.n_samples

    def _rows(self):
        return 1 + self._n()

    def _prepare(self, x_dev, image_ids):
        dev, K, n_img = x_dev.device, self._n(), len(image_ids)
        self._active = list(image_ids)
        if self.n_samples is None:
            draws = torch.zeros((K, 4), dtype=torch.int32, device=dev)
            draws[:, 0] = torch.arange(1, K + 1, dtype=torch.int32, device=dev)
            draws = draws.unsqueeze(0).expand(n_img, K, 4)
        else:
            keys = self._draw_keys(x_dev, image_ids)
            draws = _eng.op_segment_draws(np.repeat(keys, K), np.tile(np.arange(K, dtype=np.int64), n_img), self.d, "shapley",
                                          seed=self.seed, device=dev).view(n_img, K, 4)
        # per image: the empty subset (the base row), then the samples
        self.bits = torch.cat([torch.zeros((n_img, 1, 4), dtype=torch.int32, device=dev), draws], dim=1).contiguous()
        self._full = torch.as_tensor(_full_bits(self.d)).to(dev)

    def _apply(self, x_dev, img, k, grid_row, plain):
        bits = self.bits.view(-1, 4)[grid_row]
        if plain:
            bits[torch.as_tensor(plain, device=x_dev.device)] = self._full
        return _eng.op_segment_apply(x_dev, img, bits, self.labels, self.d, self.fill)

    def _maps(self, S, H, W):
        base = S[:, 1]
        delta = (S[:, 0] - base).contiguous()
        y = (S[:, 2:] - base[:, None]).contiguous()
        if self.n_samples is None:
            wtab = shapley_weights(self.d)
        else:
            wtab = np.ones(self.d + 1, dtype=np.float64)
            wtab[0] = wtab[self.d] = 0.0
        phi, _, status = _eng.op_segment_fit(self.bits[:, 1:].contiguous(), wtab, y, self.d, self.ridge, delta)
        return self._fold(phi, base.contiguous(), status, self._active)


# ---------------------------------------------------------------------------------------------------------------
# The CAM family (csrc/cam_kernels.h): a map over the L = g * g positions of the encoder output, expanded to the image as
# Guided Grad-CAM's factor is.  The gradient forms read lrp_decoder_gradient and run no masked forward; Score-CAM and
# Ablation-CAM take their channel weights from forwards and run on the driver above.
# ---------------------------------------------------------------------------------------------------------------
CAM_METHODS = tuple(sorted(_eng.CAM_MODES, key=_eng.CAM_MODES.get))
SCORECAM_WEIGHTS = ("softmax", "linear")


def _cam_model(explainer):
    """(g, upscale) of the explainer's model; ValueError / NotImplementedError where the CAM kernels do not reach"""
    eng = explainer._engine
    _eng._cam_channels(eng.D)
    return _eng.cam_geometry(eng.L, eng.img_hw[0], eng.img_hw[1])


class GradientCAMSaliency(_WordSaliency):
    """method: 'gradcam' (Selvaraju et al. 2017), 'gradcam++' (Chattopadhay et al. 2018), 'xgradcam' (Fu et al. 2020),
    'layercam' (Jiang et al. 2021) or 'hirescam' (Draelos & Carin 2020), on the gradient of the word's logit at the encoder
    output.  No masked forward: per chunk of min(max_images, max_tokens) units encode_images, one teacher-forced
    decoder_forward, decoder_gradient and lrp_op_cam.  guided: the cam also gates the guided-backprop map of the unit (Guided
    Grad-CAM for every form): the result gains "guided", (n_units, H, W, 3) float64.  "maps" is the cam in float32, "scores0"
    the word's logit, "scores" per image its (1, n_words) row.  Limited as the gradient baselines are: the engine is switched
    to the exact fp32 forward, and an adaptive decoder needs embedding_dim == hidden_dim."""

    @staticmethod
    def check_arguments(method="gradcam", guided=False):
        if method not in CAM_METHODS:
            raise ValueError("unknown CAM method %r: one of %s" % (method, list(CAM_METHODS)))
        if guided not in (False, True):
            raise ValueError("guided must be a bool")

    def __init__(self, explainer, method="gradcam", guided=False):
        self.check_arguments(method, guided)
        super(GradientCAMSaliency, self).__init__(explainer, 0.0, "logit")
        self.method, self.guided = method, bool(guided)
        self._g, self._up = _cam_model(explainer)
        eng = explainer._engine
        if eng.decoder == "adaptive" and eng.E != eng.H:
            raise NotImplementedError("the decoder gradient of the adaptive model needs embedding_dim == hidden_dim")
        eng.set_precision("fp32")                              # (as _GradientMixin: the forward whose ReLU decisions are exact fp32)

    def _check_images(self, x_dev):
        _eng.cam_geometry(self.explainer._engine.L, int(x_dev.shape[1]), int(x_dev.shape[2]))

    def explain(self, images, captions=None, words=None, segments=None):
        ex = self.explainer
        eng = ex._engine
        dev = eng.device
        x_dev, B, H, W, captions, units, words_of, active = self._units(images, captions, words, segments)
        chunk = min(eng.max_images, eng.max_tokens)
        cams, gated, s0 = [], [], []
        for c0 in range(0, len(units), chunk):
            part = units[c0:c0 + chunk]
            imgs = sorted(set(b for b, _ in part))             # at most `chunk` images: the units are in image order
            slot = dict((b, i) for i, b in enumerate(imgs))
            eng.encode_images(x_dev[torch.as_tensor(imgs, device=dev)])
            eng.decoder_forward([captions[b] for b in imgs])
            ii, tt = [slot[b] for b, _ in part], [t for _, t in part]
            d, _ = eng.decoder_gradient(ii, tt, want_r_words=False)
            gb = eng.cnn_walk(ii, d, "guided_backprop") if self.guided else None
            r = _eng.op_cam(eng.get_features(), ii, d, self._g, self._up, self.method, gb=gb)
            if self.guided:
                gated.append(r[0])
                r = r[1]
            cams.append(r)
            s0.append(_eng.perturb_word_scores(eng, ii, tt, [captions[b][t - 1] - 1 for b, t in part])[0])
        ex.caption = None                                      # the engine's caches now hold the last chunk
        ex._state_cache = {}
        s0 = torch.cat(s0)
        per_image, u0 = [None] * B, 0
        for b in active:
            per_image[b] = s0[u0:u0 + len(words_of[b])].view(1, -1)
            u0 += len(words_of[b])
        res = {"units": units, "maps": torch.cat(cams).to(torch.float32), "scores0": s0, "scores": per_image}
        if self.guided:
            res["guided"] = torch.cat(gated)
        return res


class _ForwardCAMSaliency(_WordSaliency):
    """what Score-CAM and Ablation-CAM share: the images' features kept on the device, one row per feature channel, the fold"""
    _weights = None

    def __init__(self, explainer, fill, score):
        super(_ForwardCAMSaliency, self).__init__(explainer, fill, score)
        self._g, self._up = _cam_model(explainer)

    def _check_images(self, x_dev):
        _eng.cam_geometry(self.explainer._engine.L, int(x_dev.shape[1]), int(x_dev.shape[2]))

    def _rows(self):
        return self.explainer._engine.D

    def _prepare(self, x_dev, image_ids):
        eng = self.explainer._engine
        ids = torch.as_tensor(list(image_ids), device=x_dev.device)
        self._active = ids.to(torch.int32)
        self.feat = torch.zeros((x_dev.shape[0], eng.L, eng.D), dtype=torch.float32, device=x_dev.device)
        for c0 in range(0, len(image_ids), eng.max_images):
            eng.encode_images(x_dev[ids[c0:c0 + eng.max_images]])
            self.feat[ids[c0:c0 + eng.max_images]] = eng.get_features()

    def _maps(self, S, H, W):
        return _eng.op_cam_weighted(S, self.feat, self._active, self._g, self._up, self._weights)


class ScoreCAMSaliency(_ForwardCAMSaliency):
    """Score-CAM (Wang et al. 2020): row k of an image is the image under the min-max normalised, bilinearly upsampled map of
    feature channel k (`fill` where the map is 0), D rows per image; a channel's weight is the softmax over the channels of the
    word's score under its mask ('softmax', the paper's form) or the score's rise over the all-fill image, one more row
    ('linear', the paper's "increase of confidence" without the softmax).  The coarse map is sum_c F[l][c] w_c."""

    @staticmethod
    def check_arguments(weights="softmax", fill=0.0, score="logit"):
        if weights not in SCORECAM_WEIGHTS:
            raise ValueError("weights must be 'softmax' or 'linear'")
        _check_common(fill, score)

    def __init__(self, explainer, weights="softmax", fill=0.0, score="logit"):
        self.check_arguments(weights, fill, score)
        super(ScoreCAMSaliency, self).__init__(explainer, fill, score)
        self.weights = self._weights = weights

    def _rows(self):
        return self.explainer._engine.D + (self.weights == "linear")

    def _apply(self, x_dev, img, k, grid_row, plain):
        return _eng.op_scorecam_apply(x_dev, self.feat, img, k, self._g, self._up, self.fill)   # (k = -1 copies, k = D: the fill image)


class AblationCAMSaliency(_ForwardCAMSaliency):
    """Ablation-CAM (Desai & Ramaswamy 2020): row k of an image is its encoder output with channel k set to 0, which enters the
    engine through set_features: decoder forwards only.  A channel's weight is the relative fall of the word's score,
    (s_0 - s_k) / |s_0|."""
    _weights = "ablation"

    @staticmethod
    def check_arguments(score="logit"):
        _check_common(0.0, score)

    def __init__(self, explainer, score="logit"):
        self.check_arguments(score)
        super(AblationCAMSaliency, self).__init__(explainer, 0.0, score)

    def _apply(self, x_dev, img, k, grid_row, plain):
        return _eng.op_feature_ablate(self.feat, img, k)       # (k = -1 copies the features)

    def _enter(self, eng, rows):
        eng.set_features(rows)
