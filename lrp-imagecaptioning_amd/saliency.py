"""Occlusion sensitivity (Zeiler & Fergus, ECCV 2014) and RISE (Petsiuk, Das & Saenko, BMVC 2018) as word saliencies of a
captioning model.  Neither reads a gradient or the model's structure: they are the control the backward-walking explainers are
compared against.

    OcclusionSaliency   slide a window over the image, replace it by `fill`, record how far the word's score falls; a pixel's
                        saliency is the mean fall over the windows that cover it
    RISESaliency        score n_masks randomly masked copies of the image; a pixel's saliency is the mean of the scores weighted
                        by the pixel's mask value, divided by p

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

    # ---------------------------------------------------------------- the driver
    def explain(self, images, captions=None, words=None):
        """images (B, H, W, 3) preprocessed (numpy or device tensor); captions: one id list per image (None: beam search); words:
        per image the positions t >= 1 to explain (None: every word before EOS), as in
        CaptionPerturbationAnalysis.compute_perturbation_analysis.  Returns a dict:
            units    [(image, t)]
            maps     (n_units, H, W) float32 device tensor
            scores0  (n_units,) float64 device tensor: the word's score on the unmasked image
            scores   per image (None without a word) the (1 + rows, n_words) float64 device score matrix the maps were folded
                     from: row 0 the unmasked image, row 1 + k window / mask k"""
        ex = self.explainer
        eng = ex._engine
        dev = eng.device
        x_dev = eng._dev(images)
        if x_dev.dim() != 4:
            raise ValueError("expected (B, H, W, 3) images")
        B, H, W = int(x_dev.shape[0]), int(x_dev.shape[1]), int(x_dev.shape[2])
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
        active = [b for b in range(B) if words_of[b]]
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
            eng.encode_images(rows)
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
        return {"units": units,
                "maps": torch.cat([maps[a, :int(nw[a])] for a in range(len(active))]),
                "scores0": torch.cat([S[a, 0, :int(nw[a])] for a in range(len(active))]),
                "scores": per_image}


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
