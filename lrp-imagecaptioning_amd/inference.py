"""Captioning a dataset split: the reference's inference.py (`BasicInference` I:18-156, `BeamSearchInference` I:159-264) on an
explainer object, whose engine holds the captioner.

The reference drives a Keras model: every search step re-runs the whole captioner on every partial caption of the batch
(`predict_on_batch`, I:109 / I:202).  Here a batch is ONE call of the explainer's `_beam_search`: the images are encoded once,
every step is one decoder step for all their hypotheses, and with `device_search` the beam bookkeeping stays on the device
as well (lrp_decoder_beam_search), so that a batch costs one copy of the results.

The metric objects (`pycocoevalcap` scorers behind models/metrics.py) need Java and are not part of this package: `_evaluate`
takes any objects with the reference's `calculate(id_to_prediction, id_to_references) -> {name: value}`; the default list is
empty.
"""
import numpy as np


class BasicInference(object):
    """I:18-156, the greedy decoder: per step the most probable next word, until EOS or `max_caption_length` words.

    It runs as the beam-1 search of the explainer: a beam of one keeps the arg-max continuation at every step, and its one
    complete caption is the path up to the first EOS.  The two agree except when a log-probability is exactly 0.0 (a word of
    probability one in float arithmetic): the greedy loop stops at the FIRST EOS, while the search prefers, among complete
    captions of the same total, the longer one.

    Decoding is the reference's own (I:119-124): the words of `cap[1:-1]` for cap = [SOS, w1, ..., EOS].  A caption that never
    reached EOS has no EOS to drop, so it loses its last word — kept as the reference has it."""

    _beam_size = 1
    device_search = False

    def __init__(self, explainer, metrics=(), max_caption_length=None):
        self._explainer = explainer
        self._preprocessor = explainer._preprocessor
        self._metrics = list(metrics)
        self._max_caption_length = explainer._max_caption_length if max_caption_length is None else int(max_caption_length)
        if not 1 <= self._max_caption_length <= explainer._max_caption_length:
            raise ValueError("max_caption_length must be in [1, %d], the explainer's" % explainer._max_caption_length)

    # ------------------------------------------------------------------ prediction
    def _search(self, X):
        """Per image the captions of `_beam_search` (element [0] = the answer), for a batch of any size."""
        ex = self._explainer
        imgs = np.asarray(X[1], dtype=np.float32)
        keep = ex._max_caption_length
        ex._max_caption_length = self._max_caption_length
        try:
            res = ex._beam_search((None, imgs), beam_size=self._beam_size, on_device=self.device_search)
        finally:
            ex._max_caption_length = keep
        return [res] if len(imgs) == 1 else res

    def _words(self, ids):
        word_of = self._preprocessor._word_of
        return " ".join(word_of.get(int(i), "<%d>" % int(i)) if hasattr(word_of, "get") else word_of[int(i)] for i in ids)

    def _predict_batch(self, X, y=None):
        """I:101-126 -> one string per image.  `y` (the expected captions) is unused, as in the reference."""
        sos = self._preprocessor.SOS_TOKEN_LABEL_ENCODED
        out = []
        for caps in self._search(X):
            best = caps[0]                                   # words + [EOS]; max_caption_length words: EOS never came
            cap = [sos] + (best if len(best) <= self._max_caption_length else best[:-1])
            out.append(self._words(cap[1:-1]))               # I:121: range(1, len(cap) - 1)
        return out

    def predict(self, batches, include_datum=True):
        """I:63-92 over an iterable of (X, y, datum_batch): (caption, datum) pairs, or the captions alone."""
        captions, datums = [], []
        for X, y, datum_batch in batches:
            captions += self._predict_batch(X, y)
            datums += list(datum_batch)
        return list(zip(captions, datums)) if include_datum else captions

    # ------------------------------------------------------------------ evaluation
    def _evaluate(self, caption_datum_pairs, include_prediction=False):
        """I:132-156: the first prediction per `img_filename` against all of the image's normalised reference captions."""
        id_to_prediction, id_to_references = {}, {}
        for caption_pred, datum in caption_datum_pairs:
            img_id = datum.img_filename
            if img_id in id_to_prediction:                   # I:139-140: an image is scored once
                continue
            refs = datum.all_captions_txt
            if hasattr(self._preprocessor, "normalize_captions"):
                refs = self._preprocessor.normalize_captions(refs)
            id_to_references[img_id] = [{"caption": c} for c in refs]
            id_to_prediction[img_id] = [{"caption": caption_pred}]
        metrics = {}
        for metric in self._metrics:
            metrics.update(metric.calculate(id_to_prediction, id_to_references))
        return (metrics, id_to_prediction, id_to_references) if include_prediction else metrics

    def evaluate(self, batches, include_prediction=False):
        """`evaluate_*_set` (I:51-61) for a split given as batches."""
        return self._evaluate(self.predict(batches, include_datum=True), include_prediction=include_prediction)


class BeamSearchInference(BasicInference):
    """I:159-264: per image the best complete caption of a beam search, else the best live one — element [0] of the explainer's
    search — decoded word by word WITH its trailing EOS (I:244-253: `sentence_encoded[1:]` through `decode_captions_from_list2d`;
    the references get theirs from `normalize_captions`).  The beam bookkeeping runs on the device by default (`device_search`)."""

    device_search = True

    def __init__(self, explainer, metrics=(), beam_size=3, max_caption_length=None):
        super(BeamSearchInference, self).__init__(explainer, metrics, max_caption_length)
        self._beam_size = int(beam_size)

    def _predict_batch(self, X, y=None):
        best = [caps[0] for caps in self._search(X)]
        if hasattr(self._preprocessor, "decode_captions_from_list2d"):
            return self._preprocessor.decode_captions_from_list2d(best)
        return [self._words(c) for c in best]
