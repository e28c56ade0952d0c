"""CPU: the dataset-split captioners (lrp_imagecaptioning_amd/inference.py, the reference's inference.py:18-264) on a stub
explainer: decoding, de-duplication, metric injection, and which element of a search they take."""
import numpy as np
import pytest

from lrp_imagecaptioning_amd.explainers import CaptionPreprocessorStub
from lrp_imagecaptioning_amd.inference import BasicInference, BeamSearchInference

WORD_OF = {1: "<eos>", 2: "<sos>", 3: "a", 4: "dog", 5: "runs", 6: "fast", 7: "home"}


class _StubExplainer(object):
    """`_beam_search` from a table: per image (by its first pixel) the list of captions a search would return."""

    def __init__(self, table, max_caption_length=4):
        self._preprocessor = CaptionPreprocessorStub(word_of=WORD_OF)
        self._max_caption_length = max_caption_length
        self._table = table
        self.calls = []

    def _beam_search(self, X, beam_size=3, on_device=None):
        imgs = np.asarray(X[1])
        self.calls.append((len(imgs), beam_size, on_device, self._max_caption_length))
        res = [[list(c) for c in self._table[int(img.flat[0])][:beam_size]] for img in imgs]
        return res[0] if len(res) == 1 else res


class _Datum(object):
    def __init__(self, name, refs):
        self.img_filename = name
        self.all_captions_txt = refs


def _X(*ids):
    return (None, np.array(ids, dtype=np.float32).reshape(len(ids), 1, 1, 1) * np.ones((1, 2, 2, 3), dtype=np.float32))


TABLE = {0: [[3, 4, 5, 1], [3, 4, 1]],                 # complete: "a dog runs"
         1: [[3, 4, 5, 6, 1], [3, 4, 5, 7, 1]],        # max_caption_length = 4 words and no EOS: a live caption
         2: [[1], [3, 1]]}                             # EOS at once: the empty caption


def test_greedy_decoding_is_cap_1_to_minus_1():
    ex = _StubExplainer(TABLE)
    inf = BasicInference(ex)
    assert inf._predict_batch(_X(0, 1, 2), None) == ["a dog runs", "a dog runs", ""]      # the live one loses "fast" (I:121)
    assert ex.calls == [(3, 1, False, 4)]                                                # one search of beam 1, host bookkeeping
    assert inf._predict_batch(_X(1)) == ["a dog runs"]                                   # a batch of one


def test_beam_inference_takes_element_zero_and_the_device_search():
    ex = _StubExplainer(TABLE)
    inf = BeamSearchInference(ex, beam_size=2)
    assert inf._predict_batch(_X(0, 1, 2), None) == ["a dog runs <eos>", "a dog runs fast <eos>", "<eos>"]
    assert ex.calls == [(3, 2, True, 4)]
    inf.device_search = False
    inf._predict_batch(_X(0), None)
    assert ex.calls[-1] == (1, 2, False, 4)


def test_shorter_max_caption_length_is_passed_and_restored():
    ex = _StubExplainer(TABLE)
    inf = BeamSearchInference(ex, max_caption_length=3)
    inf._predict_batch(_X(0))
    assert ex.calls == [(1, 3, True, 3)] and ex._max_caption_length == 4
    with pytest.raises(ValueError):
        BeamSearchInference(ex, max_caption_length=5)


def test_predict_pairs_and_deduplication_by_img_filename():
    ex = _StubExplainer(TABLE)
    inf = BeamSearchInference(ex, beam_size=2)
    d = [_Datum("x.jpg", ["a dog runs", "dog"]), _Datum("y.jpg", ["a dog"]), _Datum("x.jpg", ["other"])]
    batches = [(_X(0, 1), None, d[:2]), (_X(2), None, d[2:])]
    pairs = inf.predict(batches)
    assert pairs == [("a dog runs <eos>", d[0]), ("a dog runs fast <eos>", d[1]), ("<eos>", d[2])]
    assert inf.predict(batches, include_datum=False) == [p[0] for p in pairs]
    metrics, pred, refs = inf._evaluate(pairs, include_prediction=True)
    assert metrics == {}                                                                 # no scorer by default
    assert pred == {"x.jpg": [{"caption": "a dog runs <eos>"}], "y.jpg": [{"caption": "a dog runs fast <eos>"}]}
    assert refs == {"x.jpg": [{"caption": "a dog runs"}, {"caption": "dog"}], "y.jpg": [{"caption": "a dog"}]}


def test_metric_injection():
    class Count(object):
        def calculate(self, id_to_prediction, id_to_references):
            return {"images": len(id_to_prediction), "refs": sum(len(r) for r in id_to_references.values())}

    class Words(object):
        def calculate(self, id_to_prediction, id_to_references):
            return {"words": sum(len(p[0]["caption"].split()) for p in id_to_prediction.values())}

    ex = _StubExplainer(TABLE)
    ex._preprocessor.normalize_captions = lambda caps: [c + " <eos>" for c in caps]
    inf = BasicInference(ex, metrics=[Count(), Words()])
    d = [_Datum("x.jpg", ["a dog runs", "dog"]), _Datum("y.jpg", ["a dog"])]
    out = inf.evaluate([(_X(0, 1), None, d)], include_prediction=True)
    assert out[0] == {"images": 2, "refs": 3, "words": 6}
    assert out[2]["x.jpg"][0] == {"caption": "a dog runs <eos>"}                          # the preprocessor's normalisation
    assert inf.evaluate([(_X(0, 1), None, d)]) == out[0]
