"""CPU: the tie-heavy draws of tests/beam_cases.py, which test_gpu_beam_device.py runs the device bookkeeping on, really go
through the corners of the reference's order (log_prob, sentence) — conditions on the test data, not measurements.  The draws
depend on the helper's integer hash, so the seeds fixed in TIE_CASES are checked here."""
import glob
import os

import numpy as np

import beam_cases as B
from conftest import GOLDEN
from lrp_imagecaptioning_amd import beam
from lrp_imagecaptioning_amd.synthetic import canned_score_table


def _run(case, **kw):
    k, V, T, seed = case
    return B.search_full(B.tie_step(seed, B.TIE_IMAGES, k, V), B.TIE_IMAGES, k, T, B.EOS, **kw)


def test_instrumented_copy_is_beam_search():
    for case in B.TIE_CASES:
        k, V, T, seed = case
        for steps in (1, T):
            ref = beam.search(B.tie_step(seed, B.TIE_IMAGES, k, V), B.TIE_IMAGES, k, steps, B.EOS)
            got = B.search_full(B.tie_step(seed, B.TIE_IMAGES, k, V), B.TIE_IMAGES, k, steps, B.EOS)
            assert [g[0] for g in got] == ref
            for caps, lens, logp, n_complete in got:
                assert len(caps) == k and lens == [len(c) for c in caps] and 0 <= n_complete <= k
                assert all(isinstance(x, float) for x in logp)
    for path in sorted(glob.glob(os.path.join(GOLDEN, "beam_s*.npz"))):
        z = np.load(path)
        V, n_img, k, max_len, eos = int(z["V"]), int(z["n_images"]), int(z["beam"]), int(z["max_len"]), int(z["eos"])
        table = canned_score_table(int(z["seed"]), V, n_img)
        ref = beam.search(B.canned_step(table, n_img, k, V), n_img, k, max_len, eos)
        got = B.search_full(B.canned_step(table, n_img, k, V), n_img, k, max_len, eos)
        assert [g[0] for g in got] == ref
        assert [g[0][0] for g in got] == [[int(w) for w in z["caption_%d" % i]] for i in range(n_img)]


def _state_bytes(n_images, k, max_len):
    from lrp_imagecaptioning_amd import _capi
    return _capi.load().lrp_op_beam_state_bytes(n_images, k, max_len)          # a host function: no GPU needed


def test_state_size_query():
    """Every case is one the operators accept; the size grows with each argument and bad arguments are refused."""
    for k, V, T, _ in B.TIE_CASES:
        n = _state_bytes(B.TIE_IMAGES, k, T)
        # two buffers per image, each with 2k sentences of T words and 2k float64 totals at the least
        assert n % 8 == 0 and n >= B.TIE_IMAGES * 2 * (2 * k * T * 4 + 2 * k * 8)
        assert _state_bytes(B.TIE_IMAGES + 1, k, T) > n and _state_bytes(B.TIE_IMAGES, k, T + 1) > n
    assert _state_bytes(1, 32, 20) > _state_bytes(1, 31, 20)
    for bad in ((0, 3, 5), (1, 0, 5), (1, 33, 5), (1, 3, 0)):
        assert _state_bytes(*bad) < 0


def test_tie_heavy_draws_cover_the_corners_of_the_order():
    live_tie = complete_tie = fed_eos = over_k = differs = 0
    for case in B.TIE_CASES:
        k = case[0]
        assert _state_bytes(B.TIE_IMAGES, k, case[2]) > 0       # a case the device operators take
        st = {}
        full = _run(case, stats=st)
        plain = _run(case, by_logp_only=True)
        live_tie += st["live_tie_by_sentence"]          # a live-candidate tie the sentence decides
        complete_tie += st["complete_tie_of_lengths"]   # two complete captions of different lengths on one total
        fed_eos += st["fed_eos"]                        # a live row continues a hypothesis that ended in EOS
        over_k += sum(n > k for n in st["recorded"])    # an image records more complete captions than it keeps
        differs += sum(a[0] != b[0] for a, b in zip(full, plain))
    assert live_tie > 0
    assert complete_tie > 0
    assert over_k > 0
    assert fed_eos > 0
    assert differs > 0


def test_each_multi_beam_case_depends_on_the_sentence_key():
    """Every case with k > 1 returns something else under a log-prob-only order: none of them passes by accident."""
    for case in B.TIE_CASES:
        if case[0] > 1:
            full, plain = _run(case), _run(case, by_logp_only=True)
            assert any(a[0] != b[0] for a, b in zip(full, plain)), case


def test_totals_are_exact_multiples_of_a_half():
    for case in B.TIE_CASES:
        for _, _, logp, _ in _run(case):
            assert all(float(2 * x).is_integer() for x in logp)
