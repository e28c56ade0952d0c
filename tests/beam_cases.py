"""Shared by the beam-bookkeeping tests (test_beam_cases.py on the CPU, test_gpu_beam_device.py on the device): canned `step`
callables for `beam.search`, and an instrumented copy of its bookkeeping that also returns what the device kernels return
(lengths, float64 log-probabilities, the number of complete captions) and says which corners of the order a run went through.

Two kinds of scores:
  * the goldens' canned step (the `_canned_step` of tests/test_beam.py restated): the seeded score table the reference's own
    `_beam_search` ran on for tests/golden/beam_s*.npz;
  * a tie-heavy step: every log-probability is a multiple of -0.5, so exact float64 ties of the totals are frequent and the
    second key of the reference's order — the sentence, `Caption` tuple comparison (inference.py:297-315) — decides.
"""
import numpy as np

from lrp_imagecaptioning_amd import beam
from lrp_imagecaptioning_amd.synthetic import canned_next_word_scores

EOS = 1

# (k, V, max_len, seed) of the tie-heavy cases, 3 images each.  The seeds are fixed so that the draws go through every
# corner test_beam_cases.py lists (they depend on `_mix` below, so they are checked there, not assumed).
TIE_IMAGES = 3
TIE_CASES = [(3, 6, 7, 0), (4, 9, 8, 0), (1, 5, 6, 0), (32, 40, 4, 0)]


def canned_step(table, n_images, k, V):
    """`step` of beam.search on the goldens' canned scores: tracks every row's word history like the device rows do."""
    hist = {}

    def step(s, parent, word):
        nonlocal hist
        if s == 0:
            hist = {r: [] for r in range(n_images * k)}
        else:
            hist = {r: hist[int(parent[r])] + [int(word[r])] for r in range(n_images * k)}
        sc = np.stack([canned_next_word_scores(table, r // k, hist[r]) for r in range(n_images * k)])
        return beam.topk_log_softmax(sc, k)
    return step


def _mix(seed, image, history):
    """An explicit 32-bit integer hash of (seed, image, word history): the same draws in every process."""
    h = (seed * 0x9E3779B1 + image * 0x85EBCA77 + 0x165667B1) & 0xFFFFFFFF
    for w in history:
        h = ((h ^ int(w)) * 0x01000193 + 0x7F4A7C15) & 0xFFFFFFFF
        h ^= h >> 15
    return h


def tie_step(seed, n_images, k, V):
    """Tie-heavy `step`: per (seed, image, word history) k distinct columns out of V and logp = -0.5 * sort(randint(1, 4, k))."""
    hist = {}

    def step(s, parent, word):
        nonlocal hist
        if s == 0:
            hist = {r: [] for r in range(n_images * k)}
        else:
            hist = {r: hist[int(parent[r])] + [int(word[r])] for r in range(n_images * k)}
        ids = np.empty((n_images * k, k), dtype=np.int32)
        logp = np.empty((n_images * k, k), dtype=np.float64)
        for r in range(n_images * k):
            rs = np.random.RandomState(_mix(seed, r // k, hist[r]))
            ids[r] = rs.permutation(V)[:k]
            logp[r] = -0.5 * np.sort(rs.randint(1, 4, k))
        return ids, logp
    return step


def search_full(step, n_images, k, steps, eos, by_logp_only=False, stats=None):
    """The bookkeeping of `beam.search`, line for line, returning per image (captions, lengths, logp, n_complete): captions
    as `beam.search` returns them (tested equal in test_beam_cases.py), lengths with the EOS, the float64 totals, and how many of the
    captions are complete ones.  by_logp_only=True orders by the log-probability alone (a stable sort: what an implementation
    that forgets the sentence key would do).  stats: a dict that collects the corners the run went through."""
    if by_logp_only:
        order = lambda c: c[1]
    else:
        order = lambda c: (c[1], c[0])
    st = stats if stats is not None else {}
    for name in ("live_tie_by_sentence", "complete_tie_of_lengths", "fed_eos"):
        st.setdefault(name, 0)
    st.setdefault("recorded", [0] * n_images)
    beams = [[((), 0.0)] for _ in range(n_images)]
    rows = [[0] for _ in range(n_images)]
    complete = [[] for _ in range(n_images)]
    for s in range(steps):
        if s == 0:
            ids, logp = step(0, None, None)
        else:
            parent, word = [], []
            for i in range(n_images):
                pad = k - len(beams[i])
                parent += [i * k + r for r in rows[i]] + [i * k + rows[i][0]] * pad
                word += [b[0][-1] for b in beams[i]] + [beams[i][0][0][-1]] * pad
            st["fed_eos"] += sum(int(w) == eos for w in word)
            ids, logp = step(s, parent, word)
        ids, logp = np.asarray(ids), np.asarray(logp, dtype=np.float64)
        for i in range(n_images):
            cand = []
            for r, (words, lp) in enumerate(beams[i]):
                for c, l in zip(ids[i * k + r], logp[i * k + r]):
                    w = int(c) + 1
                    total = lp + float(l)
                    cand.append((words + (w,), total, r))
                    if w == eos:
                        complete[i].append((words, total))
                        st["recorded"][i] += 1
            plain = sorted(cand, key=lambda c: c[1], reverse=True)[:k]
            cand.sort(key=order, reverse=True)
            st["live_tie_by_sentence"] += [c[0] for c in plain] != [c[0] for c in cand[:k]]
            complete[i].sort(key=order, reverse=True)
            top = complete[i][:k + 1]
            st["complete_tie_of_lengths"] += any(a[1] == b[1] and len(a[0]) != len(b[0]) for a, b in zip(top, top[1:]))
            del complete[i][k:]
            keep = cand[:k]
            beams[i] = [(c[0], c[1]) for c in keep]
            rows[i] = [c[2] for c in keep]
    out = []
    for i in range(n_images):
        both = complete[i][:k]
        n_complete = len(both)
        both = both + beams[i][:k - n_complete]
        out.append(([list(c[0]) + [eos] for c in both], [len(c[0]) + 1 for c in both], [c[1] for c in both], n_complete))
    return out
