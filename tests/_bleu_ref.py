"""Plain Python restatement of the BLEU scorer (self_critical/bleu/bleu_scorer.py: cook_refs, cook_test with the
'closest' reference length, and the per-sentence / corpus formulas of compute_score), for the tests: the statistics are
Python ints, the scores Python floats (IEEE fp64) in the scorer's order of operations.  Also the reader of the fixture
tests/golden/bleu.npz and the cooked references as the device scorer takes them (keys of csrc/cider_key.h)."""
import math

import numpy as np

from _cider_dev_ref import normalise, pack_key

SMALL, TINY = 1e-9, 1e-15
SOS, EOS = 1, 2
RTOL = 1e-12      # |a - b| <= RTOL |b|: a dozen correctly rounded operations, one pow, one exp whose argument (at most ~63 in
#                   magnitude) amplifies its rounding by that factor - below ~1e-13 in all, with a margin of 10x


def counts(words, n=4):
    """precook: {n-gram tuple: count} in first-occurrence order (all 1-grams by position, then the 2-grams, ...)."""
    out = {}
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            g = tuple(words[i:i + k])
            out[g] = out.get(g, 0) + 1
    return out


def cook_refs(refs, sos=SOS, eos=EOS):
    """(lengths, {n-gram: max count over the references}) of the normalised references, insertion-ordered."""
    lens, maxc = [], {}
    for ref in refs:
        w = normalise(ref, sos, eos)
        lens.append(len(w))
        for g, c in counts(w).items():
            maxc[g] = max(maxc.get(g, 0), c)
    return lens, maxc


def stats_row(row, cooked, sos=SOS, eos=EOS):
    """[testlen, reflen, guess[0..3], correct[0..3]] of one raw row against cook_refs(...) of its image: ints."""
    lens, maxc = cooked
    w = normalise(row, sos, eos)
    testlen = len(w)
    reflen = min((abs(l - testlen), l) for l in lens)[1]
    guess = [max(0, testlen - k) for k in range(4)]
    correct = [0] * 4
    for g, c in counts(w).items():
        correct[len(g) - 1] += min(maxc.get(g, 0), c)
    return [testlen, reflen] + guess + correct


def scores_of(st):
    """The four per-sentence scores of one row's statistics (bleu_scorer.py:233-242)."""
    testlen, reflen, guess, correct = st[0], st[1], st[2:6], st[6:10]
    out, bleu = [], 1.
    for k in range(4):
        bleu *= (float(correct[k]) + TINY) / (float(guess[k]) + SMALL)
        out.append(bleu ** (1. / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        for k in range(4):
            out[k] *= math.exp(1 - 1 / ratio)
    return out


def corpus_of(stats):
    """The four corpus figures of the summed statistics (bleu_scorer.py:247-259)."""
    tot = [sum(int(s[j]) for s in stats) for j in range(10)]
    testlen, reflen, guess, correct = tot[0], tot[1], tot[2:6], tot[6:10]
    out, bleu = [], 1.
    for k in range(4):
        bleu *= float(correct[k] + TINY) / (guess[k] + SMALL)
        out.append(bleu ** (1. / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        for k in range(4):
            out[k] *= math.exp(1 - 1 / ratio)
    return out


def score_rows(hyps, ref_lists, row_div=1, sos=SOS, eos=EOS):
    """hyps [N, T]; row r against ref_lists[r // row_div] -> (stats int64 [N, 10], scores float64 [N, 4])."""
    cooked = {}
    stats, scores = [], []
    for r, row in enumerate(hyps):
        i = r // row_div
        if i not in cooked:
            cooked[i] = cook_refs(ref_lists[i], sos, eos)
        st = stats_row(row, cooked[i], sos, eos)
        stats.append(st)
        scores.append(scores_of(st))
    return np.asarray(stats, dtype=np.int64), np.asarray(scores, dtype=np.float64)


def cook_device(refs, sos=SOS, eos=EOS):
    """One image's references as the device scorer reads them: (keys [E] python ints, counts [E], ent_off [5], lens [C]),
    the entries grouped by order; within an order references ascending, first occurrence within a reference."""
    lens, maxc = cook_refs(refs, sos, eos)
    keys, cnts, ent_off = [], [], []
    for k in range(1, 5):
        ent_off.append(len(keys))
        for g, c in maxc.items():
            if len(g) == k:
                keys.append(pack_key(g))
                cnts.append(c)
    ent_off.append(len(keys))
    return keys, cnts, ent_off, lens


def rel_err(a, b):
    """max |a - b| / |b| (no score is 0: tiny > 0)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert (b != 0).all()
    return float((np.abs(a - b) / np.abs(b)).max())


def load_set(g, name):
    """A set of the fixture: (hyps int64 [N, T], refs per image [[ids], ...] * I, refs per row, scores [N, 4], corpus [4]);
    row r belongs to image r % I."""
    hyps = g[name + '/hyps'].astype(np.int64)
    tok, cap_off, img_off = g[name + '/ref_tokens'], g[name + '/ref_cap_off'], g[name + '/ref_img_off']
    refs = [[[int(x) for x in tok[cap_off[c]:cap_off[c + 1]]] for c in range(img_off[i], img_off[i + 1])]
            for i in range(len(img_off) - 1)]
    per_row = [refs[r % len(refs)] for r in range(len(hyps))]
    return hyps, refs, per_row, g[name + '/scores'], g[name + '/corpus']
