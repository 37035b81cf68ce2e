"""The Python restatement of the BLEU scorer (tests/_bleu_ref.py) against the fixture the reference's own scorer wrote
(tests/golden/bleu.npz, make_bleu_golden.py).  The GPU tests cannot read the reference; they lean on this restatement.
CPU only."""
import math

import pytest

import _bleu_ref as R


@pytest.mark.parametrize('name', ['small', 'cfg5'])
def test_restatement_matches_the_fixture(golden, name):
    hyps, refs, per_row, scores, corpus = R.load_set(golden('bleu'), name)
    assert hyps.shape == {'small': (36, 12), 'cfg5': (1024, 20)}[name] and scores.shape == (len(hyps), 4)
    stats, got = R.score_rows(hyps, per_row)
    err = R.rel_err(got, scores)
    print('BLEU restatement [%s]: max relative difference to the fixture %.3e' % (name, err))
    assert err <= R.RTOL
    assert R.rel_err(R.corpus_of(stats), corpus) <= R.RTOL
    assert scores[:, 3].min() < 1e-9 and scores[:, 3].max() > 0.9       # from no 4-gram in common to a reference itself


def test_the_statistics_of_the_edge_rows():
    cooked = R.cook_refs([[1, 7, 7, 5, 2], [1, 7, 7, 7, 6, 2], [1, 5, 6, 2]])
    # <EOS> alone: one word, one matching 1-gram
    assert R.stats_row([2, 0, 0, 0], cooked) == [1, 3, 1, 0, 0, 0, 1, 0, 0, 0]
    # five times one word: clipped by the largest count in ONE reference (3), not by the sum over the references (5)
    assert R.stats_row([7, 7, 7, 7, 7, 2], cooked) == [6, 5, 6, 5, 4, 3, 4, 2, 1, 0]
    # a tie of the closest length takes the shorter reference: lengths 4 and 6 against 5 words
    tie = R.cook_refs([[1, 4, 5, 6, 2], [1, 4, 5, 6, 7, 8, 2]])
    assert R.stats_row([4, 5, 6, 7, 2], tie)[:2] == [5, 4]
    # testlen == reflen: the ratio falls just below 1 (small > tiny) and the penalty is applied; one more word: it is not
    at, above = R.stats_row([4, 5, 6, 2], tie), R.stats_row([1, 4, 5, 6, 7, 8, 9, 2], tie)
    assert at[:2] == [4, 4] and above[:2] == [7, 6]
    assert R.scores_of(at)[0] < 1.0 and R.scores_of(at)[0] == (4 + R.TINY) / (4 + R.SMALL) * math.exp(
        1 - 1 / ((4 + R.TINY) / (4 + R.SMALL)))


def test_device_cook_groups_by_order():
    keys, counts, ent_off, lens = R.cook_device([[1, 7, 7, 5, 2], [1, 7, 7, 7, 6, 2]])
    assert lens == [4, 5] and ent_off[0] == 0 and ent_off[4] == len(keys) == len(counts)
    assert keys[:ent_off[1]] == [R.pack_key([w]) for w in (7, 5, 2, 6)] and counts[:ent_off[1]] == [3, 1, 1, 1]
    assert keys[ent_off[1]] == R.pack_key([7, 7]) and counts[ent_off[1]] == 2
