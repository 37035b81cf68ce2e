"""The fp64 restatement of the back-off language model (tests/_lm_ref.py) against the worked example of the design,
tests/golden/lm/tiny.arpa with its expected values in tiny.json - derived by hand below, not by running any code.

The model (log10; V = 10 words, <SOS> = 1, <EOS> = 0, eos_mode 'end': the <EOS> becomes </s>):
    unigrams  <unk> -1.5   <s> -99 (backoff -0.30103)   </s> -0.9   4 -0.7 (-0.4)   5 -0.8 (-0.25)   2 -1.0 (-0.5)
    bigrams   <s> 4 -0.3 (-0.2)   4 5 -0.35 (-0.15)   5 2 -0.45   2 </s> -0.05
    trigrams  <s> 4 5 -0.2   5 2 </s> -0.01

"4 5 2":   4 after <s>: bigram "<s> 4" is there                                         -> -0.3
           5 after "<s> 4": trigram "<s> 4 5" is there                                  -> -0.2
           2 after "4 5": no trigram "4 5 2"; context "4 5" is there, backoff -0.15; bigram "5 2" -> -0.45 - 0.15 = -0.6
           </s> after "5 2": trigram "5 2 </s>"                                         -> -0.01
"4 7 2":   7 after "<s> 4": no trigram; context "<s> 4" backoff -0.2; no bigram "4 7"; context "4" backoff -0.4; no
           unigram 7: out of vocabulary.  unk_as_word: <unk> -1.5 + (-0.2 - 0.4) = -2.1; otherwise skipped.
           2 after "4 7": no trigram, no context "4 7", no bigram "7 2", no context "7"; unigram 2 -> -1.0
           </s> after "7 2": no trigram, no context "7 2"; bigram "2 </s>"              -> -0.05
           score -3.45 with n_scored 4, or -1.35 with n_scored 3; n_oov 1 either way.
"2":       2 after <s>: no bigram "<s> 2"; context <s> backoff -0.30103; unigram 2 -> -1.0 - 0.30103 = -1.30103
           </s> after "<s> 2": no trigram, no context "<s> 2"; bigram "2 </s>"          -> -0.05
'word' mode, "4 5 2": the <EOS> id 0 is a word after "5 2": no trigram "5 2 0"; context "5 2" is there without a
           back-off weight (+0.0); no bigram "2 0"; context "2" backoff -0.5; no unigram 0: <unk> -1.5 - 0.5 = -2.0; then
           </s> after "2 0": nothing but the unigram </s> -> -0.9.
The exact bits follow from the float32 roundings: value = f32(logp) + (((0.0 + f32(b1)) + f32(b2)) ...) in float64."""
import json
import os

import numpy as np

import _lm_ref as R
from conftest import GOLDEN_DIR

LM_DIR = os.path.join(GOLDEN_DIR, 'lm')


def load_tiny():
    spec = json.load(open(os.path.join(LM_DIR, 'tiny.json')))
    text = open(os.path.join(LM_DIR, spec['arpa'])).read()
    return spec, text


def expected_values(terms):
    vals = []
    for t in terms:
        if t is None:
            vals.append(0.0)
            continue
        acc = 0.0
        for b in t[1:]:
            acc += R.f32(b)
        vals.append(R.f32(t[0]) + acc)
    return vals


def test_parse_the_worked_example():
    spec, text = load_tiny()
    order, table, dropped = R.parse_arpa(text, spec['vocab_size'])
    V = spec['vocab_size']
    assert order == 3 and len(table) == 12 and dropped == 0
    assert table[(V,)] == (-99.0, R.f32('-0.30103')) and table[(V + 2,)] == (-1.5, 0.0)
    assert table[(5, 2)] == (R.f32('-0.45'), 0.0) and str(table[(5, 2)][1]) == '0.0'      # a missing back-off is +0.0
    assert table[(V, 4, 5)] == (R.f32('-0.2'), 0.0)
    assert R.f32('-0.3') != -0.3                                                            # (rounded once to float32)


def test_restatement_gives_the_hand_derived_values():
    spec, text = load_tiny()
    V = spec['vocab_size']
    order, table, _ = R.parse_arpa(text, V)
    assert len(spec['cases']) == 7
    for c in spec['cases']:
        score, n_scored, n_oov, vals = R.score_row(table, order, c['row'], V, spec['sos'], spec['eos'], c['eos_mode'],
                                                   c['unk_as_word'])
        want = expected_values(c['terms'])
        assert [float(v).hex() for v in vals] == [float(v).hex() for v in want], c
        total = 0.0
        for v in want:
            total += v
        assert float(score).hex() == float(total).hex(), c
        assert (n_scored, n_oov) == (c['n_scored'], c['n_oov']), c
        assert np.allclose(vals, c['approx'], rtol=0, atol=1e-6), c


def test_generator_and_writer_round_trip():
    """Orders 1 to 4, with and without <unk>: the written ARPA text parses back to the generated n-grams; pruned
    contexts occur (an n-gram whose context is no n-gram of the model)."""
    V = 40
    for order in (1, 2, 3, 4):
        for with_unk in (True, False):
            g = R.random_lm(7 + order, V, order, with_unk=with_unk)
            assert sorted(g) == list(range(1, order + 1))
            got_order, table, dropped = R.parse_arpa(R.write_arpa(g), V)
            assert got_order == order and dropped == 0 and len(table) == sum(len(v) for v in g.values())
            assert ((V + 2,) in table) == with_unk and table[(V,)][0] == -99.0
            sp = R.specials(V)
            for k in g:
                for words, logp, backoff in g[k]:
                    ids = tuple(sp[w] if w in sp else int(w) for w in words)
                    assert table[ids] == (R.f32(logp), R.f32(backoff) if backoff is not None else 0.0)
            if order >= 3:
                assert any(ids[:-1] not in table for ids in table if len(ids) == order)
                assert any(ids[:-1] in table for ids in table if len(ids) == order)
    assert R.write_arpa(R.random_lm(5, V, 3)) == R.write_arpa(R.random_lm(5, V, 3))         # seeded
