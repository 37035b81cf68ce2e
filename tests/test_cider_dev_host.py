"""What the host CIDEr-D library exports for the device scorer (isc_cider_dev_score): the key packing, the
open-addressing document-frequency table and the cooked references - and the numpy restatement of the kernel
(_cider_dev_ref.py), driven by those exports alone, against the golden vectors and the host scorer.  CPU only."""
import math

import numpy as np
import pytest

import _cider_dev_ref as R
from insenticap_model_amd import rewards, synth
from test_cider import CASES, setup

SOS, EOS = 1, 2
_CACHE = {}


def case(name):
    """(scorer, fns, gt, rows [sample; greedy], cooked references per row, table, params), built once per case."""
    if name not in _CACHE:
        split, fns, gt, sample, greedy = setup(name)
        scorer = rewards.get_ciderd_scorer(split, SOS, EOS)
        rows = np.concatenate([sample, greedy])
        cooked = [scorer.cook_refs(gt[f]) for f in fns] * 2
        _CACHE[name] = (scorer, split, fns, gt, rows, cooked, scorer.device_table(), scorer.device_params())
    return _CACHE[name]


def corpus_ngrams(split, n=4):
    """Every distinct n-gram (as an id tuple) of the normalised corpus captions -> the number of images that hold it."""
    df = {}
    for caps_of in split.values():
        for caps in caps_of.values():
            seen = set()
            for cap in caps:
                w = R.normalise(cap, SOS, EOS)
                for k in range(1, n + 1):
                    for i in range(len(w) - k + 1):
                        seen.add(tuple(w[i:i + k]))
            for g in seen:
                df[g] = df.get(g, 0) + 1
    return df


@pytest.mark.parametrize('name', ['small', 'cfg5'])
def test_restatement_matches_the_goldens_and_the_host_scorer(golden, name):
    scorer, split, fns, gt, rows, cooked, table, params = case(name)
    assert rows.shape == {'small': (32, 12), 'cfg5': (512, 20)}[name]
    got = R.score_rows(rows, cooked, table, params, SOS, EOS)
    np.testing.assert_allclose(got, golden('cider')[name + '/scores'], rtol=0, atol=1e-12)
    host = scorer.score_arrays(rows, [gt[f] for f in fns] * 2)
    np.testing.assert_allclose(got, host, rtol=0, atol=1e-12)
    assert host.max() > 1.0


def test_params_are_the_scorers():
    scorer = case('small')[0]
    ref_len, n, sigma = scorer.device_params()
    assert (ref_len, n, sigma) == (math.log(float(CASES['small'][0])), 4, 6.0)


@pytest.mark.parametrize('name', ['small', 'cfg5'])
def test_cooked_references_equal_the_host_scorers_values_in_bits(name):
    """val, norms and length re-derived from the table in the order counts2vec uses: tf (ref_len - d) per distinct n-gram in
    first-occurrence order, norm = sqrt of the sequential sum of x^2, length = the sum of the bigram counts.  sqrt and the
    products are correctly rounded on both sides, so the comparison is in bits."""
    scorer, split, fns, gt, rows, cooked, table, params = case(name)
    ref_len, n, _ = params
    for f, (keys, vals, ord_off, norms, length) in list(zip(fns, cooked))[:24]:
        caps = gt[f]
        assert ord_off.shape == (len(caps), 5) and norms.shape == (len(caps), 4) and length.shape == (len(caps),)
        assert ord_off[0, 0] == 0 and ord_off[-1, 4] == len(keys) == len(vals)
        assert (ord_off[1:, 0] == ord_off[:-1, 4]).all() and (np.diff(ord_off, axis=1) >= 0).all()
        for c, cap in enumerate(caps):
            w = R.normalise(cap, SOS, EOS)
            for o in range(4):
                k = o + 1
                grams = [tuple(w[i:i + k]) for i in range(len(w) - k + 1)]
                distinct = list(dict.fromkeys(grams))                 # first-occurrence order
                a, b = int(ord_off[c, o]), int(ord_off[c, o + 1])
                assert [R.unpack_key(x) for x in keys[a:b]] == [list(g) for g in distinct]
                acc, tfs = 0.0, 0.0
                for g, v in zip(distinct, vals[a:b]):
                    tf = float(grams.count(g))
                    x = tf * (ref_len - R.probe(table, R.pack_key(g))[0])
                    assert x == v and math.copysign(1.0, x) == math.copysign(1.0, v)
                    acc += x * x
                    tfs += tf
                assert math.sqrt(acc) == norms[c, o]
                if o == 1:
                    assert tfs == length[c] == float(max(len(w) - 1, 0))


def test_cooked_references_reproduce_the_host_score_of_a_reference_against_itself():
    """A row that equals a reference of its image scores what the host scorer gives it (the cooked vals / norms / length
    are then both sides of the dot product)."""
    scorer, split, fns, gt, rows, cooked, table, params = case('small')
    T = 24
    hyp = np.zeros((4, T), dtype=np.int64)
    for i in range(4):
        cap = gt[fns[i]][i % len(gt[fns[i]])]
        hyp[i, :len(cap)] = cap                                   # <SOS> ... <EOS>, then <PAD>
    got = R.score_rows(hyp, cooked[:4], table, params, SOS, EOS)
    host = scorer.score_arrays(hyp, [gt[f] for f in fns[:4]])
    np.testing.assert_allclose(got, host, rtol=0, atol=1e-12)
    assert (host > 1.0).all()


@pytest.mark.parametrize('name', ['small', 'cfg5'])
def test_table_holds_every_corpus_ngram_and_nothing_else(name):
    scorer, split, fns, gt, rows, cooked, table, params = case(name)
    df = corpus_ngrams(split)
    assert scorer.num_ngrams == len(df)
    cap = len(table)
    assert cap & (cap - 1) == 0 and cap >= 2 * len(df) and (cap == 16 or cap < 4 * len(df))
    assert table.dtype.itemsize == 16 and int((table['key'] != 0).sum()) == len(df)
    items = list(df.items()) if name == 'small' else list(df.items())[::37]
    for g, count in items:
        log_df, slot, probes = R.probe(table, R.pack_key(g))
        assert slot >= 0 and log_df == math.log(max(1.0, float(count))), g
    V = CASES[name][1]
    for g in ([V + 5], [V + 5, V + 6], [4, V + 5, 5], [V + 1, V + 2, V + 3, V + 4]):      # ids no caption holds
        assert R.probe(table, R.pack_key(g))[1] == -1


def test_probing_is_exercised_in_the_small_case():
    """At least one entry of the `small` table (V = 60) sits away from its home slot; a tighter table - the capacity factor of
    the test, not of production - displaces many more and still finds everything."""
    scorer, split = case('small')[:2]
    table = case('small')[6]
    mask = len(table) - 1
    used = np.nonzero(table['key'])[0]
    away = [s for s in used if (R.hash_key(int(table['key'][s])) & mask) != s]
    assert len(away) >= 1
    tight_cap = 1
    while tight_cap <= scorer.num_ngrams:
        tight_cap <<= 1
    tight = scorer.device_table(capacity=tight_cap)
    assert len(tight) == tight_cap < len(table)
    worst = 0
    for key, log_df in zip(table['key'][used], table['log_df'][used]):
        got, slot, probes = R.probe(tight, int(key))
        assert slot >= 0 and got == log_df
        worst = max(worst, probes)
    assert worst > 2
    # a full table (no empty slot) must end a lookup of an absent key: the probe loop is bounded by the capacity
    full = tight.copy()
    full['key'][full['key'] == 0] = R.pack_key([59, 59, 59, 59])
    assert R.probe(full, R.pack_key([58, 58, 58, 58])) == (0.0, -1, tight_cap)
    with pytest.raises(RuntimeError):
        scorer.device_table(capacity=tight_cap // 2)                # not above the number of n-grams
    with pytest.raises(RuntimeError):
        scorer.device_table(capacity=tight_cap * 3)                 # no power of two


def test_key_packing():
    assert R.pack_key([0]) == 1 and R.unpack_key(R.pack_key([0])) == [0]
    k = R.pack_key([7, 65534, 9])
    assert R.unpack_key(k) == [7, 65534, 9]
    assert (k >> 16) & 0xFFFF == 0xFFFF and k & 0xFFFF == 8 and (k >> 32) & 0xFFFF == 10 and k >> 48 == 0
    assert R.unpack_key(R.pack_key([65534, 65534, 65534, 65534])) == [65534] * 4
    # orders cannot collide: the same leading ids give different keys, and id 0 (<PAD>) is not "no field"
    ks = [R.pack_key([5, 0, 0, 0][:k]) for k in range(1, 5)]
    assert len(set(ks)) == 4 and 0 not in ks
    # the library packs the same way: a scorer over a vocabulary that reaches 65534
    caps = [[[SOS, 65534, 7, 65534, EOS], [SOS, 7, 8, EOS]], [[SOS, 9, 65534, EOS]]]
    scorer = rewards.CiderD(caps, SOS, EOS)
    keys, vals, ord_off, norms, length = scorer.cook_refs(caps[0])
    w = [65534, 7, 65534, EOS]
    assert [R.unpack_key(x) for x in keys[ord_off[0, 1]:ord_off[0, 2]]] == [w[0:2], w[1:3], w[2:4]]
    assert [R.unpack_key(x) for x in keys[ord_off[0, 0]:ord_off[0, 1]]] == [[65534], [7], [EOS]]
    table = scorer.device_table()
    assert R.probe(table, R.pack_key([65534]))[0] == math.log(2.0)
    assert R.probe(table, R.pack_key([65533]))[1] == -1            # the neighbour id is another key


def test_ids_beyond_the_key_fields_are_refused():
    scorer = rewards.CiderD([[[SOS, 65535, 4, EOS]], [[SOS, 5, EOS]]], SOS, EOS)
    with pytest.raises(ValueError):
        scorer.device_table()
    with pytest.raises(ValueError):
        scorer.cook_refs([[SOS, 5, 65535, EOS]])
    ok = case('small')[0]
    with pytest.raises(ValueError):
        ok.to_device('cpu', 65536)
    with pytest.raises(ValueError):
        rewards.DeviceCiderD(ok, 'cpu', 65536)


def test_existing_scores_are_unchanged_by_the_exports():
    """The exports are read-only: scoring before and after them gives the same bits."""
    scorer, split, fns, gt, rows, cooked, table, params = case('small')
    refs = [gt[f] for f in fns] * 2
    a = scorer.score_arrays(rows, refs)
    scorer.device_table(), scorer.cook_refs(gt[fns[0]]), scorer.device_params()
    assert (scorer.score_arrays(rows, refs) == a).all()
