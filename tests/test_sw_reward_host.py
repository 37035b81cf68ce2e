"""The sentiment-word reward on the host (no GPU): rewards.get_senti_words_reward and the restatement of tests/_sw_ref.py
against the fixture recorded from the reference's own function (tests/golden/make_sw_golden.py), the table's dict round
trip, the host statement of the decay against a Python loop, the checkpoint key, the refusals a Detector reaches without
a device, and the condition the GPU test of the accumulating launch rests on (a contracted multiply-add would show)."""
import os
from collections import defaultdict

import numpy as np
import pytest
import torch

import _sw_ref as S
from conftest import ROOT
from insenticap_model_amd import _lib, checkpoint, dp, rewards, synth

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'sw', 'reward.npz')


def cases():
    z = np.load(GOLDEN)
    for k in range(int(z['n_cases'][0])):
        c = {n[len('c%d_' % k):]: z[n] for n in z.files if n.startswith('c%d_' % k)}
        V, n_labels = (int(x) for x in c['dims'])
        lex = {lab: {} for lab in range(n_labels)}
        for lab, w, x in zip(c['lex_label'], c['lex_word'], c['lex_weight']):
            lex[int(lab)][int(w)] = float(x)
        acc = defaultdict(set)
        for lab, w in zip(c['acc_label'], c['acc_word']):
            acc[int(lab)].add(int(w))
        yield k, V, n_labels, lex, c['tok'], c['labels'], c['rewards'], dict(acc)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def test_fixture_covers_what_it_should():
    got = {k: (V, n, lex, tok, lab, rew, acc) for k, V, n, lex, tok, lab, rew, acc in cases()}
    assert len(got) == 3
    V, n, lex, tok, lab, rew, acc = got[0]
    assert lex[1] == {} and (lab == 1).any() and (rew[lab == 1] == 0).all()                  # an empty lexicon
    assert 5 in lex[0] and 5 in lex[2] and lex[0][5] != lex[2][5]                          # a word in two lexicons
    assert set(lex[2].values()) <= set(S.powers(0.9, 9)) and lex[2][12] == S.powers(0.9, 9)[7] != 0.9 ** 7
    assert (tok[1, -3:] == (2, 5, 7)).all() and (rew[1, -2:] == (lex[0][5], lex[0][7])).all()     # behind <EOS>: paid
    V, n, lex, tok, lab, rew, acc = got[1]
    pads = (tok == 0) & (lab == 0)[:, None]
    assert 0 in lex[0] and pads.any() and (rew[pads] == lex[0][0]).all()                    # <PAD> in the lexicon: paid
    assert got[2][3].shape[1] == 1


def test_host_function_reproduces_the_reference_in_bits():
    for k, V, n_labels, lex, tok, labels, want, acc in cases():
        for t, l in ((tok, labels), (torch.from_numpy(tok), torch.from_numpy(labels))):
            got, accur_w = rewards.get_senti_words_reward(t, l, lex)
            assert got.dtype == np.float64 and got.shape == tok.shape and np.array_equal(bits(got), bits(want)), k
            assert isinstance(accur_w, defaultdict) and accur_w.default_factory is set
            assert {a: {int(w) for w in ws} for a, ws in accur_w.items()} == acc, k
    with pytest.raises(KeyError):                                  # a label without an entry, as the reference
        rewards.get_senti_words_reward(np.zeros((1, 2), dtype=np.int64), np.asarray([3]), {0: {}})


def test_restatement_reproduces_the_reference_in_bits():
    for k, V, n_labels, lex, tok, labels, want, acc in cases():
        weights, state = S.table(lex, V, n_labels)
        r32, r64, hits, after = S.reward(tok, labels, weights, state)
        assert np.array_equal(bits(r64), bits(want)), k
        assert np.array_equal(r32, want.astype(np.float32)) and S.accur(state, after) == acc
        assert np.array_equal(hits, [sum(int(w) in lex[int(l)] for w in row) for row, l in zip(tok, labels)])
        assert np.array_equal(S.reward(tok, labels, weights, state, mark=False)[3], state)


def test_table_round_trips_and_refuses_ids_outside_the_vocabulary():
    for k, V, n_labels, lex, tok, labels, want, acc in cases():
        t = rewards.SentimentWordWeights.from_dict(lex, V, n_labels)
        assert t.weights.dtype == torch.float64 and t.state.dtype == torch.uint8
        assert tuple(t.weights.shape) == tuple(t.state.shape) == (n_labels, V) and (t.n_labels, t.vocab_size) == (n_labels, V)
        assert t.to_dict() == lex and all(type(x) is float for ws in t.to_dict().values() for x in ws.values())
        w, s = S.table(lex, V, n_labels)
        assert np.array_equal(t.weights.numpy(), w) and np.array_equal(t.state.numpy(), s)
    # membership is the state: weights 0.0 and negative stay members; a missing label is an empty lexicon
    odd = {0: {1: 0.0, 2: -0.5}}
    t = rewards.SentimentWordWeights.from_dict(odd, 4, 3)
    assert t.to_dict() == {0: {1: 0.0, 2: -0.5}, 1: {}, 2: {}} and t.state.tolist()[0] == [0, 1, 1, 0]
    for bad in ({0: {4: 1.0}}, {0: {-1: 1.0}}, {3: {0: 1.0}}, {-1: {}}):
        with pytest.raises(ValueError):
            rewards.SentimentWordWeights.from_dict(bad, 4, 3)


def test_host_decay_matches_a_python_loop_in_bits_over_several_rounds():
    rng = np.random.default_rng(3)
    V, n_labels = 50, 3
    lex = {lab: {int(w): 1.0 for w in rng.choice(V, size=12, replace=False)} for lab in range(n_labels)}
    loop = {lab: dict(ws) for lab, ws in lex.items()}
    t = rewards.SentimentWordWeights.from_dict(lex, V, n_labels)
    for rnd in range(7):
        used = {lab: {w for w in lex[lab] if rng.random() < 0.5} for lab in range(n_labels)}
        t.mark(used)
        assert int((t.state == 2).sum()) == sum(len(u) for u in used.values())
        t.decay(0.9)
        for lab, ws in used.items():                               # decoder.py:174-176
            for w in ws:
                loop[lab][w] *= 0.9
        assert t.to_dict() == loop and int((t.state == 2).sum()) == 0
        w_ref, s_ref = S.decay(*[x.numpy() for x in (t.weights, t.state)], 0.9)      # nothing marked: nothing changes
        assert np.array_equal(bits(w_ref), bits(t.weights.numpy()))
    vals = {x for ws in loop.values() for x in ws.values()}
    assert len(vals) > 4 and vals <= set(S.powers(0.9, 8))
    # the in-place update of a caller's dict keeps its keys and objects
    mine = {lab: dict(ws) for lab, ws in lex.items()}
    inner = mine[1]
    assert t.update_dict(mine) is mine and mine[1] is inner and mine == loop


# ------------------------------------------------------------------------------------------------ Detector, checkpoint
def _detector():
    from insenticap_model_amd.detector import Detector
    st = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
    return Detector(synth.make_idx2word(64), 8, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-4}, st)


def test_detector_defaults_and_refusals(monkeypatch):
    det = _detector()
    assert (det.senti_words_flag, det.senti_words_decay, det.senti_words_form) == (0.0, 0.9, 'device')
    det.senti_words_flag = 0.05
    with pytest.raises(ValueError, match='set_sentiment_words'):
        det(([],), 'fact', False)
    lex = {0: {5: 1.0}, 1: {}, 2: {6: 1.0}}
    det.set_sentiment_words(lex)
    assert det.sentiment_words is lex
    det.senti_words_form = 'kernel'
    with pytest.raises(ValueError, match='senti_words_form'):
        det(([],), 'fact', False)
    det.senti_words_form = 'host'
    monkeypatch.setattr(dp, 'distributed', lambda group=None: True)
    det.dp_arena = object()
    with pytest.raises(ValueError, match='not built'):
        det(([], []), 'fact', True)
    det.senti_words_flag = 0.0
    det.set_sentiment_words({0: {64: 1.0}})                          # an id outside the vocabulary: refused when the table is built
    det.dp_arena = None
    det.senti_words_flag, det.senti_words_form = 0.05, 'device'
    with pytest.raises(ValueError, match='outside'):
        det(([],), 'fact', False)


def test_checkpoint_carries_the_weights_only_with_the_term_on(tmp_path):
    det = _detector()
    lex = {0: {5: 0.9 * 0.9, 7: 1.0}, 1: {}, 2: {np.int64(6): np.float64(0.9)}}
    det.set_sentiment_words(lex)
    args = (3, det, {'a': 1}, ['<PAD>'], 8, synth.SENTIMENT_CATEGORIES, 'coco', 'part')
    off = checkpoint.save_rl_checkpoint(str(tmp_path / 'off'), *args)
    keys = set(torch.load(off, weights_only=False))
    assert keys == {'epoch', 'model', 'settings', 'idx2word', 'max_seq_len', 'sentiment_categories', 'dataset_name',
                    'corpus_type'}
    assert checkpoint.load_sentiment_words(off) is None
    det.senti_words_flag = 0.05
    on = checkpoint.save_rl_checkpoint(str(tmp_path / 'on'), *args)
    assert set(torch.load(on, weights_only=False)) == keys | {'sentiment_words'}
    back = checkpoint.load_sentiment_words(on)
    assert back == {0: {5: 0.9 * 0.9, 7: 1.0}, 1: {}, 2: {6: 0.9}}
    assert all(type(w) is int and type(x) is float for ws in back.values() for w, x in ws.items())
    det2 = _detector()
    det2.set_sentiment_words(back)
    assert det2.sentiment_words is back


def test_abi_names():
    hdr = open(os.path.join(ROOT, 'include', 'insenticap_hip.h')).read()
    for name in ('isc_sw_reward', 'isc_sw_decay'):
        assert name in _lib.SIGNATURES and ('int %s(' % name) in hdr
    assert len(_lib.SIGNATURES['isc_sw_reward'][1]) == 15 and len(_lib.SIGNATURES['isc_sw_decay'][1]) == 5


def test_the_accumulate_case_tells_a_fused_multiply_add_from_two_roundings():
    """base + (float)flag * (float)w with the product rounded to float32 first (torch's `rewards + flag * sw`) against
    the fused form (one rounding of the exact sum): at least 50 of the 4096 results differ (186 with default_rng(0)), so
    the GPU test of the accumulating launch cannot pass with a contracted multiply-add."""
    base, k, pw = S.accumulate_case()
    wf = pw[k].astype(np.float32)
    f = np.float32(0.05)
    unfused = base + (f * wf).astype(np.float32)
    assert unfused.dtype == np.float32
    # a float32 x float32 product is exact in float64 (48 bits); the sum of it and a float32 is not always, but float64
    # carries 53 bits against the 24 kept: double rounding can only matter on an exact tie of the 53-bit sum, counted below
    exact = base.astype(np.float64) + f.astype(np.float64) * wf.astype(np.float64)
    fused = exact.astype(np.float32)
    differ = int((bits(unfused) != bits(fused)).sum())
    print('accumulate case: %d of %d results differ between the unfused and the fused formula' % (differ, base.size))
    assert differ >= 50
    t = torch.from_numpy(base) + 0.05 * torch.from_numpy(wf)       # torch's expression on the CPU: the unfused bits
    assert np.array_equal(bits(t.numpy()), bits(unfused))
    r32 = S.reward(k[:, None], np.zeros(len(k), dtype=np.int64), pw[None, :], np.ones((1, 12), dtype=np.uint8), 0.05,
                   base[:, None], accumulate=True)[0]
    assert np.array_equal(bits(r32[:, 0]), bits(unfused))
