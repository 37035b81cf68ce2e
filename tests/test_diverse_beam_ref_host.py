"""CPU checks of the diverse beam search (beam_groups / diversity): the restatement of tests/_diverse_beam_ref.py against
the plain search's restatement and against its own definition - what tests/test_gpu_diverse_beam_kernels.py and
tests/test_gpu_diverse_beam.py rest on - and the host-side refusals of the new entry points and keywords.

The containment property.  The kernels read a row's raw top-`beam`, the definition ranks the whole vocabulary.  A child
that can enter group g's best bp = beam / G lies in its row's best bp by key; at most P <= g bp distinct tokens are
penalised and a penalty only lowers a key; a token outside the row's raw top-(bp + P) has bp un-penalised tokens in front
of it in raw order, whose keys are >= its own and which, on equality, were inserted earlier; bp + g bp <= beam.  So
both forms select the same candidates in the same order - checked here on random rows and on dyadic rows where lambda
equals logit gaps and penalised and un-penalised keys tie exactly.

The end-to-end case set has no near tie: for every (step, group) of every case of D.CASES, with and without the trigram /
minimum-length controls, the neighbouring keys from the best candidate down to the first rejected one are more than
D.MARGIN = 2e-3 (the margin of tests/test_widths_host.py) apart in the fp64 run, and the fp32 run selects the same
tokens.  A device whose scores are within 1e-3 of the fp64 ones cannot flip a selection: the GPU test needs no flip
allowance."""
import ctypes

import numpy as np
import pytest
import torch

import _beam_ref as BR
import _diverse_beam_ref as D
from insenticap_model_amd import _lib, ops

SHAPES = ((2, 2), (4, 2), (6, 3), (6, 2), (8, 2), (8, 4), (8, 8))
EOS = BR.EOS


# ------------------------------------------------------------------------------------------------ G = 1: the plain search
@pytest.mark.parametrize('kw', [s for s in BR.scenarios() if s['n_img'] <= 9], ids=lambda k: 's%d' % k['seed'])
def test_one_group_is_the_plain_candidate_loop(kw):
    S = BR.make_step(V=50, **kw)
    args = (S['top_val'], S['top_idx'], S['score_in'], S['last_in'], S['words_in'], S['len_in'], S['done'], S['t'], S['T'],
            S['eos'], S['beam'])
    want = BR.merge_ref(*args)
    for lam in (0.0, 0.75, 1e3):
        assert D.merge_groups_ref(*args, 1, lam) == want


# ------------------------------------------------------------------------------------------------ a toy model
def toy_row(seed, prefix, V, lattice):
    """The 'log-probs' after `prefix`: a function of the words alone (specials and the last word at -inf, <EOS> likely)."""
    rng = np.random.default_rng([seed] + [int(w) for w in prefix])
    row = D.dyadic_rows(rng, 1, V)[0] if lattice else (-rng.random(V) * 6.0).astype(np.float32).astype(np.float64).tolist()
    if rng.random() < 0.35:
        row[EOS] = 0.0
    for w in (BR.PAD, BR.SOS, BR.UNK) + ((prefix[-1],) if prefix else ()):
        row[w] = D.NEG
    return row


def toy_search(seed, beam, G, lam, T, V, full=True, lattice=False, trace=None):
    """The definition (full) or the kernels' form (raw top-`beam` per row) on the toy model -> per step the `new` lists."""
    cands = [(0.0, BR.SOS, []) for _ in range(beam)]
    steps = []
    for t in range(T):
        parents = []
        for (score, last, words) in cands:
            children = D.order_row(toy_row(seed, words, V, lattice))
            parents.append((score, last, children if full else children[:beam]))
        new, all_ended, _ = D.select_step(parents, G, lam, t, EOS, trace)
        cands = [(s, w, cands[k][2] + ([] if car else [w])) for (s, w, k, car) in new]
        steps.append(new)
        if all_ended:
            break
    return steps, cands


@pytest.mark.parametrize('beam,G', SHAPES)
def test_zero_lambda_groups_are_plain_beams(beam, G):
    """lambda = 0: no group sees the others - each is the plain search of width beam / G."""
    bp = beam // G
    for seed in range(4):
        _, got = toy_search(seed, beam, G, 0.0, 7, 30)
        _, plain = toy_search(seed, bp, 1, 0.0, 7, 30)
        for g in range(G):
            assert got[g * bp:(g + 1) * bp] == plain


def test_zero_lambda_on_the_oracle():
    name, _, pairs, beam, G, _ = D.CASES['tiny_one']
    from oracle import captioner_oracle as O
    st, w, d, T_, _ = D.model(name)
    i2w, ids = D.model_ids(name)
    image, label = pairs[0]
    caps, scores, seqs, _ = D.run(name, image, label, beam, G, 0.0)
    with torch.no_grad():
        ref = O.beam_search(O.to_params(w, dtype=torch.float64), ids, i2w, D.Wd.cpu(d, 'fc_feats', dtype=torch.float64)[image],
                            D.Wd.cpu(d, 'att_feats', dtype=torch.float64)[image], D.Wd.cpu(d, 'senti_words')[image],
                            torch.tensor([label]), beam // G, 1, T_)
    bp = beam // G
    for g in range(G):
        assert (caps[g * bp:(g + 1) * bp], scores[g * bp:(g + 1) * bp], seqs[g * bp:(g + 1) * bp]) == tuple(ref)
    # ... and one group is the oracle's search itself
    with torch.no_grad():
        ref = O.beam_search(O.to_params(w, dtype=torch.float64), ids, i2w, D.Wd.cpu(d, 'fc_feats', dtype=torch.float64)[image],
                            D.Wd.cpu(d, 'att_feats', dtype=torch.float64)[image], D.Wd.cpu(d, 'senti_words')[image],
                            torch.tensor([label]), beam, 1, T_)
    assert D.run(name, image, label, beam, 1, 0.7)[:3] == tuple(ref)


# ------------------------------------------------------------------------------------------------ containment
@pytest.mark.parametrize('beam,G', SHAPES)
def test_raw_topk_suffices_on_random_rows(beam, G):
    for seed in range(6):
        for lam in (0.0, 0.3, 1.0, 1e3):
            full, _ = toy_search(seed, beam, G, lam, 6, 40, full=True)
            cut, _ = toy_search(seed, beam, G, lam, 6, 40, full=False)
            assert full == cut, (seed, lam)


@pytest.mark.parametrize('lam', [0.25, 0.5])
@pytest.mark.parametrize('beam,G', SHAPES)
def test_raw_topk_suffices_on_the_lattice(beam, G, lam):
    """Logits in multiples of 0.25 and lambda a multiple of it: penalised and un-penalised keys tie exactly, and the
    insertion order decides - in both forms alike."""
    ties = 0
    for seed in range(6):
        trace = []
        full, _ = toy_search(seed, beam, G, lam, 6, 24, full=True, lattice=True, trace=trace)
        cut, _ = toy_search(seed, beam, G, lam, 6, 24, full=False, lattice=True)
        assert full == cut, seed
        for ranked in trace:                               # a penalised key equal to an un-penalised one, both finite
            pen = {c[0] for c in ranked if not c[4] and c[0] != c[1]}
            ties += any(c[0] in pen for c in ranked if c[0] == c[1] and c[0] > D.NEG)
    assert ties > 0 or G == 1


def test_large_lambda_selects_distinct_tokens():
    for beam, G in SHAPES:
        steps, _ = toy_search(3, beam, G, 1e3, 4, 40)
        for new in steps:
            heads = [new[g * (beam // G)][1] for g in range(G) if not new[g * (beam // G)][3]]
            assert len(set(heads)) == len(heads)           # the groups' best candidates never share a token


# ------------------------------------------------------------------------------------------------ the end-to-end cases
@pytest.mark.parametrize('case', sorted(D.CASES))
def test_cases_are_decided(case):
    name, kind, pairs, beam, G, lam = D.CASES[case]
    assert beam % G == 0 and G > 1
    for control in ((0, 0), D.TRIGRAM):
        want = D.expected(case, control)
        r32 = D.expected(case, control, dtype=torch.float32)
        cut = D.expected(case, control, full=False)
        for (caps, scores, seqs, gap), b, c in zip(want, r32, cut):
            assert gap > D.MARGIN, (case, control, gap)
            assert b[2] == seqs and b[0] == caps
            assert max(abs(x - y) for x, y in zip(b[1], scores)) <= 1e-4
            assert c[:3] == (caps, scores, seqs)
            assert len(seqs) == beam and all(NB_ok(w, control, D.model(name)[3]) for w in seqs)


def test_zero_lambda_cases_are_decided():
    """The two one-image cases at lambda = 0 (test_gpu_diverse_beam.py compares their groups with plain beams of width
    beam / G on the device): the same margin."""
    for case in ('tiny_one', 'wide_one'):
        name, _, pairs, beam, G, _ = D.CASES[case]
        assert D.run(name, pairs[0][0], pairs[0][1], beam, G, 0.0)[3] > D.MARGIN


def NB_ok(words, control, T_):
    n, min_len = control
    return (n == 0 or D.NB.repeated_ngrams(words, n) == 0) and (len(words) >= min_len or len(words) == T_)


def test_cases_show_the_feature():
    """The groups change the result (vs one group) and the controls change it again, in at least half of the searches."""
    differs = binds = 0
    for case, (name, kind, pairs, beam, G, lam) in D.CASES.items():
        for (image, label), got, ctl in zip(pairs, D.expected(case), D.expected(case, D.TRIGRAM)):
            plain = D.run(name, image, label, beam, 1, 0.0)
            differs += sorted(map(tuple, got[2])) != sorted(map(tuple, plain[2]))
            binds += got[2] != ctl[2]
    print('searches whose captions the groups change: %d, the controls: %d (of 12)' % (differs, binds))
    assert differs >= 6 and binds >= 6, (differs, binds)


# ------------------------------------------------------------------------------------------------ host-side refusals
def test_entry_points_refuse_bad_groups_without_a_gpu():
    lib = _lib.load()
    m, s = _lib.BeamMergeArgs(), _lib.BeamSelectArgs()
    assert lib.isc_beam_merge_groups(None, 2, 0.5, None) == -1 and lib.isc_beam_select_groups(None, 2, 0.5, None) == -1
    assert lib.isc_beam_merge_groups(ctypes.byref(m), 2, 0.5, None) == -1          # null tables
    assert lib.isc_beam_select_groups(ctypes.byref(s), 2, 0.5, None) == -1
    for name, _ in _lib.BeamMergeArgs._fields_[5:]:
        setattr(m, name, 4096)                                                     # (never dereferenced: refused first)
    for name in ('part_max part_sum cand_val cand_idx score_in score_out last_in last_out words_in words_out len_in len_out '
                 'done src_row live').split():
        setattr(s, name, 4096)
    m.n_img, m.beam, m.T, m.t = 1, 6, 4, 1
    s.n_img, s.beam, s.T, s.t, s.n_tile, s.V = 1, 6, 4, 1, 2, 30
    for G, lam in ((0, 0.5), (-1, 0.5), (4, 0.5), (5, 0.5), (7, 0.0), (2, -0.5), (2, float('inf')), (2, float('nan')),
                   (3, -1e-300)):
        assert lib.isc_beam_merge_groups(ctypes.byref(m), G, lam, None) == -2, (G, lam)
        assert lib.isc_beam_select_groups(ctypes.byref(s), G, lam, None) == -2, (G, lam)
    m.beam = s.beam = 9                                                            # beam <= 8, as the plain entry points
    assert lib.isc_beam_merge_groups(ctypes.byref(m), 3, 0.5, None) == -2
    assert lib.isc_beam_select_groups(ctypes.byref(s), 3, 0.5, None) == -2


def test_keyword_values_are_checked_on_the_host():
    assert ops.check_beam_groups(1, 0.0, 5, True) == (1, 0.0)
    assert ops.check_beam_groups(1, 2.5, 9, False) == (1, 2.5)                     # one group asks nothing of the merge
    assert ops.check_beam_groups(3, 0.5, 6, True) == (3, 0.5)
    assert ops.check_beam_groups(8, 1, 8, True) == (8, 1.0)
    for G, lam, beam in ((0, 0.5, 6), (-2, 0.5, 6), (2.0, 0.5, 6), (True, 0.5, 6), (None, 0.5, 6), ('2', 0.5, 6), (4, 0.5, 6),
                         (2, -0.1, 6), (2, float('inf'), 6), (2, float('nan'), 6), (2, None, 6), (2, '0.5', 6), (2, True, 6)):
        with pytest.raises(ValueError):
            ops.check_beam_groups(G, lam, beam, True)
    with pytest.raises(ValueError, match='not built'):
        ops.check_beam_groups(2, 0.5, 6, False)
    with pytest.raises(ValueError, match='not built'):
        ops.check_beam_groups(3, 0.5, 9, True)


def test_bad_keywords_raise_before_anything_touches_the_device():
    """A captioner on the CPU cannot search: a bad value is still a ValueError (checked first), a good one reaches the
    usual loud failure."""
    from insenticap_model_amd import Captioner, synth
    V, st = 64, synth.TINY_SETTINGS
    cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st).eval()
    d = synth.make_inputs(1, V, st, regions=5, seq_len=8, seed=1)
    fc, att, sw = (torch.from_numpy(d[k]) for k in ('fc_feats', 'att_feats', 'senti_words'))
    lab = torch.tensor([1])
    for kw in (dict(beam_groups=4), dict(beam_groups=0), dict(beam_groups=2.0), dict(beam_groups=2, diversity=-1.0),
               dict(beam_groups=2, diversity=float('nan')), dict(diversity='x')):
        with pytest.raises(ValueError):
            cap.sample_batch(fc, att, sw, lab, 6, 1, 8, **kw)
        with pytest.raises(ValueError):
            cap.sample(fc[0], att[0], sw[0], lab, 6, 1, 8, **kw)
        with pytest.raises(ValueError):
            cap.sample_sentiments(fc, att, sw, torch.tensor([[0, 1]]), 6, 1, 8, **kw)
    cap.beam_device_merge = False
    with pytest.raises(ValueError, match='not built'):
        cap.sample_batch(fc, att, sw, lab, 6, 1, 8, beam_groups=2)
    del cap.beam_device_merge
    with pytest.raises(Exception) as e:
        cap.sample_batch(fc, att, sw, lab, 6, 1, 8, beam_groups=3, diversity=0.5)
    assert not isinstance(e.value, (ValueError, TypeError))
