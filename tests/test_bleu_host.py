"""BLEU as the self-critical reward and metric, host side: the native scorer (isc_bleu_score, rewards.Bleu) against the
fixture of the reference's scorer (tests/golden/bleu.npz) and the Python restatement (tests/_bleu_ref.py) - the integer
statistics exactly, the scores to 1e-12 relative -, the reward functions with a `Bleu`, and the references cooked for
the device.  CPU only."""
import numpy as np
import pytest

import _bleu_ref as R
from insenticap_model_amd import rewards

SOS, EOS = R.SOS, R.EOS
_CACHE = {}


def case(golden, name):
    """(hyps, refs per image, refs per row, fixture scores, fixture corpus, restatement stats), built once per set."""
    if name not in _CACHE:
        hyps, refs, per_row, scores, corpus = R.load_set(golden('bleu'), name)
        _CACHE[name] = (hyps, refs, per_row, scores, corpus, R.score_rows(hyps, per_row)[0])
    return _CACHE[name]


@pytest.mark.parametrize('name', ['small', 'cfg5'])
def test_scores_and_statistics_match_the_fixture_and_the_restatement(golden, name):
    hyps, refs, per_row, scores, corpus, ref_stats = case(golden, name)
    b = rewards.Bleu(SOS, EOS)
    got = b.score4(hyps, per_row)
    assert got.dtype == np.float64 and got.shape == (len(hyps), 4)
    err = R.rel_err(got, scores)
    print('BLEU host [%s]: max relative difference to the fixture %.3e' % (name, err))
    assert err <= R.RTOL
    stats = b.stats(hyps, per_row)
    assert stats.dtype == np.int32 and stats.shape == (len(hyps), 10)
    assert np.array_equal(stats, ref_stats)
    for order in (1, 2, 3, 4):
        one = rewards.Bleu(SOS, EOS, order=order).score_arrays(hyps, per_row)
        assert one.shape == (len(hyps),) and np.array_equal(one, got[:, order - 1])


@pytest.mark.parametrize('name', ['small', 'cfg5'])
def test_compute_score_has_the_reference_wrappers_return(golden, name):
    hyps, refs, per_row, scores, corpus, _ = case(golden, name)
    text = lambda row: ' '.join(str(w) for w in R.normalise(row, SOS, EOS))
    gts = {'img%d' % i: [text(c) for c in caps] for i, caps in enumerate(refs)}
    res = [{'image_id': 'img%d' % (r % len(refs)), 'caption': [text(row)]} for r, row in enumerate(hyps)]
    b = rewards.Bleu(SOS, EOS)
    score, lists = b.compute_score(gts, res)
    assert isinstance(score, list) and len(score) == 4 and len(lists) == 4 and b.method() == 'Bleu'
    assert R.rel_err(score, corpus) <= R.RTOL
    assert R.rel_err(np.asarray(lists).T, scores) <= R.RTOL
    with pytest.raises(ValueError):
        b.compute_score({'a': ['4 5 2']}, [{'image_id': 'a', 'caption': ['a man 2']}])      # no ids


def test_thread_counts_give_the_same_bits(golden):
    hyps, refs, per_row, scores, corpus, _ = case(golden, 'cfg5')
    a = rewards.Bleu(SOS, EOS, n_threads=1)
    b = rewards.Bleu(SOS, EOS, n_threads=16)
    assert a.n_threads == 1 and b.n_threads == 16
    assert np.array_equal(a.score4(hyps, per_row), b.score4(hyps, per_row))
    assert np.array_equal(a.stats(hyps, per_row), b.stats(hyps, per_row))


def test_row_div(golden):
    """Rows r = 5 i + j against image i: the bits of the one-row-per-image call with the references repeated."""
    hyps, refs, per_row, scores, corpus, _ = case(golden, 'cfg5')
    I = 100
    rows = np.ascontiguousarray(np.stack([hyps[(i + 37 * j) % len(hyps)] for i in range(I) for j in range(5)]))
    b = rewards.Bleu(SOS, EOS)
    grouped = b.score4(rows, refs[:I], row_div=5)
    single = b.score4(rows, [refs[r // 5] for r in range(5 * I)])
    assert np.array_equal(grouped, single)
    assert np.array_equal(b.stats(rows, refs[:I], row_div=5), R.score_rows(rows, refs[:I], row_div=5)[0])
    assert np.array_equal(b.score4(rows[:7], refs[:2], row_div=5), grouped[:7])         # the last image partly filled
    with pytest.raises(RuntimeError):
        b.score4(rows[:11], refs[:2], row_div=5)                                      # 11 rows need 3 images
    with pytest.raises(RuntimeError):
        b.score4(rows[:1], [[]])                                                      # an image without references


def test_flatten_refs_caches_per_image(golden):
    hyps, refs, per_row, scores, corpus, _ = case(golden, 'small')
    b = rewards.Bleu(SOS, EOS)
    keys = ['k%d' % i for i in range(len(refs))]
    flat = b.flatten_refs(refs, keys=keys)
    plain = b.flatten_refs(refs)
    assert all(np.array_equal(x, y) for x, y in zip(flat, plain)) and sorted(b._gt_cache) == sorted(keys)
    kept = b._gt_cache['k0']
    again = b.flatten_refs([[[SOS, 9, EOS]]] + refs[1:], keys=keys)                     # the cached image 0 is served
    assert b._gt_cache['k0'] is kept and all(np.array_equal(x, y) for x, y in zip(again, plain))
    assert np.array_equal(b.score4(hyps[:len(refs)], None, flat), b.score4(hyps[:len(refs)], refs))


@pytest.mark.parametrize('order', [4, 2])
def test_self_critical_reward_with_a_bleu_scorer(golden, order):
    hyps, refs, per_row, scores, corpus, _ = case(golden, 'cfg5')
    I = len(refs)
    fns = ['f%d' % i for i in range(I)]
    gt = dict(zip(fns, refs))
    sample, greedy = hyps[:I], hyps[I:]
    scorer = rewards.get_bleu_scorer(SOS, EOS, order=order)
    assert isinstance(scorer, rewards.Bleu) and scorer.order == order
    rew = rewards.get_self_critical_reward(sample, greedy, fns, gt, SOS, EOS, scorer)
    assert rew.dtype == np.float64 and rew.shape == sample.shape and (rew == rew[:, :1]).all()
    s4 = scorer.score4(hyps, per_row)
    assert np.array_equal(rew[:, 0], s4[:I, order - 1] - s4[I:, order - 1])
    want = scores[:I, order - 1] - scores[I:, order - 1]
    assert np.abs(rew[:, 0] - want).max() <= R.RTOL * np.abs(scores[:, order - 1]).max()
    halves = rewards.self_critical_scores(sample, fns, gt, scorer) - rewards.self_critical_scores(greedy, fns, gt, scorer)
    assert np.array_equal(halves, rew[:, 0])
    import torch
    assert np.array_equal(rewards.get_self_critical_reward(torch.from_numpy(sample), torch.from_numpy(greedy), fns, gt,
                                                           SOS, EOS, scorer), rew)


def test_group_functions_accept_a_bleu_scorer(golden):
    hyps, refs, per_row, scores, corpus, _ = case(golden, 'cfg5')
    I, n = 40, 3
    fns = ['f%d' % i for i in range(I)]
    gt = dict(zip(fns, refs[:I]))
    rows = np.ascontiguousarray(np.stack([hyps[(i + 512 * j + 5 * (j // 2)) % len(hyps)] for i in range(I) for j in range(n)]))
    scorer = rewards.get_bleu_scorer(SOS, EOS)
    got = rewards.group_self_critical_scores(rows, fns, gt, scorer, n)
    assert np.array_equal(got, scorer.score_arrays(rows, refs[:I], row_div=n))
    rew = rewards.get_group_self_critical_reward(rows, fns, gt, scorer, n)
    assert rew.shape == rows.shape and np.array_equal(rew[:, 0], rewards.group_advantages(got, n))


def test_an_unknown_scorer_still_raises():
    hyp = np.zeros((1, 4), dtype=np.int64)
    for bad in (object(), None, 'Bleu'):
        with pytest.raises(Exception, match='do not support this scorer'):
            rewards.get_self_critical_reward(hyp, hyp, ['a'], {'a': [[SOS, 4, EOS]]}, SOS, EOS, bad)
        with pytest.raises(Exception, match='do not support this scorer'):
            rewards.self_critical_scores(hyp, ['a'], {'a': [[SOS, 4, EOS]]}, bad)
        with pytest.raises(Exception, match='do not support this scorer'):
            rewards.get_self_critical_reward_device(hyp, hyp, None, bad)
    with pytest.raises(ValueError):
        rewards.Bleu(SOS, EOS, order=5)
    with pytest.raises(ValueError):
        rewards.Bleu(SOS, EOS, n=2, order=3)


def test_cooked_references_field_by_field(golden):
    hyps, refs, per_row, scores, corpus, _ = case(golden, 'small')
    b = rewards.Bleu(SOS, EOS)
    for caps in refs + case(golden, 'cfg5')[1][:16]:
        keys, counts, ent_off, lens = b.cook_refs(caps)
        want_keys, want_counts, want_off, want_lens = R.cook_device(caps)
        assert keys.dtype == np.uint64 and counts.dtype == np.int32 and ent_off.dtype == np.int32 and lens.dtype == np.int32
        assert [int(k) for k in keys] == want_keys and counts.tolist() == want_counts
        assert ent_off.tolist() == want_off and lens.tolist() == want_lens
    assert len(b.cook_refs(refs[4])[0]) > 128                                  # the image of the third hand-round batch
    with pytest.raises(ValueError):
        b.cook_refs([[SOS, 5, 65535, EOS]])
    with pytest.raises(ValueError):
        b.to_device('cpu', 65536)
    with pytest.raises(ValueError):
        rewards.DeviceBleu(b, 'cpu', 65536)
