"""Host side of self-critical RL on n samples per image (no GPU): the numpy reference of the group reward against itself,
rewards.get_group_self_critical_reward against that reference and against the CIDEr-D oracle, the argument checks of the
differentiable grouped roll-out (all before anything touches a device), isc_group_reward's refusals and
Detector.rl_samples_per_image."""
import ctypes

import numpy as np
import pytest
import torch

import _group_reward_ref as GR
from insenticap_model_amd import Captioner, _lib, rewards, synth
from oracle.ciderd_oracle import CiderDOracle

ST = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
SHAPES = [(1, 2, 1), (3, 5, 8), (2, 8, 20), (5, 3, 17), (300, 5, 20)]


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize('I,n,T', SHAPES)
def test_reference_advantages_are_the_scaled_deviation_from_the_image_mean(I, n, T):
    """s_j - mean of the others = n/(n-1) * (s_j - mean of all): within 1e-12 * max|s|."""
    s = GR.make_scores(I, n, seed=I + n)
    adv = GR.advantages(s, n).reshape(I, n)
    s2 = s.reshape(I, n)
    want = n / (n - 1.0) * (s2 - s2.mean(1, keepdims=True))
    assert np.abs(adv - want).max() <= 1e-12 * np.abs(s).max()
    assert s.max() <= 10.0 and (s == 0).any() == (I > 1)


def test_reference_with_two_samples_is_the_signed_difference_exactly():
    s = np.random.default_rng(3).random(14) * 10.0
    adv = GR.advantages(s, 2).reshape(-1, 2)
    s2 = s.reshape(-1, 2)
    assert np.array_equal(adv[:, 0], s2[:, 0] - s2[:, 1]) and np.array_equal(adv[:, 1], s2[:, 1] - s2[:, 0])


@pytest.mark.parametrize('n', [2, 3, 5, 8])
def test_reference_with_equal_scores_gives_advantages_at_rounding_level(n):
    """Equal scores inside an image: |adv| <= 4 * 2^-53 * |s| (the sum of n - 1 equal terms and its division round)."""
    for s in (0.0, 1.0, 0.1, 3.3333333333333335, 9.999999999, 10.0, 1e-7):
        adv = GR.advantages(np.full(2 * n, s), n)
        assert np.abs(adv).max() <= 4 * 2.0 ** -53 * abs(s), (n, s)


def test_reference_reward_and_statistics_follow_the_definitions():
    I, n, T = 3, 4, 5
    rng = np.random.default_rng(0)
    s = GR.make_scores(I, n, seed=1)
    cls = rng.random((I * n, T)).astype(np.float32)
    adv, rw, st = GR.group_reward(s, n, T, cls, 0.4)
    assert rw.dtype == np.float32 and rw.shape == (I * n, T)
    want = (adv[:, None] + 0.4 * cls.astype(np.float64)).astype(np.float32)
    assert np.array_equal(rw, want)
    np.testing.assert_allclose(st, [s.mean(), adv.mean(), cls.astype(np.float64).mean(), rw.astype(np.float64).mean()],
                               rtol=1e-13, atol=1e-15)
    adv0, rw0, st0 = GR.group_reward(s, n, T)
    assert np.array_equal(rw0, np.repeat(adv0.astype(np.float32)[:, None], T, 1)) and st0[2] == 0.0
    assert abs(st0[1]) <= 1e-14 * np.abs(s).max()                 # the mean advantage is 0 up to rounding


# ------------------------------------------------------------------------------------------------ rewards.py
def _cider_case(I, n):
    split, fns, gt, sample, _ = synth.make_cider_data(40, 60, I * n, seq_len=12, seed=7)
    assert sample.shape[0] == I * n
    return split, list(fns[:I]), gt, sample


@pytest.mark.parametrize('I,n', [(5, 3), (8, 2), (3, 5)])
def test_group_reward_on_the_host_equals_the_reference_bit_for_bit(I, n):
    """Every row scored against ITS image's references (the CIDEr-D oracle on the same captions, the 1e-12 of
    tests/test_cider.py); the advantages repeated over T equal the explicit-loop reference bit for bit."""
    split, fns, gt, sample = _cider_case(I, n)
    scorer = rewards.get_ciderd_scorer(split, 1, 2)
    scores = rewards.group_self_critical_scores(sample, fns, gt, scorer, n)
    assert scores.dtype == np.float64 and scores.shape == (I * n,)
    caps = {}
    for v in split.values():
        caps.update(v)
    orc = CiderDOracle(list(caps.values()), 1, 2)
    want = [orc.score(sample[r], gt[fns[r // n]]) for r in range(I * n)]
    np.testing.assert_allclose(scores, want, rtol=0, atol=1e-12)
    assert scores.max() > 0.1 and (scores > 0).sum() >= I * n - 2     # (n-gram overlap; rows of other images score low)
    rew = rewards.get_group_self_critical_reward(sample, fns, gt, scorer, n)
    assert rew.dtype == np.float64 and rew.shape == sample.shape
    ref = np.repeat(GR.advantages(scores, n)[:, None], sample.shape[1], 1)
    assert np.array_equal(rew, ref)
    assert np.array_equal(rewards.get_group_self_critical_reward(torch.from_numpy(sample), fns, gt, scorer, n), ref)
    assert np.array_equal(rewards.group_advantages(GR.make_scores(300, 5, 2), 5), GR.advantages(GR.make_scores(300, 5, 2), 5))


def test_group_reward_on_the_host_checks_its_shapes():
    split, fns, gt, sample = _cider_case(5, 3)
    scorer = rewards.get_ciderd_scorer(split, 1, 2)
    for n in (1, 0, 2.0, True, None):
        with pytest.raises(ValueError, match='n >= 2'):
            rewards.group_self_critical_scores(sample, fns, gt, scorer, n)
    with pytest.raises(ValueError, match='sampled rows'):
        rewards.group_self_critical_scores(sample, fns, gt, scorer, 2)
    with pytest.raises(ValueError, match='whole number'):
        rewards.group_advantages(np.zeros(7), 2)


# ------------------------------------------------------------------------------------------------ forward_rl's checks
def make():
    return Captioner(synth.make_idx2word(64), synth.SENTIMENT_CATEGORIES, synth.TINY_SETTINGS)


def cpu_inputs(B=2, T=4):
    d = synth.make_inputs(B, 64, synth.TINY_SETTINGS, regions=6, seq_len=T, seed=0)
    return [torch.from_numpy(d[k]) for k in ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')]


def test_grouped_rollout_with_gradients_passes_its_checks_and_reaches_the_device():
    """Training mode, gradients enabled, n = 3 on CPU tensors: every argument check passes - also with `_replay`,
    `_masks` and the token constraints - and the call gets as far as the device (HipLibraryError: no CPU path)."""
    a = cpu_inputs()
    cap = make().train()
    for kw in (dict(), dict(_replay=torch.zeros(6, 4, dtype=torch.int64)), dict(_masks={}),
               dict(suppress_special=True, decoding_constraint=1, min_len=2)):
        with pytest.raises(_lib.HipLibraryError):
            cap.forward_rl(*a, 4, 0, captions_per_image=3, **kw)


def test_grouped_rollout_with_gradients_refuses_before_the_device():
    """Labels of I*n entries, greedy with n > 1 and filtered sampling with gradients: ValueErrors on CPU tensors (a call
    that got as far as the device would raise HipLibraryError)."""
    fc, att, cpt, sw, labels = cpu_inputs()
    cap = make().train()
    with pytest.raises(ValueError, match='one label per image'):
        cap.forward_rl(fc, att, cpt, sw, labels.repeat_interleave(3), 4, 0, captions_per_image=3)
    with pytest.raises(ValueError, match='sample_max=0'):
        cap.forward_rl(fc, att, cpt, sw, labels, 4, 1, captions_per_image=3)
    for kw in (dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9)):
        with pytest.raises(ValueError, match='filtered sampling'):
            cap.forward_rl(fc, att, cpt, sw, labels, 4, 0, captions_per_image=3, **kw)
    with pytest.raises(ValueError, match='_replay'):                   # forced tokens exclude the constraints
        cap.forward_rl(fc, att, cpt, sw, labels, 4, 0, captions_per_image=3, min_len=2,
                       _replay=torch.zeros(6, 4, dtype=torch.int64))
    # the two forms do not mix: gradients in eval mode, training mode without gradients
    with pytest.raises(ValueError, match='training mode with gradients enabled'):
        cap.eval().forward_rl(fc, att, cpt, sw, labels, 4, 0, captions_per_image=3)
    with torch.no_grad(), pytest.raises(ValueError, match='training mode with gradients enabled'):
        cap.train().forward_rl(fc, att, cpt, sw, labels, 4, 0, captions_per_image=3)


# ------------------------------------------------------------------------------------------------ isc_group_reward, refusals
def test_group_reward_entry_point_refuses_before_any_launch():
    """NULL pointers: ISC_E_NULL; n < 2, I < 1, T < 1: ISC_E_SHAPE - from the entry point's own checks, before a launch
    (the buffers here are host memory: nothing may touch them), and they keep their sentinel."""
    lib = _lib.load()
    scores = (ctypes.c_double * 8)(*[1.0] * 8)
    reward = (ctypes.c_float * 64)(*[-7.0] * 64)
    stats = (ctypes.c_double * 4)(*[-7.0] * 4)
    p = lambda x: ctypes.cast(x, ctypes.c_void_p)
    assert lib.isc_group_reward(None, 2, 2, None, 0.4, 4, p(reward), p(stats), None) == -1
    assert lib.isc_group_reward(p(scores), 2, 2, None, 0.4, 4, None, p(stats), None) == -1
    assert lib.isc_group_reward(p(scores), 2, 2, None, 0.4, 4, p(reward), None, None) == -1
    for I, n, T in ((4, 1, 4), (4, 0, 4), (0, 2, 4), (-1, 2, 4), (2, 2, 0), (2, -3, 4)):
        assert lib.isc_group_reward(p(scores), I, n, None, 0.4, T, p(reward), p(stats), None) == -2, (I, n, T)
    assert all(x == -7.0 for x in reward) and all(x == -7.0 for x in stats)


# ------------------------------------------------------------------------------------------------ Detector
def _detector():
    from insenticap_model_amd.detector import Detector
    return Detector(synth.make_idx2word(64), 8, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-5}, ST)


def test_detector_rl_samples_per_image_attribute():
    det = _detector()
    assert det.rl_samples_per_image == 1
    for bad in (0, -1, 2.0, 1.5, '3', None, True):
        with pytest.raises(ValueError, match='rl_samples_per_image'):
            det.rl_samples_per_image = bad
        assert det.rl_samples_per_image == 1
    det.rl_samples_per_image = np.int64(5)
    assert det.rl_samples_per_image == 5 and isinstance(det.rl_samples_per_image, int)


def test_detector_rl_samples_per_image_raises_under_a_process_group(monkeypatch):
    """n > 1 with data-parallel training enabled and a process group alive: ValueError before a batch is fetched or
    anything is enqueued (the loaders here would raise on their first use); evaluation keeps the n = 1 path."""
    from insenticap_model_amd import dp

    class NoData:
        def __iter__(self):
            raise AssertionError('a batch was fetched')

        def __len__(self):
            return 1
    det = _detector()
    det.rl_samples_per_image = 3
    det.dp_arena = object()
    monkeypatch.setattr(dp, 'distributed', lambda group=None: True)
    for data_type in ('fact', 'senti'):
        with pytest.raises(ValueError, match='rl_samples_per_image'):
            det((NoData(), NoData()), data_type, True)
