"""The native image-sentiment detector inside the product: Detector.native_sentiment_detector on against off -
Detector.forward('fact', training=False) and Detector.sample - with fp32 features, with float16 features (handed to the
detector as they are) and with one feature value beyond the split-f16 domain.  Tiny shapes of tests/test_detector.py
(V = 64, T = 8, B = 4, a 2x3 grid of 64 channels).  pytest -m gpu.

The region features are the recipe of tests/_senti_det_ref.py (one channel profile per image: the golden batches'
i.i.d. features give every image the same label, and their scores lie within 7e-4 of the threshold), the detector's
weights make_module_weights(shapes, 51, gain=3.0).  Each test first asserts the margin conditions of its features on the
fp64 reference (top-2 probability margin and |score - 0.7| >= 5e-3) and that the labels are not all equal.
With equal labels and replayed draws everything behind the detector runs the same kernels on the same inputs: labels,
captions and the dictionary are compared exactly.  The out-of-domain case runs the flagged batch's iteration on the same
engine in both models too (native off: the captioner's own flag redoes it) - but should the stock path's first attempt
stay unflagged at these tiny widths the engines differ, so its dictionary is held to the tolerance
tests/test_detector.py applies across implementations (rtol 2e-4, atol 2e-5); its labels exactly."""
import os
import warnings

import numpy as np
import pytest
import torch

import _senti_det_ref as R
from insenticap_model_amd import ops, synth
from test_detector import _make_detector, _tensors

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
V, TN, B = 64, 8, 4
ST = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
CASE = dict(R.DEFAULTS, C=64, B=B, h=2, w=3)
FEATURE_SEEDS = (7, 9)


def setup(f16=False, poke=None):
    """(batches with the recipe's region features, the CIDEr split, the detector's weights, fp64 labels per batch)."""
    batches, split = synth.make_rl_batches(2, B, V, ST, seq_len=TN)
    m, w = R.module(CASE)
    out, labels = [], []
    for b, seed in zip(batches, FEATURE_SEEDS):
        f = R.features(CASE, seed)
        if poke is not None and seed == FEATURE_SEEDS[0]:
            f = f.copy()
            f[poke] = 1e5
        if f16:
            f = f.astype(np.float16)
        r = R.forward(w, f.astype(np.float32), 0.7, m.neu_idx)
        top2, tm = R.top2_margin(r['probs']), R.threshold_margin(r['scores'], 0.7)
        assert top2 >= R.MARGIN and tm >= R.MARGIN, 'features %d: margins %.3g / %.3g - change the seed' % (seed, top2, tm)
        assert len(set(r['labels'].tolist())) > 1
        labels.append(r['labels'])
        b = list(b)
        b[2] = f
        out.append(tuple(b))
    return out, split, w, labels


def detector(w, split, native):
    det = _make_detector(DEV)
    det.senti_detector.load_state_dict({k: torch.from_numpy(v).to(DEV) for k, v in w.items()})
    det.set_ciderd_scorer(split)
    assert det.native_sentiment_detector is False
    det.native_sentiment_detector = native
    assert det.senti_detector.native is native
    return det


def forward_eval(det, batches):
    """The eval-mode 'fact' dictionary with the sampled roll-outs' draws replayed from tests/golden/detector.npz, chosen
    by the batch (its fc features) and not by a call count: an iteration that is redone gets its draws again."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'detector.npz'))
    draws = {float(torch.from_numpy(b[1]).sum()): torch.from_numpy(g['det/draws%d' % i]).to(DEV) for i, b in enumerate(batches)}
    assert len(draws) == len(batches)
    orig = det.captioner.forward_rl

    def replay_rl(*a, **k):
        if not k.get('sample_max', a[-1] if len(a) >= 7 else 1):     # Detector passes sample_max by keyword
            k['_replay'] = draws[float(a[0].cpu().sum())]
        return orig(*a, **k)
    det.captioner.forward_rl = replay_rl
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        losses = det(([_tensors(b) for b in batches],), 'fact', False)
    det.captioner.forward_rl = orig
    labels = [det._image_sentiments(b[0], torch.from_numpy(b[2]).to(DEV)).cpu().numpy() for b in batches]   # (the cache)
    return losses, labels


def samples(det, batches):
    out = []
    for b in batches:
        for i in range(B):
            caps, sentis = det.sample(torch.from_numpy(b[1][i]).to(DEV), torch.from_numpy(b[2][i]).to(DEV),
                                      torch.from_numpy(b[5][i]).to(DEV), beam_size=3, decoding_constraint=1)
            out.append((list(caps), list(sentis)))
    return out


@pytest.mark.parametrize('f16', [False, True], ids=['fp32', 'f16'])
def test_native_on_equals_native_off(f16):
    batches, split, w, want = setup(f16=f16)
    off, on = detector(w, split, False), detector(w, split, True)
    l_off, lab_off = forward_eval(off, batches)
    before = ops.senti_det_launches()
    l_on, lab_on = forward_eval(on, batches)
    d = ops.senti_det_launches()
    assert d['tail'] - before['tail'] == 2              # one native call per batch; the second look hit the label cache
    assert d['f16'] - before['f16'] == (2 if f16 else 0)
    for a, b, c in zip(lab_off, lab_on, want):
        assert np.array_equal(a, c) and np.array_equal(b, c)
    assert set(l_on) == set(l_off) == {'da_loss', 'fact_reward', 'cls_reward', 'all_rewards', 'cap_loss', 'xe_loss'}
    for k in l_off:
        assert l_on[k] == l_off[k], (k, l_on[k], l_off[k])
    s_off = samples(off, batches)
    before = ops.senti_det_launches()['tail']
    s_on = samples(on, batches)
    assert ops.senti_det_launches()['tail'] - before == 2 * B
    assert s_on == s_off
    cats = on.senti_detector.sentiment_categories
    assert [s[1][0] for s in s_on] == [cats[i] for lab in want for i in lab]


def test_a_feature_beyond_the_split_f16_domain_is_served_like_native_off():
    batches, split, w, want = setup(poke=(1, 0, 1, 5))
    off, on = detector(w, split, False), detector(w, split, True)
    l_off, lab_off = forward_eval(off, batches)
    l_on, lab_on = forward_eval(on, batches)
    for a, b, c in zip(lab_off, lab_on, want):          # (the cache holds the recomputed labels, not `neutral`)
        assert np.array_equal(a, c) and np.array_equal(b, c)
    assert set(l_on) == set(l_off)
    for k in l_off:
        np.testing.assert_allclose(l_on[k], l_off[k], rtol=2e-4, atol=2e-5, err_msg=k)
    ops.device_status(reset=True)
