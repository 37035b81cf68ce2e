"""CPU checks of what the GPU tests of the image-sentiment detector's training rest on: the fp64 restatement
(tests/_senti_det_train_ref.py) against double-precision torch autograd of helper_nets.SentimentDetector and against the
reference's fixture, and every case's input condition (tests/_senti_det_train_cases.py)."""
import os

import numpy as np
import pytest
import torch

import _senti_det_train_cases as Cs
import _senti_det_train_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'senti_det_train.npz')
ALL = list(Cs.CASES) + list(Cs.MASKED) + list(Cs.TINY)


@pytest.mark.parametrize('name', ALL)
def test_restatement_vs_double_precision_autograd(name):
    c = Cs.reference(name)
    m = Cs.module(c['c'], c['p'], weights=c['w'])[0].double()
    m.zero_grad()
    loss = R.torch_loss(m, c['feats'], c['labels'], c['keep'], c['p'], c['scale'])
    loss.backward()
    assert abs(float(loss.detach()) - c['loss']) <= 1e-12 * abs(c['loss'])
    assert [n for n, _ in m.named_parameters()] == c['names']
    for n, q in m.named_parameters():
        ref = c['grads'][n]
        assert ref.shape == tuple(q.shape)
        assert np.abs(q.grad.numpy() - ref).max() <= 1e-12 * np.abs(ref).max(), n
    # the saved quantities the device tests read
    x = torch.from_numpy(np.array(c['feats'])).double()
    if c['keep'] is None:
        logits, maps = m(x)
        assert np.abs(logits.detach().numpy() - c['aux']['logits']).max() <= 1e-12 * np.abs(c['aux']['logits']).max()
        assert np.abs(maps.detach().numpy() - c['aux']['maps']).max() <= 1e-12 * np.abs(c['aux']['maps']).max()


@pytest.mark.parametrize('name', ALL)
def test_input_conditions(name):
    c = Cs.reference(name)
    cc, seed = Cs.case(name)
    assert R.relu_margin(c['aux']) >= 1e-5
    w = c['w']
    first = R.find_seed(lambda s: R.forward_backward(w, *Cs.inputs(cc, s), keep=c['keep'], dropout_p=c['p'],
                                                     scale=c['scale'])[2])
    assert first == seed                                        # the constant is the first seed >= 7 that meets it
    if c['keep'] is not None:
        assert c['keep'][0].all() and 0.3 < c['keep'][1:].mean() < 0.7
    assert len(set(c['labels'].tolist())) > 1 or cc['B'] == 1
    if name in Cs.TINY:                                         # the tiny-gradient condition
        for d in c['aux']['dx']:
            assert np.abs(d).max() < 2.0 ** -24
        assert len(c['aux']['dx']) == 2
        assert all(np.abs(g).max() > 0 for g in c['grads'].values())
    elif name in Cs.CASES:                                      # ... and the plain cases are not tiny by accident
        assert np.abs(c['aux']['dx'][-1]).max() > 2.0 ** -14


def test_restatement_vs_the_references_fixture():
    """Iteration 1 of the fixture: the reference's own module gave its loss and its ten gradients in fp32 - the fp64
    restatement stands within fp32's rounding of them (1e-6 of the loss, 1e-5 of each gradient's largest element)."""
    g = np.load(GOLDEN)
    names = R.names(2, 2)
    w = {n: g['sd/' + n] for n in names}
    L64, G64, aux = R.forward_backward(w, g['feats'], g['labels'])
    assert R.relu_margin(aux) >= 1e-5
    assert abs(L64 - g['loss'][0]) <= 1e-6 * g['loss'][0]
    for n in names:
        ref = g['grad1/' + n]
        assert np.abs(G64[n] - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-9, n
    # the fixture's inputs are the cases' draw at its recorded seed
    feats, labels = Cs.inputs(dict(Cs.DEFAULTS, C=64, h=5, w=5, B=6), int(g['seed'][0]))
    assert np.array_equal(feats, g['feats']) and np.array_equal(labels, g['labels'])


def test_flipped_weights_give_the_transposed_convolution():
    """conv3x3(dY, W') with W'[ci,co,ky,kx] = W[co,ci,2-ky,2-kx] equals torch's conv_transpose2d(dY, W, padding=1)."""
    import _senti_det_ref as S
    rng = np.random.default_rng(2)
    W = rng.standard_normal((6, 4, 3, 3))
    dy = rng.standard_normal((2, 3, 5, 6))
    got = S.conv3x3(dy, R.flipped(W), 0.0)
    ref = torch.nn.functional.conv_transpose2d(torch.from_numpy(dy).permute(0, 3, 1, 2), torch.from_numpy(W), padding=1)
    assert np.abs(got - ref.permute(0, 2, 3, 1).numpy()).max() <= 1e-12
