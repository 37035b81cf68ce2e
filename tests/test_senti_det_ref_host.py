"""tests/_senti_det_ref.py - the fp64 restatement the GPU tests of the native image-sentiment detector compare with -
checked on the CPU: against the reference project's own outputs (tests/golden/detector.npz), against the stock module in
double precision, for the margin conditions of every GPU case, for the exactness guarantee of the lattice case, and for
whether the GPU tests' comparison notices a wrong reference."""
import numpy as np
import pytest
import torch

import _senti_det_ref as R
from insenticap_model_amd import synth

ST = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
LATTICE_CASES = ('baseline', 'grid_2x3', 'grid_1x1', 'grid_1x5', 'grid_5x1', 'c256_3x3', 'c128_14x14', 'one_image', 'product')


def golden_setup():
    """The golden file's detector: weights make_module_weights(shapes, 51) at the default gain, the att features of
    synth.make_rl_batches(2, 4, 64, ...) - a 2x3 grid of 64 channels - threshold 0.7 (tests/test_detector.py)."""
    c = dict(R.DEFAULTS, C=64, B=4, h=2, w=3)
    m, w = R.module(c, gain=2.0)
    batches, _ = synth.make_rl_batches(2, 4, 64, ST, seq_len=8)
    return c, m, w, [np.ascontiguousarray(b[2], dtype=np.float32) for b in batches]


def test_reference_equals_the_golden_file(golden):
    g = golden('detector')
    c, m, w, feats = golden_setup()
    for i, f in enumerate(feats):
        assert f.shape == (4, 2, 3, 64)
        r = R.forward(w, f, 0.7, m.neu_idx)
        assert np.array_equal(r['labels'], g['senti_det/labels%d' % i])
        np.testing.assert_allclose(r['scores'], g['senti_det/scores%d' % i], atol=1e-5)
        np.testing.assert_allclose(r['maps'], g['senti_det/maps%d' % i], atol=1e-4)
        np.testing.assert_allclose(r['logits'], g['senti_det/logits%d' % i], atol=1e-4)


@pytest.mark.parametrize('name', ['baseline', 'grid_1x5', 'convs_3', 'fcs_0', 'k_8', 'thr_2'])
def test_reference_equals_the_stock_module_in_double_precision(name):
    c = R.case(name)
    m, w = R.module(c)
    feats = R.features(c)
    r = R.forward(w, feats, c['threshold'], m.neu_idx)
    s = R.stock_outputs(m.double(), feats, c['threshold'])
    for k in R.VALUE_KEYS:
        assert np.abs(s[k] - r[k]).max() <= 1e-12 * max(1.0, np.abs(r[k]).max()), k
    assert np.array_equal(s['labels'], r['labels'])


@pytest.mark.parametrize('name', list(R.CASES))
def test_every_gpu_case_meets_its_margin_conditions(name):
    c = R.reference(name)
    r, thr = c['ref'], c['c']['threshold']
    top2, tm = R.top2_margin(r['probs']), R.threshold_margin(r['scores'], thr)
    counts = np.bincount(r['labels'], minlength=c['c']['k']).tolist()
    print('%s: labels %s  rows under threshold %d  top-2 margin %.4f  threshold margin %.4f'
          % (name, counts, int((r['scores'] < thr).sum()), top2, tm))
    assert top2 >= R.MARGIN and tm >= R.MARGIN, (name, top2, tm)
    if name == 'baseline':
        assert sum(1 for n in counts if n) >= 2 and (r['scores'] < thr).any() and (r['scores'] > thr).any()
    if name == 'k_8':
        assert sum(1 for n in np.bincount(r['probs'].argmax(-1), minlength=8) if n) >= 4
    if name == 'k_2':
        assert all(np.bincount(r['probs'].argmax(-1), minlength=2))
    if name == 'thr_2':
        assert (r['labels'] == c['neu_idx']).all()
    # the stock fp32 module itself decides every row as the fp64 reference does
    assert np.array_equal(c['stock']['labels'], r['labels'])


@pytest.mark.parametrize('name', LATTICE_CASES)
def test_lattice_case_is_exact_by_construction(name):
    c = R.case(name)
    w, feats = R.lattice_operands(c)
    r32 = R.lattice_expect(w, feats)                    # asserts the guarantee from the operands
    assert (r32 > 0).any() and (r32 == 0).any()
    # and the stock fp32 module, whatever its summation order, lands on the same bits
    m, _ = R.module(c, weights=w)
    s = R.stock_outputs(m, feats, 0.7)
    assert np.array_equal(s['conv_out'], r32.astype(np.float64))


@pytest.mark.parametrize('inject', R.INJECTIONS)
def test_the_comparison_notices_a_wrong_reference(inject):
    """The right values (the fp64 reference itself, rounded to fp32 - what a faultless kernel would hand back) against a
    reference with one error injected: the GPU tests' comparison must raise.  And on the right reference it passes."""
    c = R.reference('baseline')
    got = {k: v.astype(np.float32) if v.dtype == np.float64 else v for k, v in c['ref'].items()}
    R.compare(got, c['ref'], c['e'], 'baseline')
    wrong = R.forward(c['w'], c['feats'], c['c']['threshold'], c['neu_idx'], inject=inject)
    with pytest.raises(AssertionError):
        R.compare(got, wrong, c['e'], inject, keys=('conv_out', 'logits', 'maps', 'scores'), labels=False)
    if inject in ('tap_transposed', 'border_not_zeroed'):
        # ... and so must the lattice case's bit comparison
        lc = R.case('baseline')
        w, feats = R.lattice_operands(lc)
        r32 = R.lattice_expect(w, feats)
        bad = R.forward(w, feats, 0.7, 2, inject=inject)['conv_out']
        assert not np.array_equal(bad, r32.astype(np.float64))
