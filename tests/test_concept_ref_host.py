"""tests/_concept_ref.py (the fp64 numpy restatement every concept kernel is held to) against the fixture the reference
wrote (tests/golden/concept.npz, made by tests/golden/make_concept_golden.py from the unmodified ConceptDetector,
MultiLabelClsLoss and concept collate).  The reference computes in fp32; tolerances are a few fp32 roundings of the
largest element.  The sentiment-word aggregation has no recorded reference output (preprocess.py cannot be imported where
the fixture is made - nltk, skimage): `senti_words` is a hand restatement of preprocess.py:288-301, checked here against
values worked out by hand."""
import numpy as np

import _concept_ref as R


def _params(g, prefix='sd/'):
    return {k: g[prefix + k] for k in R.NAMES}


def test_forward_and_topk_equal_the_reference(golden):
    g = golden('concept')
    f = R.forward(_params(g), g['feats'])
    assert np.abs(f['probs'] - g['probs']).max() <= 4 * 2.0 ** -23
    num = int(g['hyper'][2])
    assert np.array_equal(R.topk(f['logits'], num), g['sample_idx'])
    picked = np.take_along_axis(f['probs'], g['sample_idx'], axis=1)
    assert np.abs(picked - g['sample_scores']).max() <= 4 * 2.0 ** -23


def test_topk_ordering_rule():
    z = np.array([[1.0, 1.0, 1.0, 1.0],
                  [0.0, -0.0, 0.0, -1.0],
                  [np.nan, -np.inf, np.inf, 5.0],
                  [np.nan, np.nan, -np.inf, -np.inf]], dtype=np.float32)
    assert R.topk(z, 4).tolist() == [[0, 1, 2, 3], [0, 1, 2, 3], [2, 3, 1, 0], [2, 3, 0, 1]]
    assert R.topk_gap(np.array([[3.0, 1.0, 2.5, 0.0]]), 2) == 0.5


def test_loss_gradients_and_two_steps_equal_the_reference(golden):
    g = golden('concept')
    lr, clip = float(g['hyper'][0]), float(g['hyper'][1])
    feats, targets = g['feats'], g['targets']
    after, losses, grads = R.adam_steps(_params(g), lambda p: R.backward(p, feats, targets), 2, lr, clip)
    for it in range(2):
        assert abs(losses[it] - g['loss'][it]) <= 4 * 2.0 ** -23 * g['loss'][it]
        for k in R.NAMES:
            ref = g['grad%d/%s' % (it + 1, k)]
            # iteration 2 starts from each side's own weights after an Adam step of +-lr per element: 1e-3 of the largest
            assert np.abs(grads[it][k] - ref).max() <= (1e-5 if it == 0 else 1e-3) * np.abs(ref).max() + 1e-9, (it, k)
    for k in R.NAMES:
        d = np.abs(after[k] - g['after2/' + k])
        assert d.max() <= 4 * lr * 1.01 and np.median(d) <= lr / 40, k


def test_loss_is_the_reference_formula_and_finite_where_it_is_not():
    rng = np.random.default_rng(3)
    z = rng.normal(size=(4, 9)) * 3
    t = rng.integers(0, 2, size=(4, 9))
    s = R.sigmoid(z)
    t1, t2, L, dz = R.loss(z, t)
    assert abs(t1 + np.mean(t * np.log(s))) < 1e-14 and abs(t2 + np.mean((1 - t) * np.log(1 - s))) < 1e-14
    eps = 1e-6
    zp = z.copy()
    zp[1, 2] += eps
    assert abs((R.loss(zp, t)[2] - L) / eps - dz[1, 2]) < 1e-8
    big = np.array([[800.0, -800.0, 40.0, -40.0]])
    for tt in ([[1, 1, 1, 1]], [[0, 0, 0, 0]]):
        assert all(np.isfinite(x) for x in R.loss(big, tt)[:3]) and np.isfinite(R.loss(big, tt)[3]).all()


def test_hits_counts():
    t = np.array([[1, 0, 1, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]])
    h, n = R.hits(np.array([[0, 1], [2, 3], [4, 0]]), t)
    assert h.tolist() == [1, 0, 2] and n.tolist() == [2, 0, 5]


def test_senti_words_by_hand():
    """preprocess.py:288-301 worked out by hand: concept 0 -> (7, .5) (8, .25); 1 -> nothing; 2 -> (8, .25) (7, .1) (9, .5)."""
    lists = [[(7, 0.5), (8, 0.25)], [], [(8, 0.25), (7, 0.1), (9, 0.5)]]
    # image 0: sums 7: .6, 8: .5, 9: .5 -> 7, then the tie in first-occurrence order 8, 9; image 1: nothing; image 2:
    # concept order (2, 0): 8: .5, 7: .6, 9: .5 -> 7, 8, 9; image 3: out-of-range and empty concepts only
    out = R.senti_words([[0, 2], [1, 1], [2, 0], [5, 1]], lists, 4, 0)
    assert out.tolist() == [[7, 8, 9, 0], [0, 0, 0, 0], [7, 8, 9, 0], [0, 0, 0, 0]]
    assert R.senti_words([[2]], lists, 2, 99).tolist() == [[9, 8]]          # .25, .1, .5 -> 9, 8, 7, cut to 2
