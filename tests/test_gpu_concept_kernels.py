"""Each kernel of csrc/concept.hip alone, at its edge shapes, against the fp64 restatement (tests/_concept_ref.py).

Indices, words, hits, counts and sentiment-word ids are exact.  Scores, probabilities, loss terms and dz are held to the
project's yardstick (tests/test_gpu_sent_cls.py): |native - fp64| <= 4 max(e, 2^-23 max|fp64|), e = the error of the
same formula evaluated by torch in fp32 on the CPU against fp64, computed here.  The head orders by the LOGITS it is
handed, so its expected indices come from the rule applied to those very fp32 values - no margin is involved."""
import numpy as np
import pytest
import torch

import _concept_ref as R
from insenticap_model_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _check(name, got, ref64, e):
    err, bound = R.yardstick(got, ref64, e)
    print('%s: native err %.3g  torch-fp32-cpu err %.3g  bound %.3g' % (name, err, e, bound))
    assert err <= bound, (name, err, bound)


def _sig_e(z32):
    """fp64 sigmoid of the fp32 logits and the error of torch's fp32 CPU sigmoid against it (non-finite logits left out)."""
    ref = R.sigmoid(z32)
    cpu = torch.sigmoid(torch.from_numpy(z32)).double().numpy()
    ok = np.isfinite(ref) & np.isfinite(z32)
    return ref, float(np.abs(cpu - ref)[ok].max()) if ok.any() else 0.0


def _head_expect(z32, num, table, targets):
    idx = R.topk(z32, num)
    h, n = R.hits(idx, targets)
    return idx, table[idx], h, n


# ------------------------------------------------------------------ head
@pytest.mark.parametrize('B,C,num', [(1, 1, 1), (3, 5, 5), (65, 64, 1), (2, 65, 16), (7, 2000, 5), (130, 2001, 5)])
def test_head_shapes(B, C, num):
    rng = np.random.default_rng(B * 7919 + C)
    z = (rng.normal(size=(B, C)) * 3).astype(np.float32)
    table = (np.arange(C, dtype=np.int64) * 3 + 7)
    targets = (rng.random((B, C)) < 0.3).astype(np.uint8)
    idx, words, h, n = _head_expect(z, num, table, targets)
    zd, td = torch.from_numpy(z).to(DEV), torch.from_numpy(targets).to(DEV)
    out = ops.concept_head(zd, num, torch.from_numpy(table).to(DEV), td)
    again = ops.concept_head(zd, num, torch.from_numpy(table).to(DEV), td.to(torch.int64))
    assert np.array_equal(out['idx'].cpu().numpy(), idx) and np.array_equal(out['words'].cpu().numpy(), words)
    assert out['hits'].dtype == torch.int32 and np.array_equal(out['hits'].cpu().numpy(), h)
    assert np.array_equal(out['n_true'].cpu().numpy(), n)
    ref, e = _sig_e(z)
    _check('probs', out['probs'].cpu().numpy(), ref, e)
    _check('scores', out['scores'].cpu().numpy(), np.take_along_axis(ref, idx, axis=1), e)
    assert torch.equal(out['scores'], torch.gather(out['probs'], 1, out['idx']))
    for k in out:                                           # two runs (uint8 against int64 targets): the same bits
        assert torch.equal(out[k], again[k]), k


def test_head_ordering_rule():
    """All-equal logits -> 0 .. num-1; equal values across the lane boundary (63, 64); both infinities; -0.0 against +0.0;
    NaN below every number."""
    C, num = 130, 6
    z = np.full((6, C), -2.0, dtype=np.float32)
    z[0, :] = 0.25                                           # all equal
    z[1, 63] = z[1, 64] = 5.0                                # a tie across lanes 63 | 0 of the next stride
    z[1, 129] = 5.0
    z[2, 7], z[2, 100], z[2, 3] = np.inf, -np.inf, 9.0       # +inf first; -inf last of all
    z[3, :] = -1.0
    z[3, 70], z[3, 5], z[3, 64] = -0.0, 0.0, 0.0             # -0.0 == +0.0: index order 5, 64, 70
    z[4, :] = np.nan
    z[4, 90], z[4, 10] = -np.inf, -1e30                      # every number, also -inf, ranks above NaN
    z[5, 2] = np.nan                                         # one NaN among numbers: last
    exp = R.topk(z, num)
    assert exp[0].tolist() == [0, 1, 2, 3, 4, 5] and exp[1].tolist()[:3] == [63, 64, 129]
    assert exp[2].tolist()[:2] == [7, 3] and exp[3].tolist()[:3] == [5, 64, 70] and exp[4].tolist()[:4] == [10, 90, 0, 1]
    zd = torch.from_numpy(z).to(DEV)
    ops.register_status_words()
    torch.cuda.synchronize()
    ops.device_status(reset=True)
    ops.concept_head(zd[:4], num)                            # rows without a NaN (the infinities are ordinary values) ...
    torch.cuda.synchronize()
    assert ops.device_status(reset=True) == 0                # ... raise nothing
    out = ops.concept_head(zd, num)
    assert np.array_equal(out['idx'].cpu().numpy(), exp)     # (the read-back waits for the kernel)
    assert ops.device_status(reset=True) & ops.STATUS_NONFINITE_STATS      # a NaN logit raises the numerics status word
    full = ops.concept_head(zd[:, :16].contiguous(), 16, want=('idx',))['idx'].cpu().numpy()
    assert np.array_equal(full, R.topk(z[:, :16], 16))       # num == C: -inf and the NaN come last
    assert int(R.topk(z[2:3], C)[0, -1]) == 100 and int(R.topk(z[5:6], C)[0, -1]) == 2
    torch.cuda.synchronize()
    ops.device_status(reset=True)                            # (rows 4 and 5 again: leave the words clean)
    sc = out['scores'].cpu().numpy()
    assert sc[2, 0] == 1.0 and abs(sc[0, 0] - R.sigmoid(0.25)) <= 4 * 2.0 ** -23
    assert np.isnan(sc[4, 2]) and out['probs'].cpu().numpy()[2, 100] == 0.0


def test_head_strided_rows_and_optional_outputs():
    rng = np.random.default_rng(11)
    B, C, num = 9, 77, 4
    big = (rng.normal(size=(B, C + 12)) * 2).astype(np.float32)
    view = torch.from_numpy(big).to(DEV)[:, :C]
    assert view.stride(0) == C + 12
    table = torch.arange(C, dtype=torch.int64, device=DEV) + 1000
    targets = torch.from_numpy((rng.random((B, C)) < 0.5).astype(np.int64)).to(DEV)
    ref = ops.concept_head(view.contiguous(), num, table, targets)
    got = ops.concept_head(view, num, table, targets)
    for k in ref:
        assert torch.equal(ref[k], got[k]), k
    assert np.array_equal(got['idx'].cpu().numpy(), R.topk(big[:, :C], num))
    names = ('probs', 'idx', 'scores', 'words', 'hits')
    for leave in names:                                      # every optional output null in turn
        want = tuple(n for n in names if n != leave)
        part = ops.concept_head(view, num, table, targets, want=want)
        assert leave not in part and (leave != 'hits' or 'n_true' not in part)
        for k in part:
            assert torch.equal(part[k], ref[k]), (leave, k)
    only = ops.concept_head(view, num, want=('idx',))
    assert list(only) == ['idx'] and torch.equal(only['idx'], ref['idx'])


def test_head_hits_and_counts():
    rng = np.random.default_rng(12)
    B, C, num = 6, 70, 5
    z = rng.normal(size=(B, C)).astype(np.float32)
    zd = torch.from_numpy(z).to(DEV)
    idx = R.topk(z, num)
    for fill, h_exp, n_exp in ((0, 0, 0), (1, num, C)):      # all-zero and all-one targets
        t = torch.full((B, C), fill, dtype=torch.uint8, device=DEV)
        out = ops.concept_head(zd, num, targets=t, want=('hits',))
        assert out['hits'].tolist() == [h_exp] * B and out['n_true'].tolist() == [n_exp] * B
    # ground truth given as id lists with duplicates (the collate's `cpts[ids] = 1` makes a set of them)
    gt = [[int(idx[b, 0]), int(idx[b, 0]), int(idx[b, 2]), (int(idx[b, 0]) + 1) % C, (int(idx[b, 0]) + 1) % C]
          for b in range(B)]
    t = np.zeros((B, C), dtype=np.int64)
    for b, ids in enumerate(gt):
        t[b, ids] = 7                                        # any non-zero value counts as set
    h, n = R.hits(idx, t)
    assert all(int(n[b]) == len(set(gt[b])) for b in range(B))
    out = ops.concept_head(zd, num, targets=torch.from_numpy(t).to(DEV), want=('hits',))
    assert out['hits'].tolist() == h.tolist() == [len(set(gt[b]) & set(idx[b].tolist())) for b in range(B)]
    assert out['n_true'].tolist() == n.tolist()


def test_head_shape_limits():
    z = torch.zeros(2, 20, device=DEV)
    for bad in (0, 17, 21, -3):
        with pytest.raises(ValueError):
            ops.concept_head(z, bad)
    with pytest.raises(ValueError):
        ops.concept_head(z[:, :4].contiguous(), 5)


# ------------------------------------------------------------------ loss
def _loss_case(B, C, scale, targets):
    rng = np.random.default_rng(B * 31 + C)
    z = rng.uniform(-1.0, 1.0, size=(B, C)).astype(np.float32) * np.float32(scale)
    if targets == 'rand':
        t = (rng.random((B, C)) < 0.4).astype(np.uint8)
    else:
        t = np.full((B, C), targets, dtype=np.uint8)
    return z, t


def _loss_e(z, t):
    """The stable formula in fp32 on the CPU (torch) against fp64: the error scale of each output."""
    zt, tt = torch.from_numpy(z), torch.from_numpy(t).float()
    sp = torch.nn.functional.softplus
    n = z.size
    t1, t2 = (tt * sp(-zt)).sum() / n, ((1 - tt) * sp(zt)).sum() / n
    dz = (torch.sigmoid(zt) - tt) / n
    r1, r2, rl, rdz = R.loss(z, t)
    return (r1, r2, rl, rdz), (abs(float(t1) - r1), abs(float(t2) - r2), abs(float(t1 + t2) - rl),
                               float(np.abs(dz.double().numpy() - rdz).max()))


@pytest.mark.parametrize('B,C', [(1, 4), (3, 68), (80, 2000)])
@pytest.mark.parametrize('scale,targets', [(3.0, 'rand'), (30.0, 'rand'), (30.0, 0), (30.0, 1)])
def test_loss(B, C, scale, targets):
    z, t = _loss_case(B, C, scale, targets)
    ref, e = _loss_e(z, t)
    zd = torch.from_numpy(z).to(DEV)
    out3, dz = ops.concept_loss(zd, torch.from_numpy(t).to(DEV), want_dz=True)
    out3_64, dz_64 = ops.concept_loss(zd, torch.from_numpy(t.astype(np.int64)).to(DEV), want_dz=True)
    none3, none_dz = ops.concept_loss(zd, torch.from_numpy(t).to(DEV))
    got = out3.cpu().numpy()
    assert np.isfinite(got).all() and torch.isfinite(dz).all()
    for i, name in enumerate(('term1', 'term2', 'loss')):
        _check('%s B=%d C=%d scale=%g' % (name, B, C, scale), got[i:i + 1], np.asarray([ref[i]]), e[i])
    _check('dz', dz.cpu().numpy(), ref[3], e[3])
    assert torch.equal(out3, out3_64) and torch.equal(dz, dz_64)          # uint8 against int64 targets: the same bits
    assert none_dz is None and torch.equal(none3, out3)                    # ... and with or without dz


def test_loss_gradient_scale_and_strided_logits():
    z, t = _loss_case(5, 36, 4.0, 'rand')
    big = np.zeros((5, 40), dtype=np.float32)
    big[:, :36] = z
    view = torch.from_numpy(big).to(DEV)[:, :36]
    td = torch.from_numpy(t).to(DEV)
    a3, adz = ops.concept_loss(torch.from_numpy(z).to(DEV), td, want_dz=True)
    b3, bdz = ops.concept_loss(view, td, want_dz=True)
    assert torch.equal(a3, b3) and torch.equal(adz, bdz)
    _, dz2 = ops.concept_loss(view, td, g=2.0, want_dz=True)
    assert torch.equal(dz2, adz * 2)                         # g / (B C) doubles exactly


# ------------------------------------------------------------------ sentiment words
def _table(lists, device=DEV):
    off, word, score = [0], [], []
    for lst in lists:
        for w, s in lst:
            word.append(w)
            score.append(s)
        off.append(len(word))
    return (torch.tensor(off, dtype=torch.int32, device=device), torch.tensor(word, dtype=torch.int64, device=device),
            torch.tensor(score, dtype=torch.float64, device=device), max(len(x) for x in lists))


def _run_words(idx, lists, n_out, pad_id):
    off, word, score, longest = _table(lists)
    got = ops.senti_words_from_concepts(torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(DEV), off, word, score,
                                        longest, n_out, pad_id)
    again = ops.senti_words_from_concepts(torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(DEV), off, word, score,
                                          longest, n_out, pad_id)
    assert torch.equal(got, again)
    return got.cpu().numpy()


@pytest.mark.parametrize('n_out', [1, 10, 20])
@pytest.mark.parametrize('num', [1, 5])
def test_senti_words_vs_host(n_out, num):
    rng = np.random.default_rng(100 + n_out + num)
    C = 40
    lists = []
    for c in range(C):
        if c % 5 == 0:
            lists.append([])                                 # concepts with empty lists
            continue
        n = int(rng.integers(1, 30))
        # scores that do not add exactly (the order of the float64 sums matters) mixed with dyadic ones (exact ties)
        lists.append([(int(rng.integers(4, 60)), float(rng.random()) if rng.random() < 0.5 else float(rng.integers(1, 4)) / 4)
                      for _ in range(n)])
    B = 70
    idx = rng.integers(0, C, size=(B, num))
    idx[0, :] = 0                                            # an image whose concepts have no entry at all
    idx[1, :] = 5 if num == 1 else [0, 5, 10, 15, 20]        # only empty lists
    if num == 5:
        idx[2, :] = [3, 3, 3, 3, 3]                          # one concept five times: every word summed five times
        idx[3, :] = [C + 3, -1, 7, 8, 9]                     # indices outside the table contribute nothing
    ref = R.senti_words(idx, lists, n_out, 0)
    assert (ref[0] == 0).all() and (ref[1] == 0).all()
    got = _run_words(idx, lists, n_out, 0)
    assert got.dtype == np.int64 and np.array_equal(got, ref)
    assert np.array_equal(_run_words(idx[:3], lists, n_out, -7), R.senti_words(idx[:3], lists, n_out, -7))


def test_senti_words_sums_ties_and_overflow_of_n_out():
    lists = [[(7, 0.5), (8, 0.25)], [], [(8, 0.25), (7, 0.1), (9, 0.5)],
             [(20 + i, 1.0) for i in range(30)],                        # 30 exact ties: first-occurrence order
             [(11, 0.1), (12, 0.2), (11, 0.2), (12, 0.1)]]              # .1 + .2 against .2 + .1: not a tie in float64?
    idx = [[0, 2, 1], [2, 0, 1], [3, 3, 0], [4, 1, 1], [1, 1, 1]]
    ref = R.senti_words(idx, lists, 20, 0)
    assert ref[0, :4].tolist() == [7, 8, 9, 0] and ref[2, :20].tolist() == [20 + i for i in range(20)]
    assert np.array_equal(_run_words(idx, lists, 20, 0), ref)
    assert np.array_equal(_run_words(idx, lists, 3, 0), R.senti_words(idx, lists, 3, 0))


def test_senti_words_at_the_cap_and_beyond():
    cap = ops.SENTI_WORDS_CAP
    rng = np.random.default_rng(9)
    per = cap // 4
    lists = [[(int(rng.integers(4, 500)), float(rng.random())) for _ in range(per)] for _ in range(4)] + [[]]
    idx = [[0, 1, 2, 3], [3, 3, 3, 3], [4, 4, 4, 4], [2, 4, 0, 4]]           # image 0 and 1: exactly cap candidates
    ref = R.senti_words(idx, lists, 20, 0)
    assert np.array_equal(_run_words(idx, lists, 20, 0), ref)
    off, word, score, longest = _table(lists)
    with pytest.raises(ValueError):                          # five concepts of this table would exceed the cap: refused
        ops.senti_words_from_concepts(torch.zeros(1, 5, dtype=torch.int64, device=DEV), off, word, score, longest, 20, 0)
    with pytest.raises(ValueError):
        ops.senti_words_from_concepts(torch.zeros(1, 4, dtype=torch.int64, device=DEV), off, word, score, longest, 21, 0)
