"""Self-critical RL on n sampled captions per image without repeating the image: isc_group_reward against the numpy
reference (tests/_group_reward_ref.py), the differentiable grouped sampled roll-out
(`forward_rl(..., sample_max=0, captions_per_image=n)` in training mode) against the float64 oracle on the expanded inputs
and against this build's own repeated call, and `Detector.rl_samples_per_image`.

End-to-end bars: those of tests/test_gpu_backward.py / tests/test_gpu_group_backward.py."""
import numpy as np
import pytest
import torch

import _group_reward_ref as GR
from insenticap_model_amd import Captioner, RewardCriterion, _lib, ops, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GRAD_RTOL = 1e-4   # gradients within 1e-4 relative to the tensor's max
SENT = -7.0


# ------------------------------------------------------------------------------------------------ isc_group_reward
@pytest.mark.parametrize('with_cls', [False, True], ids=['scores_only', 'with_classifier_term'])
@pytest.mark.parametrize('I,n,T', [(1, 2, 1), (3, 5, 8), (2, 8, 20), (5, 3, 17), (300, 5, 20)])
def test_group_reward_kernel_vs_the_reference(I, n, T, with_cls):
    """Scores with ties inside an image, zeros and values up to 10.  Without the classifier term the reward equals the
    reference bit for bit (the same fp64 operations in the same order, rounded once to fp32); with it, within 1 fp32 ulp
    (the kernel does not contract the multiply-add: measured on an MI355X it is bit-equal there too).  Each stats4 entry
    within N * 2^-53 * sum|x| of the reference's, the bound computed from the inputs; two runs give the same bits; the
    sentinel row behind the output stays."""
    rng = np.random.default_rng(I * 100 + n * 10 + T)
    scores = GR.make_scores(I, n, seed=I + n + T)
    rows = I * n
    cls = rng.random((rows, T)).astype(np.float32) * (rng.random((rows, 1)) > 0.4) if with_cls else None
    if cls is not None:
        cls = np.ascontiguousarray(cls, dtype=np.float32)
    adv, ref, ref_stats = GR.group_reward(scores, n, T, cls, 0.4)
    sd = torch.from_numpy(scores).to(DEV)
    cd = None if cls is None else torch.from_numpy(cls).to(DEV)
    runs = []
    for _ in range(2):
        big = torch.full((rows + 1, T), SENT, dtype=torch.float32, device=DEV)
        st = torch.full((5,), SENT, dtype=torch.float64, device=DEV)
        rw, s4 = ops.group_reward(sd, n, cd, 0.4, T, reward=big[:rows], stats4=st[:4])
        torch.cuda.synchronize()
        assert bool((big[rows:] == SENT).all()) and float(st[4]) == SENT
        runs.append((rw.cpu().numpy().copy(), s4.cpu().numpy().copy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    got, got_stats = runs[0]
    n_diff = int((got != ref).sum())
    print('GROUPREWARD [%dx%dx%d cls=%d] reward entries that differ from the reference: %d; stats %s ref %s'
          % (I, n, T, with_cls, n_diff, got_stats.tolist(), ref_stats.tolist()))
    if not with_cls:
        assert np.array_equal(got, ref)
    else:
        ulp = np.spacing(np.abs(ref).astype(np.float32))
        assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= ulp.astype(np.float64)).all()
    bounds = GR.stats_bounds(scores, adv, got, cls)
    for k in range(4):
        assert abs(got_stats[k] - ref_stats[k]) <= bounds[k], (k, got_stats[k], ref_stats[k], bounds[k])
    assert with_cls or got_stats[2] == 0.0


def test_group_reward_kernel_refuses_shapes_and_leaves_the_outputs_alone():
    lib = _lib.load()
    scores = torch.ones(8, dtype=torch.float64, device=DEV)
    reward = torch.full((8, 4), SENT, dtype=torch.float32, device=DEV)
    stats = torch.full((4,), SENT, dtype=torch.float64, device=DEV)
    for I, n, T in ((8, 1, 4), (8, 0, 4), (0, 2, 4), (-2, 2, 4), (4, 2, 0), (4, 2, -1)):
        rc = lib.isc_group_reward(scores.data_ptr(), I, n, None, 0.4, T, reward.data_ptr(), stats.data_ptr(), ops.stream())
        assert rc == -2, (I, n, T)
    with pytest.raises(_lib.HipLibraryError):
        ops.group_reward(scores, 1, None, 0.4, 4, reward=reward, stats4=stats)
    torch.cuda.synchronize()
    assert bool((reward == SENT).all()) and bool((stats == SENT).all())
    assert lib.isc_group_reward(scores.data_ptr(), 4, 2, None, 0.4, 4, reward.data_ptr(), stats.data_ptr(), ops.stream()) == 0
    torch.cuda.synchronize()
    assert bool((reward == 0).all()) and stats.tolist() == [1.0, 0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------ the grouped roll-out
def _captioner(w, V, st, p_drop):
    """Training mode; p_drop = 0: dropout off."""
    cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, dict(st, dropout_p=p_drop))
    cap.load_state_dict({k: torch.from_numpy(x) for k, x in w.items()})
    cap.to(DEV)
    cap.train()
    return cap


def _batch(I, n, V, st, R_, T, seed, eos):
    """Inputs of I images and the raw draws of the I*n rows.  The sentiment words live in the top 14 ids, everything else
    (concept words, draws) below them: the `word_embed` rows of the sentiment words get their gradient from the sentiment
    branch alone.  Draws: row 0 meets <EOS> at step 1; every row of image 1 is finished by step 3; the last live row ends
    at step T - 3, so steps T - 2 and T - 1 lie behind the reference's early `break` (log-probs zero there)."""
    b = synth.make_inputs(I, V, st, regions=R_, seq_len=T, seed=seed)
    lo = V - 14
    b['senti_words'] = lo + b['senti_words'] % 14
    b['cpt_words'] = 4 + b['cpt_words'] % (lo - 4)
    rng = np.random.default_rng(seed + 7)
    draws = rng.integers(4, lo, size=(I * n, T)).astype(np.int64)
    ends = rng.integers(2, T - 2, size=I * n)
    ends[0] = 1
    ends[n:2 * n] = rng.integers(1, 4, size=n)
    ends[-1] = T - 3
    for r, e in enumerate(ends):
        draws[r, e] = eos
    b['draws'], b['ends'] = draws, ends
    return b


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


INPUTS = ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')


def _hip_run(cap, b, n, T, reward, masks=None, grouped=True, replay=True, **kw):
    """forward_rl + REINFORCE loss with a fixed reward + domain-alignment loss + backward.  grouped: captions_per_image = n
    on the per-image inputs; else the plain call on the inputs repeated n times."""
    rep = (lambda x: x) if grouped else (lambda x: x.repeat_interleave(n, 0))
    a = [rep(_dev(b[k])) for k in INPUTS]
    if grouped:
        kw['captions_per_image'] = n
    if replay:
        kw['_replay'] = _dev(b['draws'])
    cap.zero_grad()
    seq, lp, mk = cap.forward_rl(*a, T, 0, _masks=masks, **kw)
    assert lp.requires_grad
    rl = -(lp * mk * reward).sum() / mk.sum()
    da = torch.nn.MSELoss()(cap.cpt_feats, cap.fc_feats.detach())
    (rl + da).backward()
    grads = {k: q.grad.detach().cpu().numpy().copy() for k, q in cap.named_parameters() if q.grad is not None}
    return dict(seq=seq.cpu().numpy(), lp=lp.detach().cpu().numpy(), mk=mk.cpu().numpy(),
                losses=(float(rl.detach()), float(da.detach())), grads=grads,
                shapes=(tuple(cap.fc_feats.shape), tuple(cap.cpt_feats.shape)))


def _oracle_run(w, V, b, n, T, reward, masks, p_drop):
    """The oracle with float64 parameters and autograd on the EXPANDED inputs (per-image masks repeated)."""
    from oracle import captioner_oracle as O
    p = O.to_params(w, dtype=torch.float64, requires_grad=True)
    ids = O.Ids(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES)
    I, R_ = b['att_feats'].shape[:2]
    rep = lambda a: torch.from_numpy(np.ascontiguousarray(a)).repeat_interleave(n, 0)
    om = None
    if masks is not None:
        om = dict(fc=masks['fc'].repeat_interleave(n, 0), att=masks['att'].view(I, R_, -1).repeat_interleave(n, 0),
                  words=masks['words'].view(I, -1, masks['words'].shape[1]).repeat_interleave(n, 0),
                  label=masks['label'].repeat_interleave(n, 0), out=torch.stack([masks['out%d' % t] for t in range(T)]))
    seq, lp, mk, P, _, _ = O.forward_rl(p, ids, rep(b['fc_feats']).double(), rep(b['att_feats']).double(),
                                        rep(b['cpt_words']), rep(b['senti_words']), rep(b['senti_labels']), T, sample_max=0,
                                        replay=torch.from_numpy(b['draws']), masks=om, p_drop=p_drop)
    rl = O.reward_criterion(lp, mk, reward.double())
    da = O.domain_align_loss(P.cpt, P.fc_raw)
    (rl + da).backward()
    return dict(seq=seq.numpy(), lp=lp.detach().numpy(), mk=mk.numpy(), losses=(float(rl.detach()), float(da.detach())),
                grads={k: q.grad.numpy() for k, q in p.items() if q.grad is not None})


def _compare(got, ref, what, min_grads=36):
    assert np.array_equal(got['seq'], ref['seq']) and np.array_equal(got['mk'], ref['mk']), what
    np.testing.assert_allclose(got['lp'], ref['lp'], atol=1e-4, err_msg=what)
    np.testing.assert_allclose(got['losses'], ref['losses'], rtol=5e-5, err_msg=what)
    for k, r in ref['grads'].items():
        assert k in got['grads'], (what, k)
        np.testing.assert_allclose(got['grads'][k], r, atol=GRAD_RTOL * np.abs(r).max() + 1e-7, err_msg='%s %s' % (what, k))
    assert len(ref['grads']) >= min_grads and set(got['grads']) == set(ref['grads']), what


SENTI_BRANCH = ('attention.senti_att.h2word.weight', 'attention.senti_att.h2word.bias',
                'attention.senti_att.label2word.weight', 'attention.senti_att.label2word.bias',
                'attention.senti_att.word_alpha.weight', 'senti2att.0.weight', 'senti2att.0.bias',
                'senti_label_embed.0.weight')


@pytest.mark.parametrize('mode', [1, 0], ids=['split_f16', 'exact_fp32'])
@pytest.mark.parametrize('n', [2, 5])
def test_grouped_rl_tiny_vs_float64_oracle_on_the_expanded_inputs(n, mode):
    """'tiny' settings, V = 64, I = 3, R = 6, T = 8, both GEMM engines, training mode: with dropout off and with explicit
    masks (per-image 'fc' [I,E], 'att' [I*R,E], 'words' [I*Mw,Wd], 'label' [I,Wd], repeated for the oracle; 'out<t>'
    per row).  Tokens and masks equal, log-probs within 1e-4, REINFORCE and domain-alignment losses within rtol 5e-5 and
    every parameter gradient within GRAD_RTOL * max|ref| + 1e-7 of the oracle's float64 autograd on the repeated inputs;
    the same parameter set as the oracle's (>= 36); [I, E] attributes.  The sentiment branch - which had no grouped
    backward - has non-zero gradients, the `word_embed` rows of the sentiment words included."""
    V, I, R_, T, st = 64, 3, 6, 8, synth.TINY_SETTINGS
    w = synth.make_weights(V, st, seed=3)
    eos = synth.make_idx2word(V).index('<EOS>')
    b = _batch(I, n, V, st, R_, T, 60 + n, eos)
    E, H, Wd, p_drop = st['feat_emb_dim'], st['rnn_hid_dim'], st['word_emb_dim'], st['dropout_p']
    Mw = b['senti_words'].shape[1] + 1
    g = torch.Generator().manual_seed(n)
    keep = lambda *shape: (torch.rand(*shape, generator=g) >= p_drop).to(torch.uint8)
    masks = dict(fc=keep(I, E), att=keep(I * R_, E), words=keep(I * Mw, Wd), label=keep(I, Wd),
                 **{'out%d' % t: keep(I * n, H) for t in range(T)})
    reward = torch.randn(I * n, T, generator=g)
    prev = ops.h3_mode()
    ops.set_h3_mode(mode)
    try:
        for p, m in ((0.0, None), (p_drop, masks)):
            cap = _captioner(w, V, st, p)
            got = _hip_run(cap, b, n, T, reward.to(DEV), m)
            ref = _oracle_run(w, V, b, n, T, reward, m, p_drop)
            what = 'n=%d engine=%d masks=%d' % (n, mode, m is not None)
            # the draws do what the docstring of _batch says
            live = ref['mk'] > 0
            assert ref['seq'][0, 1] == eos and not live[0, 2:].any()
            assert not live[n:2 * n, 4:].any()
            assert live[:, T - 3].any() and not live[:, T - 2:].any() and (ref['lp'][:, T - 2:] == 0).all()
            assert (got['lp'][:, T - 2:] == 0).all()
            assert got['shapes'] == ((I, E), (I, E)), what
            _compare(got, ref, what)
            sw_rows = np.unique(b['senti_words'])
            for grads in (ref['grads'], got['grads']):
                for k in SENTI_BRANCH:
                    assert np.abs(grads[k]).max() > 0, (what, k)
                assert np.abs(grads['word_embed.0.weight'][sw_rows]).max() > 0, what
    finally:
        ops.set_h3_mode(prev)


@pytest.mark.parametrize('I,n,R_', [(2, 5, 36), (2, 3, 196)], ids=['36_regions', '196_regions'])
def test_grouped_rl_default_dims_vs_the_repeated_form(I, n, R_):
    """Default dimensions, V = 10000, T = 20, training mode with dropout off, the same `_replay` for both calls: the
    grouped call against this build's own call on the repeated inputs at the same bars, and the grouped call's peak
    device memory below the repeated call's."""
    V, T, st = 10000, 20, synth.DEFAULT_SETTINGS
    w = synth.make_weights(V, st, seed=5)
    eos = synth.make_idx2word(V).index('<EOS>')
    b = _batch(I, n, V, st, R_, T, 80 + n, eos)
    cap = _captioner(w, V, st, 0.0)
    reward = torch.randn(I * n, T, generator=torch.Generator().manual_seed(n)).to(DEV)
    peak, runs = {}, {}
    for grouped in (False, True):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        runs[grouped] = _hip_run(cap, b, n, T, reward, None, grouped=grouped)
        torch.cuda.synchronize()
        peak[grouped] = torch.cuda.max_memory_allocated()
    print('GROUPRL peak bytes grouped %d repeated %d' % (peak[True], peak[False]))
    assert runs[True]['shapes'] == ((I, st['feat_emb_dim']),) * 2
    assert runs[False]['shapes'] == ((I * n, st['feat_emb_dim']),) * 2
    _compare(runs[True], runs[False], 'I=%d n=%d R=%d' % (I, n, R_))
    assert peak[True] < peak[False]


def test_grouped_rl_training_mode_is_repeatable_and_takes_the_constraints():
    """I = 4, n = 3, tiny settings, training mode with the default dropout, fixed torch seed: two runs give equal tokens
    and bit-equal gradients (no atomics anywhere in the grouped backward).  Under suppress_special, decoding_constraint=1,
    min_len=3 no live position holds <PAD>, <SOS>, <UNK>, a repeat of the token just fed, or <EOS> before step 3, and
    the gradients are finite."""
    V, I, n, R_, T, st = 64, 4, 3, 6, 8, synth.TINY_SETTINGS
    w = synth.make_weights(V, st, seed=3)
    i2w = synth.make_idx2word(V)
    b = _batch(I, n, V, st, R_, T, 33, i2w.index('<EOS>'))
    cap = _captioner(w, V, st, st['dropout_p'])
    reward = torch.randn(I * n, T, generator=torch.Generator().manual_seed(1)).to(DEV)
    for kw in (dict(), dict(suppress_special=True, decoding_constraint=1, min_len=3)):
        runs = []
        for _ in range(2):
            torch.manual_seed(1234)
            torch.cuda.manual_seed_all(1234)
            runs.append(_hip_run(cap, b, n, T, reward, replay=False, **kw))
        a, c = runs
        assert a['seq'].shape == (I * n, T) and np.array_equal(a['seq'], c['seq']) and np.array_equal(a['mk'], c['mk'])
        assert np.array_equal(a['lp'], c['lp']) and a['losses'] == c['losses']
        assert len(a['grads']) >= 36
        for k, gk in a['grads'].items():
            assert np.isfinite(gk).all(), k
            assert np.array_equal(gk, c['grads'][k]), k
        if kw:
            seq, live = a['seq'], a['mk'] > 0
            pad, sos, eos, unk = (i2w.index(x) for x in ('<PAD>', '<SOS>', '<EOS>', '<UNK>'))
            assert live.any() and not np.isin(seq[live], [pad, sos, unk]).any()
            fed = np.concatenate([np.full((I * n, 1), sos), seq[:, :-1]], 1)
            assert (seq[live] != fed[live]).all()
            assert not (seq[:, :3] == eos)[live[:, :3]].any()
        # an image's rows are different draws, not copies
        assert any(not np.array_equal(a['seq'][i * n], a['seq'][i * n + 1]) for i in range(I))


# ------------------------------------------------------------------------------------------------ Detector
def _detector(V, TN, st):
    from insenticap_model_amd.detector import Detector
    from test_detector import load_helper
    det = Detector(synth.make_idx2word(V), TN, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-4}, st)
    det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=3).items()})
    load_helper(det.senti_detector, 51)
    load_helper(det.sent_senti_cls, 52)
    return det.to(DEV)


@pytest.mark.parametrize('data_type', ['fact', 'senti'])
def test_detector_trains_on_samples_per_image_without_a_greedy_rollout(data_type):
    """One Detector.forward training call over tiny synthetic loaders of 2 batches, I = 4, rl_samples_per_image = 3: the
    greedy roll-out is never called (a wrapper on captioner.forward_rl counts the sample_max=1 calls), the sampled one
    runs with captions_per_image = 3 on the I images, the dictionary has today's keys and `sample_score`, every value is
    finite, |fact_reward| <= 1e-6 (the mean advantage), the parameters change.  With rl_samples_per_image = 1 the wrapper
    sees today's one greedy call per iteration."""
    V, TN, B = 64, 8, 4
    st = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
    batches, split = synth.make_rl_batches(2, B, V, st, seq_len=TN, seed=70)
    t = torch.from_numpy
    if data_type == 'fact':
        items = [(b[0], t(b[1]), t(b[2]), (t(b[3][0]), b[3][1]), t(b[4]), t(b[5]), b[6]) for b in batches]
    else:
        rng = np.random.default_rng(5)
        items = [(b[0], t(b[1]), t(b[2]), t(b[4]), t(b[5]),
                  t(rng.integers(0, len(synth.SENTIMENT_CATEGORIES), size=B).astype(np.int64))) for b in batches]
    s = synth.make_inputs(4, V, st, regions=6, seq_len=TN, seed=72)
    scs = [((t(s['captions']), s['lengths']), t(s['cpt_words']), t(s['senti_words']), t(s['senti_labels']))]
    torch.manual_seed(0)
    det = _detector(V, TN, st)
    det.set_ciderd_scorer(split)
    assert det.rl_samples_per_image == 1
    seen = []
    orig = det.captioner.forward_rl

    def spy(*args, **kw):
        out = orig(*args, **kw)
        seen.append((kw.get('sample_max'), kw.get('captions_per_image', 1), args[0].shape[0], out[0].shape[0]))
        return out
    det.captioner.forward_rl = spy
    det.rl_samples_per_image = 3
    before = {k: v.detach().clone() for k, v in det.captioner.state_dict().items()}
    out = det((items, scs), data_type, True)
    torch.cuda.synchronize()
    assert det._rl_graph is None                                  # served eagerly
    assert seen == [(0, 3, B, 3 * B)] * 2                         # no greedy roll-out; rows = 3 per image
    want = {'da_loss', 'cls_reward', 'all_rewards', 'cap_loss', 'seq2seq_loss', 'sample_score', 'fact_reward'}
    if data_type == 'fact':
        want.add('xe_loss')
    assert set(out) == want
    assert all(np.isfinite(v) for v in out.values()), out
    assert abs(out['fact_reward']) <= 1e-6
    assert out['sample_score'] >= 0.0 and (data_type == 'fact' or out['sample_score'] == 0.0)
    after = det.captioner.state_dict()
    assert len([k for k in before if not torch.equal(before[k], after[k])]) >= 36
    # evaluation keeps the n = 1 path: sample + greedy per batch
    del seen[:]
    det((items,), data_type, False)
    assert sorted(seen) == [(0, 1, B, B)] * 2 + [(1, 1, B, B)] * 2
    # ... and so does training with rl_samples_per_image = 1 (eager sequence: the wrapper sees every roll-out)
    del seen[:]
    det.rl_samples_per_image, det.train_graphs = 1, False
    out1 = det((items, scs), data_type, True)
    assert sorted(seen) == [(0, 1, B, B)] * 2 + [(1, 1, B, B)] * 2
    assert 'sample_score' not in out1
