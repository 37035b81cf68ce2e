"""CIDEr-D on the device (isc_cider_dev_score, rewards.DeviceCiderD): the kernel against the golden vectors of the
reference's scorer and against the host scorer on the same rows (1e-12: the bar tests/test_cider.py holds the host scorer
to), its edge shapes, the refusal of T = 64, the device form of the self-critical reward, `Detector.device_cider`
against the same detector with the flag off, and one capture into a HIP graph.  No test sends an id above 65534 to the
device and none provokes a fault: the refusals are host checks."""
import numpy as np
import pytest
import torch

from insenticap_model_amd import _lib, ops, rewards, synth
from test_cider import CASES, setup

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SOS, EOS = 1, 2
ATOL = 1e-12
_CACHE = {}


def case(name):
    if name not in _CACHE:
        split, fns, gt, sample, greedy = setup(name)
        scorer = rewards.get_ciderd_scorer(split, SOS, EOS)
        _CACHE[name] = (scorer, scorer.to_device(DEV, CASES[name][1]), fns, gt, sample, greedy)
    return _CACHE[name]


def both(scorer, dev, hyps, ref_lists, row_div=1):
    """(device scores, host scores) of int64 rows [N, T]; row r against ref_lists[r // row_div]."""
    hyps = np.ascontiguousarray(hyps, dtype=np.int64)
    pack = dev.pack_refs(ref_lists)
    got = dev.score(torch.from_numpy(hyps).to(DEV), pack, row_div=row_div)
    torch.cuda.synchronize()
    host = scorer.score_arrays(hyps, [ref_lists[r // row_div] for r in range(len(hyps))])
    return got.cpu().numpy(), host


@pytest.mark.parametrize('name', ['small', 'cfg5'])
def test_kernel_matches_the_goldens_and_the_host_scorer(golden, name):
    scorer, dev, fns, gt, sample, greedy = case(name)
    rows = np.concatenate([sample, greedy])
    assert rows.shape == {'small': (32, 12), 'cfg5': (512, 20)}[name]
    refs = [gt[f] for f in fns] * 2
    got, host = both(scorer, dev, rows, refs)
    print('CIDERDEV [%s] max |device - host| = %.3e, max |device - golden| = %.3e'
          % (name, np.abs(got - host).max(), np.abs(got - golden('cider')[name + '/scores']).max()))
    np.testing.assert_allclose(got, golden('cider')[name + '/scores'], rtol=0, atol=ATOL)
    np.testing.assert_allclose(got, host, rtol=0, atol=ATOL)
    assert got.max() > 1.0
    # two launches give the same bits (cached references: the second pack comes from the per-image cache)
    pack = dev.pack_refs(refs, keys=list(fns) * 2)
    d = torch.from_numpy(rows).to(DEV)
    a, b = dev.score(d, pack), dev.score(d, dev.pack_refs(refs, keys=list(fns) * 2))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), got)


def test_edge_shapes_against_the_host_scorer():
    scorer, dev, fns, gt, sample, greedy = case('small')
    refs = [gt[f] for f in fns]
    rng = np.random.default_rng(3)

    def check(what, hyps, ref_lists, sc=scorer, dv=dev, row_div=1):
        got, host = both(sc, dv, hyps, ref_lists, row_div)
        assert np.isfinite(got).all(), what
        assert np.abs(got - host).max() <= ATOL, (what, got, host)
        return got

    T = 12
    # <EOS> then <PAD>: L = 1, the norms of orders 2-4 are zero and the guard is taken
    hyp = np.zeros((1, T), dtype=np.int64)
    hyp[0, 0] = EOS
    got = check('<EOS> first', hyp, refs[:1])
    assert got[0] == 0.0         # (<EOS> ends every caption of every image: its idf, hence the 1-gram's norm too, is 0)
    # a leading <SOS> is dropped
    ref0 = refs[0][0][1:-1]
    hyp = np.zeros((2, T), dtype=np.int64)
    hyp[0, :len(ref0[:8])] = ref0[:8]
    hyp[0, len(ref0[:8])] = EOS
    hyp[1, 0] = SOS
    hyp[1, 1:T] = hyp[0, :T - 1]
    got = check('leading <SOS>', hyp, [refs[0], refs[0]])
    assert got[0] == got[1] and got[0] > 1.0
    # no <EOS>: L = T + 1, at T = 1, 20 and 63 (the references' own words tiled, so that n-grams match)
    for Tn in (1, 20, 63):
        words = [w for capn in refs[1] for w in capn[1:-1]]
        hyp = np.asarray([(words * 8)[:Tn], (words[3:] * 8)[:Tn]], dtype=np.int64)
        assert not (hyp == EOS).any()
        got = check('no <EOS>, T = %d' % Tn, hyp, [refs[1], refs[1]])
        assert (got > 0).all()
    # one repeated id against a reference that holds it twice: tf > 1 and clipping
    caps = [[[SOS, 7, 7, 5, EOS], [SOS, 5, 6, 7, EOS]], [[SOS, 8, 9, EOS]], [[SOS, 9, 9, 9, 4, EOS]]]
    sc2 = rewards.CiderD(caps, SOS, EOS)
    dv2 = sc2.to_device(DEV, 128)
    hyp = np.zeros((1, 6), dtype=np.int64)
    hyp[0, :4] = 7
    hyp[0, 4] = EOS
    got = check('repeated id', hyp, [caps[0]], sc2, dv2)
    assert got[0] > 0
    # ids that occur in no reference: every lookup is absent (the appended <EOS> aside, hence no <EOS> in the references)
    caps3 = [[[4, 5, 6]], [[5, 6, 7, 8]]]
    sc3 = rewards.CiderD(caps3, SOS, 99)       # (<EOS> = 99 is appended to references and rows alike ...)
    dv3 = sc3.to_device(DEV, 128)
    hyp = np.asarray([[70, 71, 72, 73, 74, 75]], dtype=np.int64)
    got = check('unseen ids', hyp, [caps3[0]], sc3, dv3)
    assert 0 <= got[0] < 1.0                   # ... so only its 1-gram can match
    # id 65534 in the hypothesis and a reference, a scorer over such a vocabulary
    caps4 = [[[SOS, 65534, 7, 65534, 9, EOS], [SOS, 7, 8, EOS]], [[SOS, 9, 65534, 65533, EOS]]]
    sc4 = rewards.CiderD(caps4, SOS, EOS)
    dv4 = sc4.to_device(DEV, 65535)
    hyp = np.asarray([[65534, 7, 65534, 9, EOS, 0, 0], [65533, 7, 65534, 9, EOS, 0, 0]], dtype=np.int64)
    got = check('id 65534', hyp, [caps4[0], caps4[0]], sc4, dv4)
    assert got[0] > got[1] > 0                 # (65533 is another word)
    # images with 1 and with 7 references, one reference of 40 words
    ids = lambda n: [int(x) for x in rng.integers(4, 30, size=n)]
    caps5 = [[[SOS] + ids(9) + [EOS]], [[SOS] + ids(int(k)) + [EOS] for k in (5, 40, 8, 11, 3, 17, 9)],
             [[SOS] + ids(6) + [EOS], [SOS] + ids(7) + [EOS]]]
    sc5 = rewards.CiderD(caps5, SOS, EOS)
    dv5 = sc5.to_device(DEV, 64)
    hyp = np.zeros((3, 45), dtype=np.int64)
    hyp[0, :10] = caps5[0][0][1:]
    hyp[1, :41] = caps5[1][1][1:]              # the 40-word reference itself: 41 words with <EOS>, 4 x 41 - 6 n-grams
    hyp[2, :5] = caps5[2][1][2:7]
    hyp[2, 5] = EOS
    got = check('1 / 7 / 2 references, 40 words', hyp, caps5, sc5, dv5)
    assert got[0] > 5.0 and got[1] > 0.5
    # row_div = 5 with I = 3: the rows of one image share its references
    hyp = np.zeros((15, 14), dtype=np.int64)
    for r in range(15):
        capn = caps5[r // 5][r % len(caps5[r // 5])][1:-1][:13]
        keep = [w if rng.random() < 0.8 else int(rng.integers(4, 30)) for w in capn]
        hyp[r, :len(keep)] = keep
        if r % 3:
            hyp[r, len(keep)] = EOS
    got = check('row_div = 5', hyp, caps5, sc5, dv5, row_div=5)
    assert len(set(np.round(got, 9))) >= 10
    # N = 1 and N = 5 (no multiple of the four waves of a workgroup): rows behind the output stay untouched
    for N in (1, 5):
        rows = np.ascontiguousarray(sample[:N])
        out = torch.full((N + 3,), -7.0, dtype=torch.float64, device=DEV)
        pack = dev.pack_refs(refs[:N])
        dev.score(torch.from_numpy(rows).to(DEV), pack, out=out[:N])
        torch.cuda.synchronize()
        assert bool((out[N:] == -7.0).all()), N
        assert np.abs(out[:N].cpu().numpy() - scorer.score_arrays(rows, refs[:N])).max() <= ATOL, N


def test_t_64_is_refused_and_nothing_is_written():
    scorer, dev, fns, gt, sample, greedy = case('small')
    pack = dev.pack_refs([gt[f] for f in fns[:2]])
    out = torch.full((2,), -7.0, dtype=torch.float64, device=DEV)
    hyp = torch.full((2, 64), 5, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.HipLibraryError, match='ISC_E_SHAPE'):
        dev.score(hyp, pack, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    with pytest.raises(ValueError):
        dev.score(hyp[:, :8].contiguous(), pack, row_div=2)         # 2 rows are not 2 images x 2
    with pytest.raises(RuntimeError):
        dev.pack_refs([gt[fns[0]], []])                              # an image without references
    with pytest.raises(ValueError):
        scorer.to_device(DEV, 65536)


def test_self_critical_reward_on_the_device():
    scorer, dev, fns, gt, sample, greedy = case('cfg5')
    host = rewards.get_self_critical_reward(sample, greedy, fns, gt, SOS, EOS, scorer).astype('float32')
    pack = dev.pack_refs([gt[f] for f in fns], keys=list(fns))
    got = rewards.get_self_critical_reward_device(torch.from_numpy(sample).to(DEV), torch.from_numpy(greedy).to(DEV),
                                                  pack, dev)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == sample.shape and got.is_contiguous()
    got = got.cpu().numpy()
    assert (got == got[:, :1]).all()                                  # repeated over T
    ulp = np.spacing(np.abs(host)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - host.astype(np.float64)) <= ulp).all()
    assert np.abs(host).max() > 0.5


def test_score_is_capturable():
    """One capture of DeviceCiderD.score into a HIP graph, replayed twice, gives the eager bits (also on new rows)."""
    scorer, dev, fns, gt, sample, greedy = case('small')
    pack = dev.pack_refs([gt[f] for f in fns])
    rows = torch.from_numpy(sample).to(DEV)
    eager_s, eager_g = dev.score(rows, pack).clone(), dev.score(torch.from_numpy(greedy).to(DEV), pack).clone()
    out = torch.zeros(len(sample), dtype=torch.float64, device=DEV)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        dev.score(rows, pack, out=out)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            dev.score(rows, pack, out=out)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_s)
    rows.copy_(torch.from_numpy(greedy))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_g) and not torch.equal(eager_s, eager_g)


# ------------------------------------------------------------------------------------------------ Detector
def _detector(V, TN, st):
    from insenticap_model_amd.detector import Detector
    from test_detector import load_helper
    det = Detector(synth.make_idx2word(V), TN, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-4}, st)
    det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=3).items()})
    load_helper(det.senti_detector, 51)
    load_helper(det.sent_senti_cls, 52)
    return det.to(DEV)


def _run_detector(flag, calls):
    """A fresh detector (same weights), device_cider = flag, then the calls in order, each behind the same seed.  With the
    flag on the host scorer's score_arrays raises: it must not be called.  Returns (dicts, sampled token matrices)."""
    V, TN, B = 64, 8, 4
    st = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
    batches, split = synth.make_rl_batches(2, B, V, st, seq_len=TN, seed=70)
    t = torch.from_numpy
    fact = [(b[0], t(b[1]), t(b[2]), (t(b[3][0]), b[3][1]), t(b[4]), t(b[5]), b[6]) for b in batches]
    rng = np.random.default_rng(5)
    senti = [(b[0], t(b[1]), t(b[2]), t(b[4]), t(b[5]),
              t(rng.integers(0, len(synth.SENTIMENT_CATEGORIES), size=B).astype(np.int64))) for b in batches]
    s = synth.make_inputs(4, V, st, regions=6, seq_len=TN, seed=72)
    scs = [((t(s['captions']), s['lengths']), t(s['cpt_words']), t(s['senti_words']), t(s['senti_labels']))]
    torch.manual_seed(0)
    det = _detector(V, TN, st)
    det.set_ciderd_scorer(split)
    det.device_cider = flag
    host_score = det.ciderd_scorer.score_arrays
    if flag:
        def never(*a, **k):
            raise AssertionError('the host CIDEr-D scorer was called with device_cider on')
        det.ciderd_scorer.score_arrays = never
    sampled = []
    orig = det.captioner.forward_rl

    def spy(*args, **kw):
        out = orig(*args, **kw)
        if kw.get('sample_max') == 0:
            sampled.append(out[0].detach().cpu().numpy().copy())
        return out
    det.captioner.forward_rl = spy
    outs = []
    for data_type, training, n in calls:
        det.rl_samples_per_image, det.train_graphs = n, False
        torch.manual_seed(1234)
        torch.cuda.manual_seed_all(1234)
        data = (fact if data_type == 'fact' else senti, scs) if training else (fact if data_type == 'fact' else senti,)
        outs.append(det(data, data_type, training))
        torch.cuda.synchronize()
    assert det._rl_graph is None                                     # every call ran the eager sequence
    return outs, sampled, host_score, fact


def test_detector_takes_the_fact_reward_from_the_device_scorer():
    """One 'fact' evaluation call and one grouped 'fact' training call (n = 3), two batches of 4 images each, with the flag
    off and on: the sampled tokens are identical; fact_reward within 1e-6 (one float32 ulp at a score <= 10 - asserted),
    sample_score within 1e-9, cap_loss within 1e-5 relative.  One 'senti' training call returns the same dictionary."""
    calls = [('fact', False, 1), ('fact', True, 3), ('senti', True, 1)]
    off, tok_off, host_score, fact = _run_detector(False, calls)
    on, tok_on, _, _ = _run_detector(True, calls)
    assert len(tok_off) == len(tok_on) == 6
    for a, b in zip(tok_off, tok_on):
        assert np.array_equal(a, b)
    # the synthetic scores stay below 10 (the bound on fact_reward is one float32 ulp there)
    for i, toks in enumerate(tok_off[:4]):
        b = fact[i % 2]
        n = toks.shape[0] // len(b[0])
        sc = host_score(toks, [b[6][fn] for fn in b[0] for _ in range(n)])
        assert 0 <= sc.min() and sc.max() < 10.0
    ev_off, ev_on = off[0], on[0]
    assert set(ev_off) == set(ev_on) and 'fact_reward' in ev_on
    assert abs(ev_off['fact_reward'] - ev_on['fact_reward']) <= 1e-6
    assert abs(ev_off['cap_loss'] - ev_on['cap_loss']) <= 1e-5 * abs(ev_off['cap_loss'])
    tr_off, tr_on = off[1], on[1]
    assert set(tr_off) == set(tr_on) and 'sample_score' in tr_on
    print('CIDERDEV detector: eval', ev_off, ev_on, 'grouped', tr_off, tr_on)
    assert abs(tr_off['fact_reward'] - tr_on['fact_reward']) <= 1e-6
    assert abs(tr_off['sample_score'] - tr_on['sample_score']) <= 1e-9 and tr_on['sample_score'] > 0
    assert abs(tr_off['cap_loss'] - tr_on['cap_loss']) <= 1e-5 * abs(tr_off['cap_loss'])
    assert off[2] == on[2]


def test_detector_keeps_the_host_scorer_outside_the_device_scorers_domain():
    """max_seq_len > 63: one warning, the host scorer serves, the numbers are the flag-off ones."""
    from insenticap_model_amd.detector import Detector
    st = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
    det = Detector(synth.make_idx2word(64), 8, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-4}, st).to(DEV)
    _, split = synth.make_rl_batches(1, 4, 64, st, seq_len=8, seed=70)
    det.set_ciderd_scorer(split)
    assert det.device_cider is False and det._device_ciderd(DEV, 8) is None
    det.device_cider = True
    twin = det._device_ciderd(DEV, 8)
    assert isinstance(twin, rewards.DeviceCiderD) and det._device_ciderd(DEV, 63) is twin
    with pytest.warns(UserWarning, match='host CIDEr-D'):
        assert det._device_ciderd(DEV, 64) is None
    det.set_ciderd_scorer(split)                                     # a new host scorer: the twin is rebuilt
    again = det._device_ciderd(DEV, 8)
    assert again is not twin and again.host is det.ciderd_scorer
