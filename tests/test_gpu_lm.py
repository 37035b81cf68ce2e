"""The n-gram language models above the kernel (tests/test_gpu_lm_kernels.py holds the kernel alone to the restatement):
DeviceNgramLMSet against the host set in bits, the device form of the LM reward against the host form, eager 'fact' and
'senti' iterations of a Detector (one of the width sets of tests/_widths.py) with lm_flag = 0.1 - host LM path against
device LM path: the same rewards, the same logged 'lm_reward', the same updated parameters, in bits -, lm_flag = 0 with
models set against no models, the refused grouped iteration, caption_perplexity and train.eval_ppl."""
import numpy as np
import pytest
import torch

import _lm_ref as R
import _widths as W
from insenticap_model_amd import rewards, synth, train

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
V, TN, B = W.V, W.T, 5
# (h_768: rnn_hid_dim != att_hid_dim, and fc_feat_dim == att_feat_dim, which the image-sentiment detector's convolutions need)
ST = dict(W.H_768, **synth.HELPER_SETTINGS)
_cache = {}


def lm_set():
    """Three order-3 models over 60 of the V words each, no special id among them: (host set, device twin, their
    n-grams, <SOS>, <EOS>), built once."""
    if 'set' not in _cache:
        idx2word = synth.make_idx2word(V)
        sos, eos = idx2word.index('<SOS>'), idx2word.index('<EOS>')
        grams = [R.random_lm(90 + i, V, 3, per_order=150, words=list(range(10 + 5 * i, 70 + 5 * i))) for i in range(3)]
        host = rewards.NgramLMSet([rewards.NgramLM.from_arpa(R.write_arpa(g), V) for g in grams], V, 'word', True,
                                  sos=sos, eos=eos)
        _cache['set'] = (host, host.to_device(DEV), grams, sos, eos)
    return _cache['set']


def random_rows(N, T, seed):
    host, dev, grams, sos, eos = lm_set()
    rows = np.concatenate([R.walk_rows(grams[i % 3], (N + 2 - i) // 3, T, V, sos, eos, seed=seed + i) for i in range(3)])
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(rows))
    return rows[perm], rng.integers(0, 3, size=len(rows)).astype(np.int64)


def test_device_set_equals_the_host_set_in_bits():
    host, dev, grams, sos, eos = lm_set()
    rows, labels = random_rows(257, 20, seed=5)
    assert rows.shape == (257, 20)
    s, ns, no, tok = host.score(rows, labels, tok_logp=True)
    d_tok = torch.zeros(257, 22, dtype=torch.float64, device=DEV)
    d_s, d_ns, d_no = dev.score(torch.from_numpy(rows).to(DEV), torch.from_numpy(labels).to(DEV), tok_logp=d_tok)
    torch.cuda.synchronize()
    assert np.array_equal(d_s.cpu().numpy().view(np.int64), s.view(np.int64))
    assert np.array_equal(d_ns.cpu().numpy(), ns) and np.array_equal(d_no.cpu().numpy(), no)
    assert np.array_equal(d_tok.cpu().numpy().view(np.int64), tok.view(np.int64))
    assert (no > 0).any() and (ns > 3).any() and len(set(s.tolist())) > 200
    # a non-contiguous token matrix and no labels
    wide = torch.from_numpy(np.concatenate([rows, rows], axis=1)).to(DEV)
    d2 = dev.score(wide[:, :20])[0]
    assert np.array_equal(d2.cpu().numpy().view(np.int64), host.score(rows)[0].view(np.int64))


def test_lm_reward_on_the_device():
    host, dev, grams, sos, eos = lm_set()
    sample, labels = random_rows(64, 12, seed=11)
    greedy, _ = random_rows(64, 12, seed=12)
    greedy[::5] = sample[::5]
    t = lambda a: torch.from_numpy(a).to(DEV)
    want = rewards.get_lm_reward(sample, greedy, labels, sos, eos, host).astype('float32')
    got = rewards.get_lm_reward_device(t(sample), t(greedy), t(labels), dev)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == sample.shape and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), want) and set(np.unique(want)) == {-1.0, 0.0, 1.0}
    # 'ppl_diff': the scores are the host's bits; the two 10 ** x are the device's pow against the host's - a few fp64
    # ulps of perplexities p <= P apart, far inside one float32 ulp of P; the float32 of their difference is held to that
    want = rewards.get_lm_reward(sample, greedy, labels, sos, eos, host, form='ppl_diff')
    got = rewards.get_lm_reward_device(t(sample), t(greedy), t(labels), dev, form='ppl_diff').cpu().numpy()
    s, sn, _ = host.score(sample, labels)
    g, gn, _ = host.score(greedy, labels)
    top = np.maximum(10.0 ** (-s / sn), 10.0 ** (-g / gn))
    assert (got == got[:, :1]).all() and np.isfinite(got).all()
    assert (np.abs(got.astype(np.float64) - want) <= np.spacing(top.astype(np.float32)).astype(np.float64)[:, None]).all()
    assert (got[::5] == 0).all() and np.abs(want).max() > 1.0


# ------------------------------------------------------------------------------------------------ Detector
def _give_back(det):
    from insenticap_model_amd import ops
    torch.cuda.synchronize()
    if det.__dict__.get('_rl_graph') is not None:
        det._rl_graph.close()
    cap = det.captioner
    st = cap.__dict__.pop('_ro_stream', None)
    if st is not None:
        cap.enable_rollout_graphs(False)
        ops.release_stream_state(DEV.index, st.cuda_stream)


def _data():
    if 'data' not in _cache:
        batches, split = synth.make_rl_batches(1, B, V, ST, seq_len=TN, seed=70)
        t = torch.from_numpy
        fact = [(b[0], t(b[1]), t(b[2]), (t(b[3][0]), b[3][1]), t(b[4]), t(b[5]), b[6]) for b in batches]
        rng = np.random.default_rng(5)
        senti = [(b[0], t(b[1]), t(b[2]), t(b[4]), t(b[5]), t(rng.integers(0, 3, size=B).astype(np.int64))) for b in batches]
        s = synth.make_inputs(4, V, ST, regions=6, seq_len=TN, seed=72)
        scs = [((t(s['captions']), s['lengths']), t(s['cpt_words']), t(s['senti_words']), t(s['senti_labels']))]
        _cache['data'] = (fact, senti, scs, split)
    return _cache['data']


def _detector():
    from insenticap_model_amd.detector import Detector
    from test_detector import load_helper
    torch.manual_seed(0)
    det = Detector(W.idx2word(), TN, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-4}, ST)
    det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, ST, seed=W.WIDTHS['h_768']['wseed']).items()})
    load_helper(det.senti_detector, 51)
    load_helper(det.sent_senti_cls, 52)
    det = det.to(DEV)
    det.set_ciderd_scorer(_data()[3])
    det.train_graphs = False
    return det


def _run(data_type, lms, lm_flag, lm_path, training=True):
    """One eager iteration of a fresh detector -> (loss dictionary, the rewards handed to the RL criterion, parameters).
    lm_path 'device': device_cider on; 'host': device_cider on as well (the same CIDEr-D path), the device LM twin
    withheld, so that the LM reward alone takes the host scorer."""
    fact, senti, scs, _ = _data()
    det = _detector()
    if lms is not None:
        det.set_lms(lms)
    det.lm_flag = lm_flag
    det.device_cider = True
    called = {'host': 0, 'device': 0}
    if lms is not None:
        host_score, twin = lms.score, det._device_lms

        def counted(*a, **k):
            called['host'] += 1
            return host_score(*a, **k)
        lms.score = counted
        if lm_path == 'host':
            det._device_lms = lambda device, T: None
        else:
            def counted_twin(device, T):
                called['device'] += 1
                return twin(device, T)
            det._device_lms = counted_twin
    seen = []
    crit = det.cap_rl_crit.forward

    def spy(logp, masks, reward):
        seen.append(reward.detach().clone())
        return crit(logp, masks, reward)
    det.cap_rl_crit.forward = spy
    torch.manual_seed(1234)
    torch.cuda.manual_seed_all(1234)
    items = fact if data_type == 'fact' else senti
    try:
        out = det((items, scs) if training else (items,), data_type, training)
        torch.cuda.synchronize()
    finally:
        if lms is not None:
            lms.score = host_score
    assert det._rl_graph is None and len(seen) == 1
    params = [p.detach().clone() for p in det.captioner.parameters()]
    _give_back(det)
    return out, seen[0], params, called


@pytest.mark.parametrize('data_type', ['fact', 'senti'])
def test_detector_iteration_host_lm_path_against_device_lm_path(data_type):
    host, dev, grams, sos, eos = lm_set()
    o_h, r_h, p_h, c_h = _run(data_type, host, 0.1, 'host')
    o_d, r_d, p_d, c_d = _run(data_type, host, 0.1, 'device')
    assert c_h['host'] == 2 and c_d == {'host': 0, 'device': 1}          # (sample and greedy rows / no host call at all)
    assert 'lm_reward' in o_h and set(o_h) == set(o_d)
    print('LM detector %s: host %r device %r' % (data_type, o_h, o_d))
    # a sum of signs, divided by len((loader, loader)) as every entry of the dictionary is
    assert o_h['lm_reward'] == o_d['lm_reward'] and float(2 * o_h['lm_reward']).is_integer()
    assert torch.equal(r_h, r_d)
    assert all(torch.equal(a, b) for a, b in zip(p_h, p_d))
    for k in o_h:
        assert o_h[k] == o_d[k], k
    # the term is in the rewards: against lm_flag = 0 they differ by 0.1 x sign, row by row
    o_0, r_0, p_0, _ = _run(data_type, host, 0.0, 'device')
    assert 'lm_reward' not in o_0
    delta = (r_d - r_0)[:, 0].cpu().numpy()
    assert np.abs(delta).max() > 0.05 and (np.abs(np.abs(delta[np.abs(delta) > 0.05]) - 0.1) < 1e-6).all()
    assert abs(delta.sum() / 0.1 - o_d['lm_reward'] * 2) < 1e-3          # (the dictionary divides by len((loader, loader)))
    assert not all(torch.equal(a, b) for a, b in zip(p_0, p_d))


def test_lm_flag_zero_changes_nothing():
    host, dev, grams, sos, eos = lm_set()
    o_n, r_n, p_n, _ = _run('fact', None, 0.0, 'device')
    o_z, r_z, p_z, called = _run('fact', host, 0.0, 'device')
    assert called == {'host': 0, 'device': 0}
    assert o_n == o_z and list(o_n) == list(o_z) and 'lm_reward' not in o_z
    assert torch.equal(r_n, r_z) and all(torch.equal(a, b) for a, b in zip(p_n, p_z))


def test_evaluation_call_logs_the_lm_reward():
    host, dev, grams, sos, eos = lm_set()
    o_h, r_h, _, _ = _run('fact', host, 0.1, 'host', training=False)
    o_d, r_d, _, _ = _run('fact', host, 0.1, 'device', training=False)
    assert 'lm_reward' in o_d and o_h == o_d and torch.equal(r_h, r_d)


def test_grouped_iteration_with_the_lm_reward_raises():
    fact, senti, scs, _ = _data()
    det = _detector()
    det.set_lms(lm_set()[0])
    det.lm_flag, det.rl_samples_per_image = 0.1, 2
    with pytest.raises(ValueError, match='rl_samples_per_image'):
        det((fact, scs), 'fact', True)
    det.lm_flag = 0.0                                                     # without the term the grouped iteration runs
    assert 'sample_score' in det((fact, scs), 'fact', True)
    _give_back(det)


def test_caption_perplexity_and_eval_ppl(tmp_path):
    host, dev, grams, sos, eos = lm_set()
    det = _detector()
    det.set_lms(host)
    rows, labels = random_rows(40, TN, seed=21)
    want = rewards.lm_perplexity(*host.score(rows, labels), labels)
    d_rows, d_labels = torch.from_numpy(rows).to(DEV), torch.from_numpy(labels).to(DEV)
    assert det.caption_perplexity(d_rows, d_labels) == want               # device_cider off: the host scorer
    det.device_cider = True
    assert det.caption_perplexity(d_rows, d_labels) == want and det._lms_dev is not None      # on the device: the same bits
    assert all(1 < want[l]['ppl'] < want[l]['ppl1'] for l in range(3))
    _give_back(det)
    prefix = str(tmp_path / 'result_0')
    for lab, senti in enumerate(synth.SENTIMENT_CATEGORIES):
        with open('%s_%s_senti.txt' % (prefix, senti), 'w') as f:
            for r in rows[labels == lab]:
                f.write(' '.join(str(w) for w in R.normalise(r, sos, eos)) + '\n')
    got = train.eval_ppl(prefix, 'senti', host, sentis=synth.SENTIMENT_CATEGORIES)
    assert got == {s: want[l]['ppl'] for l, s in enumerate(synth.SENTIMENT_CATEGORIES)}
