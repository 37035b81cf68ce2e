"""The sentiment-word reward above the kernel (tests/test_gpu_sw_reward_kernels.py holds the kernel alone to the
restatement): iterations of a Detector (one of the width sets of tests/_widths.py) with senti_words_flag = 0.05 - 'host'
form against 'device' form in bits ('fact' and 'senti', training and evaluation, the decayed lexicon), against flag 0 (the
rewards differ by exactly flag x the restated term), grouped and constrained iterations against the same iteration with the
term added by the torch expression, graph-served iterations against the same phases run eagerly, flag 0 with a lexicon
against no lexicon, senti_word_stats and the refusals.  pytest -m gpu."""
import copy

import numpy as np
import pytest
import torch

import _sw_ref as S
import _widths as W
from insenticap_model_amd import dp, rewards, synth
from test_gpu_rl_graph import force_draws

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
V, TN, B = W.V, W.T, 5
ST = dict(W.H_768, **synth.HELPER_SETTINGS)
FLAG = 0.05
_cache = {}


def lexicon():
    """Three lexicons of 100 of the V words each (the ids of <PAD>, <SOS>, <EOS> among them or not, as the draw has it),
    word 17 in all three with different weights; weights 0.9 ** k by repeated multiplication."""
    rng = np.random.default_rng(31)
    pw = S.powers(0.9, 4)
    lex = {lab: {int(w): pw[int(rng.integers(0, 4))] for w in rng.choice(V, size=100, replace=False)} for lab in range(3)}
    for lab in range(3):
        lex[lab][17] = pw[lab]
    return lex


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


def _detector(graphs=False):
    from insenticap_model_amd.detector import Detector
    from test_detector import load_helper
    torch.manual_seed(0)
    det = Detector(W.idx2word(), TN, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-4}, ST)
    det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, ST, seed=W.WIDTHS['h_768']['wseed']).items()})
    load_helper(det.senti_detector, 51)
    load_helper(det.sent_senti_cls, 52)
    det = det.to(DEV)
    det.set_ciderd_scorer(_data()[3])
    det.train_graphs = graphs
    return det


def _restated(seq, labels, lex):
    """The float32 term of rows on the device, from the numpy restatement."""
    weights, state = S.table(lex, V, 3)
    r64 = S.reward(seq.cpu().numpy(), labels.cpu().numpy(), weights, state)[1]
    return torch.from_numpy(r64).float().to(DEV)


def _run(data_type, lex, flag, form='device', training=True, calls=1, inject=None, n_rl=1, constraints=None):
    """`calls` forward() calls of one eager iteration each on a fresh detector -> (loss dictionaries, the rewards handed
    to the RL criterion, parameters, the lexicon afterwards, the sampled rows and their labels).  `inject`: flag 0 in the
    detector, and the term - restated in numpy from the sampled rows - added to the rewards by the torch expression in
    front of the criterion."""
    fact, senti, scs, _ = _data()
    det = _detector()
    lex = copy.deepcopy(lex)
    if lex is not None:
        det.set_sentiment_words(lex)
    det.senti_words_flag, det.senti_words_form = flag, form
    det.rl_samples_per_image, det.rollout_constraints = n_rl, constraints
    seen, rolled = [], []
    crit, roll = det.cap_rl_crit.forward, det.captioner.forward_rl

    def spy_rl(*a, **k):
        out = roll(*a, **k)
        if not k.get('sample_max', 1):
            lab = a[4].repeat_interleave(k.get('captions_per_image', 1))
            rolled.append((out[0].detach().clone(), lab.detach().clone()))
        return out

    def spy(logp, masks, reward):
        if inject is not None:
            reward = reward + inject * _restated(*rolled[-1], lex)
        seen.append(reward.detach().clone())
        return crit(logp, masks, reward)
    det.captioner.forward_rl, det.cap_rl_crit.forward = spy_rl, spy
    torch.manual_seed(1234)
    torch.cuda.manual_seed_all(1234)
    items = fact if data_type == 'fact' else senti
    outs = [det((items, scs) if training else (items,), data_type, training) for _ in range(calls)]
    torch.cuda.synchronize()
    assert det._rl_graph is None and len(seen) == calls == len(rolled)
    params = [p.detach().clone() for p in det.captioner.parameters()]
    _give_back(det)
    return outs, seen, params, lex, rolled


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize('data_type', ['fact', 'senti'])
def test_host_form_against_device_form_and_against_flag_zero(data_type):
    lex = lexicon()
    o_h, r_h, p_h, l_h, s_h = _run(data_type, lex, FLAG, 'host', calls=2)
    o_d, r_d, p_d, l_d, s_d = _run(data_type, lex, FLAG, 'device', calls=2)
    print('SW detector %s: host %r device %r' % (data_type, o_h, o_d))
    assert o_h == o_d and all('senti_words_reward' in o and list(o) == list(q) for o, q in zip(o_h, o_d))
    assert same_bits(r_h, r_d) and same_bits(p_h, p_d)
    assert l_h == l_d and l_h != lex and l_h.keys() == lex.keys() and all(l_h[k].keys() == lex[k].keys() for k in lex)
    # the words the first call paid are paid 0.9 x as much in the second: the loop of decoder.py:174-176 on the restatement
    loop = copy.deepcopy(lex)
    for call, (seq, labels) in enumerate(s_d):
        weights, state = S.table(loop, V, 3)
        r32, r64, hits, after = S.reward(seq.cpu().numpy(), labels.cpu().numpy(), weights, state)
        assert o_d[call]['senti_words_reward'] == float(torch.from_numpy(r32).to(DEV).sum()) / 2 and hits.sum() > 0
        for lab, ws in S.accur(state, after).items():
            for w in ws:
                loop[lab][w] *= 0.9
    assert l_d == loop
    # against flag 0: the same rows (the term draws no random numbers), rewards apart by exactly flag x the term
    o_0, r_0, p_0, l_0, s_0 = _run(data_type, lex, 0.0)
    assert 'senti_words_reward' not in o_0[0] and l_0 == lex and torch.equal(s_0[0][0], s_d[0][0])
    term = _restated(*s_d[0], lex)
    assert torch.equal(r_d[0], r_0[0] + FLAG * term) and float(term.abs().sum()) > 0
    for row in range(term.shape[0]):
        assert torch.equal(r_d[0][row] - r_0[0][row], (r_0[0][row] + FLAG * term[row]) - r_0[0][row])
    assert not same_bits(p_0, p_d)


def test_flag_zero_with_a_lexicon_changes_nothing():
    o_n, r_n, p_n, _, _ = _run('fact', None, 0.0)
    o_z, r_z, p_z, l_z, _ = _run('fact', lexicon(), 0.0)
    assert o_n == o_z and list(o_n[0]) == list(o_z[0]) and 'senti_words_reward' not in o_z[0]
    assert same_bits(r_n, r_z) and same_bits(p_n, p_z) and l_z == lexicon()


@pytest.mark.parametrize('data_type', ['fact', 'senti'])
def test_evaluation_call_logs_the_term_and_decays(data_type):
    lex = lexicon()
    o_h, r_h, _, l_h, _ = _run(data_type, lex, FLAG, 'host', training=False)
    o_d, r_d, _, l_d, s_d = _run(data_type, lex, FLAG, 'device', training=False)
    assert 'senti_words_reward' in o_d[0] and o_h == o_d and same_bits(r_h, r_d)
    assert l_h == l_d and l_d != lex                        # (decoder.py:174-176 has no `training` condition)
    assert o_d[0]['senti_words_reward'] == float(_restated(*s_d[0], lex).sum())       # (len((loader,)) == 1)


@pytest.mark.parametrize('kind', ['grouped', 'constrained'])
def test_grouped_and_constrained_iterations_equal_the_torch_expression(kind):
    kw = dict(n_rl=2) if kind == 'grouped' else \
        dict(constraints=dict(suppress_special=True, decoding_constraint=1, min_len=3))
    lex = lexicon()
    o_d, r_d, p_d, l_d, s_d = _run('fact', lex, FLAG, 'device', **kw)
    o_i, r_i, p_i, l_i, s_i = _run('fact', lex, 0.0, inject=FLAG, **kw)
    assert s_d[0][0].shape[0] == (2 * B if kind == 'grouped' else B) and torch.equal(s_d[0][0], s_i[0][0])
    assert same_bits(r_d, r_i) and same_bits(p_d, p_i) and l_d != lex and l_i == lex
    assert o_d[0]['senti_words_reward'] == float(_restated(*s_d[0], lex).sum()) / 2
    assert o_d[0]['all_rewards'] == float(r_d[0].mean(-1).mean(-1)) / 2           # from the final tensor
    for k in o_i[0]:
        if k != 'all_rewards':
            assert o_d[0][k] == o_i[0][k], k
    o_h, r_h, p_h, l_h, _ = _run('fact', lex, FLAG, 'host', **kw)
    assert o_h == o_d and same_bits(r_h, r_d) and same_bits(p_h, p_d) and l_h == l_d


# ------------------------------------------------------------------------------------------------ graph-served
def _serve(lex, flag, warmup, n_iter=5):
    """n_iter forward() calls of one training iteration each through RLTrainGraph (forced draws, scheduled sampling off:
    no random numbers, as tests/test_gpu_rl_graph.py compares) on a fresh detector -> its loss dictionaries, lexicon
    afterwards, sampled rows of the eager iterations, graph counters and parameters; the detector's streams are given back."""
    from insenticap_model_amd.train_graph import RLTrainGraph
    fact, senti, scs, _ = _data()
    det = _detector(graphs=True)
    lex = copy.deepcopy(lex)
    if lex is not None:
        det.set_sentiment_words(lex)
    det.senti_words_flag = flag
    det.xe_ss_prob = det.seq2seq_ss_prob = 0.0
    draws = [np.random.default_rng(80).integers(2, V, size=(B, TN), dtype=np.int64)]
    det._rl_graph = RLTrainGraph(det, warmup=warmup)
    roll, det._test_rolled = det.captioner.forward_rl, []

    def spy_rl(*a, **k):                                   # the sampled rows and their labels of every eager iteration
        out = roll(*a, **k)
        if not k.get('sample_max', 1) and not torch.cuda.is_current_stream_capturing():
            det._test_rolled.append((out[0].detach().clone(), a[4].detach().clone()))
        return out
    det.captioner._orig_forward_rl = spy_rl                # (force_draws wraps this one)
    outs = []
    try:
        for i in range(n_iter):
            force_draws(det, draws)
            outs.append(det((fact, scs), 'fact', True))
        torch.cuda.synchronize()
        g = det._rl_graph
        return dict(outs=outs, lex=lex, rolled=det._test_rolled, keys=set(g.KEYS),
                    counts=(g.captures, g.replays, g.eager_steps),
                    params={k: p.detach().clone() for k, p in det.captioner.named_parameters()})
    finally:
        _give_back(det)                                    # (one graph object's streams at a time)


def test_graph_served_iterations_with_the_term_equal_the_eager_phases():
    lex = lexicon()
    g = _serve(lex, FLAG, 2)
    e = _serve(lex, FLAG, 10 ** 6)
    z = _serve(lex, 0.0, 2)
    n = _serve(None, 0.0, 2)
    og, oe = g['outs'], e['outs']
    # served from graphs, as without the term: (captures, replays, eager steps)
    assert g['counts'] == (1, 3, 2) and e['counts'] == (0, 0, 5) and z['counts'] == (1, 3, 2) == n['counts']
    for k in g['params']:
        assert torch.equal(g['params'][k], e['params'][k]), k
    for a, b in zip(og, oe):
        assert a.keys() == b.keys() == g['keys'] | {'senti_words_reward'}
        for k in a:
            assert a[k] == b[k], k
    # five end-of-call decays (decoder.py:174-176) and the logged sums, restated from the rows of the eager phases
    assert g['lex'] == e['lex'] and g['lex'] != lex and len(e['rolled']) == 5 and len(g['rolled']) == 2
    loop = copy.deepcopy(lex)
    for call, (seq, labels) in enumerate(e['rolled']):
        weights, state = S.table(loop, V, 3)
        r32, _, hits, after = S.reward(seq.cpu().numpy(), labels.cpu().numpy(), weights, state)
        assert og[call]['senti_words_reward'] == float(torch.from_numpy(r32).to(DEV).sum()) / 2 and hits.sum() > 0
        for lab, ws in S.accur(state, after).items():
            for w in ws:
                loop[lab][w] *= 0.9
    assert g['lex'] == loop
    # flag 0 with a lexicon: today's keys, today's bits, the lexicon untouched
    assert z['outs'] == n['outs'] and all(o.keys() == z['keys'] for o in z['outs']) and z['lex'] == lex
    for k in z['params']:
        assert torch.equal(z['params'][k], n['params'][k]), k
    assert any(not torch.equal(g['params'][k], z['params'][k]) for k in g['params'])


# ------------------------------------------------------------------------------------------------ metric, refusals
def test_senti_word_stats_equals_the_restatement():
    lex = lexicon()
    table = rewards.SentimentWordWeights.from_dict(lex, V, 3, DEV)
    rng = np.random.default_rng(7)
    tok = rng.integers(0, V, size=(41, TN)).astype(np.int64)
    tok[3] = 17
    labels = rng.integers(0, 3, size=41).astype(np.int64)
    before = (table.weights.clone(), table.state.clone())
    got = rewards.senti_word_stats(torch.from_numpy(tok).to(DEV), torch.from_numpy(labels).to(DEV), table)
    want = S.stats(tok, labels, *S.table(lex, V, 3))
    assert got == want and sum(v['captions'] for v in got.values()) == 41 and all(v['distinct'] > 3 for v in got.values())
    assert all(0 < v['with_word'] <= v['captions'] and v['hits'] >= v['with_word'] for v in got.values())
    assert torch.equal(before[0], table.weights) and torch.equal(before[1], table.state)      # a scratch copy is marked


def test_refusals(monkeypatch):
    fact, senti, scs, _ = _data()
    det = _detector()
    det.senti_words_flag = FLAG
    with pytest.raises(ValueError, match='set_sentiment_words'):
        det((fact, scs), 'fact', True)
    lex = lexicon()
    det.set_sentiment_words(lex)
    monkeypatch.setattr(dp, 'distributed', lambda group=None: True)
    det.dp_arena = object()
    with pytest.raises(ValueError, match='not built'):
        det((fact, scs), 'fact', True)
    monkeypatch.undo()
    det.dp_arena = None
    assert lex == lexicon()
    # the table follows the dict OBJECT: a replaced dict is built anew
    t0 = det._device_sw(DEV)
    assert det._device_sw(DEV) is t0
    det.set_sentiment_words(lexicon())
    assert det._device_sw(DEV) is not t0
    _give_back(det)
