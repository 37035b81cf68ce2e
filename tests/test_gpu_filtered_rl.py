"""Self-critical RL under temperature / top-k / nucleus sampling: the differentiable filtered roll-out
(`forward_rl(..., sample_max=0, temperature / top_k / top_p)` with gradients enabled) against the float64 reference
roll-out of tests/_filtered_rl_ref.py, and `Detector.rollout_sampling`.

The cases, their uniforms and their CPU facts (same kept sets in fp32 and fp64, no draw near a CDF boundary) are those of
tests/test_filtered_rl_host.py: nothing is skipped or relaxed here.  Bars: those of tests/test_gpu_group_rl.py."""
import numpy as np
import pytest
import torch

import _filtered_rl_ref as FR
import test_gpu_filtered_bwd_kernel as K
from insenticap_model_amd import Captioner, _lib, ops, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GRAD_RTOL = 1e-4
INPUTS = ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')
V, I, T = FR.V, FR.I, FR.T


def _captioner(p_drop):
    st = synth.TINY_SETTINGS
    cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, dict(st, dropout_p=p_drop))
    cap.load_state_dict({k: torch.from_numpy(x) for k, x in FR.case_weights().items()})
    cap.to(DEV)
    cap.train()
    return cap


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _loss(lp, slp, mk, reward, mix):
    """REINFORCE on the sampling log-probs (mix: plus half the model's) with a fixed reward."""
    term = slp + 0.5 * lp if mix else slp
    return -(term * mk * reward).sum() / mk.sum()


def _hip_run(cap, name, n, with_masks, reward, mix=False, da=True, **over):
    b, u, masks = FR.case_inputs(name, n, with_masks)
    kw = dict(FR.CONTROLS[name], _uniforms=_dev(u), return_sampling_logprobs=True, _masks=masks)
    if n > 1:
        kw['captions_per_image'] = n
    kw.update(over)
    cap.zero_grad()
    seq, lp, mk, slp = cap.forward_rl(*[_dev(b[k]) for k in INPUTS], T, 0, **kw)
    assert lp.requires_grad and slp.requires_grad
    rl = _loss(lp, slp, mk, reward, mix)
    dal = torch.nn.MSELoss()(cap.cpt_feats, cap.fc_feats.detach()) if da else torch.zeros((), device=DEV)
    (rl + dal).backward()
    grads = {k: q.grad.detach().cpu().numpy().copy() for k, q in cap.named_parameters() if q.grad is not None}
    return dict(seq=seq.cpu().numpy(), lp=lp.detach().cpu().numpy(), slp=slp.detach().cpu().numpy(), mk=mk.cpu().numpy(),
                losses=(float(rl.detach()), float(dal.detach())), grads=grads)


_ORACLE = {}


def _oracle_run(name, n, with_masks, reward, mix=False):
    """The float64 reference of one case (computed once, shared by both engines)."""
    key = (name, n, with_masks, mix)
    if key not in _ORACLE:
        from oracle import captioner_oracle as O
        p, o = FR.oracle_case(name, n, with_masks)
        rl = _loss(o['lp'], o['slp'], o['mk'], reward.double(), mix)
        da = O.domain_align_loss(o['P'].cpt, o['P'].fc_raw)
        (rl + da).backward()
        _ORACLE[key] = dict(seq=o['seq'].numpy(), lp=o['lp'].detach().numpy(), slp=o['slp'].detach().numpy(),
                            mk=o['mk'].numpy(), losses=(float(rl.detach()), float(da.detach())), steps=o['steps'],
                            grads={k: q.grad.numpy() for k, q in p.items() if q.grad is not None})
    return _ORACLE[key]


def _compare(got, ref, what, min_grads=36):
    assert np.array_equal(got['seq'], ref['seq']) and np.array_equal(got['mk'], ref['mk']), what
    np.testing.assert_allclose(got['lp'], ref['lp'], atol=1e-4, err_msg=what)
    np.testing.assert_allclose(got['slp'], ref['slp'], atol=1e-4, err_msg=what)
    np.testing.assert_allclose(got['losses'], ref['losses'], rtol=5e-5, err_msg=what)
    for k, r in ref['grads'].items():
        assert k in got['grads'], (what, k)
        np.testing.assert_allclose(got['grads'][k], r, atol=GRAD_RTOL * np.abs(r).max() + 1e-7, err_msg='%s %s' % (what, k))
    assert len(ref['grads']) >= min_grads and set(got['grads']) == set(ref['grads']), what


def _reward(n):
    return torch.randn(I * n, T, generator=torch.Generator().manual_seed(10 + n))


@pytest.mark.parametrize('mode', [1, 0], ids=['split_f16', 'exact_fp32'])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('name', list(FR.CONTROLS))
def test_filtered_rl_gradients_vs_float64_reference(name, n, mode):
    """'tiny' settings, V = 64, I = 3, R = 6, T = 8, `_uniforms` fixed; dropout off and explicit masks.  REINFORCE on the
    SAMPLING log-probs with a random reward plus the domain-alignment loss: tokens and masks equal the reference's, both
    log-prob tensors within 1e-4 (zero behind the early break), losses within rtol 5e-5, every parameter gradient within
    1e-4 max|ref| + 1e-7, the oracle's parameter set."""
    reward = _reward(n)
    prev = ops.h3_mode()
    ops.set_h3_mode(mode)
    try:
        for with_masks in (False, True):
            cap = _captioner(synth.TINY_SETTINGS['dropout_p'] if with_masks else 0.0)
            got = _hip_run(cap, name, n, with_masks, reward.to(DEV))
            ref = _oracle_run(name, n, with_masks, reward)
            what = '%s n=%d engine=%d masks=%d' % (name, n, mode, with_masks)
            assert (got['slp'][:, ref['steps']:] == 0).all() and (got['lp'][:, ref['steps']:] == 0).all(), what
            _compare(got, ref, what)
    finally:
        ops.set_h3_mode(prev)


@pytest.mark.parametrize('mode', [1, 0], ids=['split_f16', 'exact_fp32'])
def test_a_loss_that_mixes_model_and_sampling_logprobs(mode):
    """loss = REINFORCE on (log q + 0.5 log p): both terms enter d logits in the one launch."""
    name, n = 'k8_p0.9_cons', 3
    reward = _reward(n)
    prev = ops.h3_mode()
    ops.set_h3_mode(mode)
    try:
        got = _hip_run(_captioner(0.0), name, n, False, reward.to(DEV), mix=True)
        _compare(got, _oracle_run(name, n, False, reward, mix=True), 'mixed engine=%d' % mode)
    finally:
        ops.set_h3_mode(prev)


def test_top_k_1_has_zero_classifier_gradients_from_the_rl_term():
    """With one id kept log q(token) = 0 whatever the logits: its d logits are exactly zero, and so is everything behind."""
    got = _hip_run(_captioner(0.0), 'k5', 3, False, _reward(3).to(DEV), da=False, top_k=1)
    assert (np.abs(got['slp']) <= 2.0 ** -23).all()          # (log q = 0 up to the fixed-point mass of the one kept id)
    assert set(got['grads']) >= {'classifier.weight', 'classifier.bias'}
    for k, g in got['grads'].items():
        assert (g == 0).all(), k


def _launch_counts():
    lib = _lib.load()
    return {k: getattr(lib, k)() for k, (_, args) in _lib.SIGNATURES.items() if k.endswith('_launches') and not args}


def test_default_controls_with_gradients_are_todays_call_in_bits_and_launches():
    """temperature = 1, top_k = 0, top_p = 1 spelled out: the outputs, the gradients and the library's launch counters of
    the call without them."""
    b, _, _ = FR.case_inputs('k5', 3, False)
    cap = _captioner(synth.TINY_SETTINGS['dropout_p'])
    reward = _reward(3).to(DEV)
    runs = []
    for kw in (dict(), dict(temperature=1.0, top_k=0, top_p=1.0)):
        torch.manual_seed(77)
        torch.cuda.manual_seed_all(77)
        cap.zero_grad()
        before = _launch_counts()
        out = cap.forward_rl(*[_dev(b[k]) for k in INPUTS], T, 0, captions_per_image=3, **kw)
        assert len(out) == 3
        seq, lp, mk = out
        (-(lp * mk * reward).sum() / mk.sum()).backward()
        torch.cuda.synchronize()
        after = _launch_counts()
        runs.append((seq.cpu(), lp.detach().cpu(), mk.cpu(), {k: q.grad.cpu().clone() for k, q in cap.named_parameters() if q.grad is not None},
                     {k: after[k] - before[k] for k in after}))
    a, c = runs
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and torch.equal(a[2], c[2])
    assert all(torch.equal(a[3][k], c[3][k]) for k in a[3]) and a[4] == c[4]
    assert a[4]['isc_rollout_finalize_launches'] > 0


def test_two_filtered_calls_give_equal_gradient_bits():
    cap = _captioner(0.0)
    reward = _reward(3).to(DEV)
    a, c = (_hip_run(cap, 'k8_p0.9_cons', 3, False, reward, mix=True) for _ in range(2))
    assert np.array_equal(a['slp'], c['slp']) and a['losses'] == c['losses'] and len(a['grads']) >= 36
    for k, g in a['grads'].items():
        assert np.array_equal(g, c['grads'][k]), k


def test_the_filtered_backward_call_is_graph_capturable():
    """One capture of isc_logsoftmax_bwd_raw_filtered into a HIP graph; a replay on other coefficients gives the eager bits."""
    Vk, tau, B, T_ = 200, 0.7, 3, 4
    x, rows = K.make_rows(Vk, tau, seed=5)
    ks, gm, lz, ban = K.saved(x, rows, tau)
    pm, ps = K.tile_stats(np.nan_to_num(x))
    _, raw, ld_b, ld_t, pmd, psd, srows = next(K.layouts(x, B, T_, pm, ps))
    rng = np.random.default_rng(0)
    pairs = [(K.dv(rng.integers(0, Vk, size=B * T_).astype(np.int64)), K.dv(rng.standard_normal(B * T_).astype(np.float32)))]
    coef_a, coef_b = (K.dv(rng.standard_normal(B * T_).astype(np.float32)) for _ in range(2))
    flt = dict(tok=K.dv(np.array([r['tok'] for r in rows], np.int64)), coef=coef_a.clone(), inv_tau=1.0 / tau,
               kstar=K.dv(ks), gmax=K.dv(gm), logz=K.dv(lz), ban=K.dv(ban))
    out = torch.zeros(B * T_, K.pad32(Vk), device=DEV)

    def call(o):
        ops.logsoftmax_bwd_raw_filtered(raw, ld_b, ld_t, B, T_, Vk, pmd, psd, srows, pairs, flt, o)
    eager = []
    for c in (coef_a, coef_b):
        flt['coef'].copy_(c)
        o = torch.zeros_like(out)
        call(o)
        eager.append(o)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        call(out)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            call(out)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    for c, want in ((coef_a, eager[0]), (coef_b, eager[1])):
        flt['coef'].copy_(c)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------------------------------------ Detector
def _detector(Vd, TN, st):
    from insenticap_model_amd.detector import Detector
    from test_detector import load_helper
    det = Detector(synth.make_idx2word(Vd), TN, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-4}, st)
    det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(Vd, st, seed=3).items()})
    load_helper(det.senti_detector, 51)
    load_helper(det.sent_senti_cls, 52)
    # (a captioner that has served a greedy roll-out from a HIP graph keeps one of the device's 32 pool streams; these
    # tests are not about that route, and the suite is long enough to run out of streams)
    det.captioner.enable_rollout_graphs(False)
    return det.to(DEV)


def _loaders(data_type, Vd=64, TN=8, B=4):
    st = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
    batches, split = synth.make_rl_batches(2, B, Vd, st, seq_len=TN, seed=70)
    t = torch.from_numpy
    if data_type == 'fact':
        items = [(b[0], t(b[1]), t(b[2]), (t(b[3][0]), b[3][1]), t(b[4]), t(b[5]), b[6]) for b in batches]
    else:
        rng = np.random.default_rng(5)
        items = [(b[0], t(b[1]), t(b[2]), t(b[4]), t(b[5]),
                  t(rng.integers(0, len(synth.SENTIMENT_CATEGORIES), size=B).astype(np.int64))) for b in batches]
    s = synth.make_inputs(4, Vd, st, regions=6, seq_len=TN, seed=72)
    scs = [((t(s['captions']), s['lengths']), t(s['cpt_words']), t(s['senti_words']), t(s['senti_labels']))]
    return st, items, scs, split


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('data_type', ['fact', 'senti'])
def test_detector_trains_under_rollout_sampling(data_type, n):
    """One training call over two tiny batches with rollout_sampling = (temperature 0.8, top_p 0.9): the sampled roll-out
    gets the controls and returns the sampling log-probs (a wrapper on forward_rl sees it), the greedy baseline does not,
    the iteration runs eagerly, the logged keys are today's, every value is finite and the parameters change."""
    Vd, TN, B = 64, 8, 4
    st, items, scs, split = _loaders(data_type, Vd, TN, B)
    torch.manual_seed(0)
    det = _detector(Vd, TN, st)
    det.set_ciderd_scorer(split)
    det.rollout_sampling = dict(temperature=0.8, top_p=0.9)
    det.rl_samples_per_image = n
    ops.device_status(reset=True)      # (status words an earlier test's non-finite inputs left set would cost a retry)
    seen = []
    orig = det.captioner.forward_rl

    def spy(*args, **kw):
        out = orig(*args, **kw)
        seen.append((kw.get('sample_max'), kw.get('temperature'), kw.get('top_p'), len(out),
                     bool(out[-1].requires_grad) if kw.get('sample_max') == 0 else None))
        return out
    det.captioner.forward_rl = spy
    before = {k: v.detach().clone() for k, v in det.captioner.state_dict().items()}
    out = det((items, scs), data_type, True)
    torch.cuda.synchronize()
    assert det._rl_graph is None
    sampled = [s for s in seen if s[0] == 0]
    assert sampled == [(0, 0.8, 0.9, 4, True)] * 2
    assert [s for s in seen if s[0] == 1] == ([(1, None, None, 3, None)] * 2 if n == 1 else [])
    want = {'da_loss', 'cls_reward', 'all_rewards', 'cap_loss', 'seq2seq_loss'}       # (today's keys, per form)
    if n > 1:
        want |= {'sample_score', 'fact_reward'}
    if data_type == 'fact':
        want |= {'xe_loss', 'fact_reward'}
    assert set(out) == want
    assert all(np.isfinite(v) for v in out.values()), out
    after = det.captioner.state_dict()
    assert len([k for k in before if not torch.equal(before[k], after[k])]) >= 36
    # evaluation is untouched: no controls on its sampled roll-out
    del seen[:]
    det((items,), data_type, False)
    assert all(s[1] is None and s[3] == 3 for s in seen) and len(seen) == 4


def test_detector_all_default_rollout_sampling_is_none_and_bad_keys_raise():
    st, items, scs, split = _loaders('fact')
    runs = []
    for rs in (None, dict(temperature=1.0, top_k=0, top_p=1.0)):
        torch.manual_seed(0)
        torch.cuda.manual_seed_all(0)
        det = _detector(64, 8, st)
        det.set_ciderd_scorer(split)
        det.rollout_sampling = rs
        ops.device_status(reset=True)
        out = det((items, scs), 'fact', True)
        torch.cuda.synchronize()
        runs.append((out, {k: v.detach().cpu().clone() for k, v in det.captioner.state_dict().items()},
                     det._rl_graph is not None))
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2]
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
    det = _detector(64, 8, st)
    det.set_ciderd_scorer(split)
    for bad in (dict(temperatur=0.8), dict(top_p=0.9, min_len=2)):
        det.rollout_sampling = bad
        with pytest.raises(ValueError, match='rollout_sampling'):
            det((items, scs), 'fact', True)
    det.rollout_sampling = dict(temperature=-1.0)
    with pytest.raises(ValueError):
        det((items, scs), 'fact', True)
