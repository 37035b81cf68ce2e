"""Every captioner path at layer widths that differ from each other (tests/_widths.py), against the CPU oracle in fp64.

Every other end-to-end test builds its model with W = E = H = A, where a wrong symbol in the plumbing above the kernels
(a buffer sized A where E is read, a leading dimension H where H + E + W is meant, Wih[:, H + E:] cut one term short)
cannot be seen.  Here: teacher-forced forwards (a), the XE training iteration on both unroll forms (b), the same with
explicit dropout masks (c), greedy roll-outs on the general kernels, the fused gate and the few-row step, from the
roll-out graph too (d), the sampled roll-out's gradients (e), beam searches eagerly and from their graphs (f) and the
grouped sampled roll-out (g).  The bounds are the project's: log-probs 1e-4 (test_gpu_parity.LOGP_TOL), gradients
1e-4 of the tensor's max and post-Adam parameters (test_gpu_train_sizes._compare, not widened), tokens, masks and beams
exact - test_widths_host.py asserts on the CPU that no step of these roll-outs is a near-tie.  The last test prints
each path's worst error as a fraction of its bound.  pytest -m gpu."""
import numpy as np
import pytest
import torch

import _widths as Wd
from conftest import trusted_prefix
from insenticap_model_amd import Captioner, RewardCriterion, ops, synth
from test_gpu_group_rollout import _assert_replay_forms_agree, _both_forms
from test_gpu_parity import LOGP_TOL
from test_gpu_train_sizes import GRAD_RTOL, _compare, _hip_iteration, _oracle_iteration

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
W_TOL = 1e-5                 # attention weights, fc_feats / cpt_feats: the bound of test_gpu_parity's end-to-end tests
BEAM_SCORE_TOL = 1e-3        # test_beam5_batch64_matches_per_image_and_oracle
T = Wd.T
RATIOS = {}                  # (width set, path) -> worst error / bound
_caps, _memo = {}, {}


def _note(name, path, err, bound):
    RATIOS[(name, path)] = max(RATIOS.get((name, path), 0.0), float(err) / bound)


def _close(name, path, got, ref, tol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, path, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if got.size else 0.0
    _note(name, path, err, tol)
    assert err <= tol, (name, path, err, tol)


def _cap(name):
    if name not in _caps:
        st, w, _, _ = Wd.setup(name)
        cap = Captioner(Wd.idx2word(), synth.SENTIMENT_CATEGORIES, st)
        cap.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
        _caps[name] = cap.to(DEV).eval()
    return _caps[name]


def _dev(d, key, rows=None):
    return Wd.cpu(d, key, rows).to(DEV)


def _n():
    return ops._lib.load().isc_rows_launches()


@pytest.fixture
def h3_mode():
    prev = ops.h3_mode()
    yield ops.set_h3_mode
    ops.set_h3_mode(prev)


def _oracle_forward(name, which):
    key = ('fwd', name, which)
    if key not in _memo:
        from oracle import captioner_oracle as O
        st, w, d, s2s = Wd.setup(name)
        p, f64 = O.to_params(w, dtype=torch.float64), torch.float64
        with torch.no_grad():
            if which == 'xe':
                _memo[key] = O.forward_xe(p, Wd.oracle_ids(), Wd.cpu(d, 'fc_feats', dtype=f64), Wd.cpu(d, 'att_feats', dtype=f64),
                                          Wd.cpu(d, 'cpt_words'), Wd.cpu(d, 'captions'), Wd.cpu(d, 'senti_labels'))
            else:
                _memo[key] = O.forward_seq2seq(p, Wd.oracle_ids(), Wd.cpu(s2s, 'captions'), Wd.cpu(s2s, 'cpt_words'),
                                               Wd.cpu(s2s, 'senti_words'), Wd.cpu(s2s, 'senti_labels'))
    return _memo[key]


def _oracle_iter(name):
    key = ('iter', name)
    if key not in _memo:
        st, w, d, s2s = Wd.setup(name)
        _memo[key] = _oracle_iteration(w, Wd.V, d, s2s, dtype=torch.float64)
    return _memo[key]


# ----------------------------------------------------------------------------- a. teacher-forced forwards
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('name', Wd.SMALL)
def test_a_teacher_forced_forwards(name, mode, h3_mode):
    st, w, d, s2s = Wd.setup(name)
    cap = _cap(name)
    h3_mode(mode)
    path = 'a forward h3=%d' % mode
    with torch.no_grad():
        logp = cap.forward_xe(_dev(d, 'fc_feats'), _dev(d, 'att_feats'), _dev(d, 'cpt_words'), _dev(d, 'captions'),
                              _dev(d, 'senti_labels'), 0.0)
    ologp, P, ow = _oracle_forward(name, 'xe')
    assert logp.shape == (Wd.B, T, Wd.V)
    _close(name, path + ' logp', logp.cpu(), ologp, LOGP_TOL)
    _close(name, path + ' weights', cap.cont_weights.cpu(), ow[0], W_TOL)
    assert cap.senti_weights == [] and cap.cont_senti_weights == [] and ow[1] == [] and ow[2] == []
    _close(name, path + ' feats', cap.fc_feats.cpu(), P.fc_raw, W_TOL)
    _close(name, path + ' feats', cap.cpt_feats.cpu(), P.cpt, W_TOL)
    with torch.no_grad():
        logp2 = cap.forward_seq2seq(_dev(s2s, 'captions'), _dev(s2s, 'cpt_words'), _dev(s2s, 'senti_words'),
                                    _dev(s2s, 'senti_labels'), 0.0)
    ologp2, P2, ow2 = _oracle_forward(name, 's2s')
    assert logp2.shape == (Wd.S2S_B, T, Wd.V)
    _close(name, path + ' logp', logp2.cpu(), ologp2, LOGP_TOL)
    _close(name, path + ' weights', cap.senti_weights.cpu(), ow2[1], W_TOL)
    assert cap.cont_weights == [] and cap.cont_senti_weights == [] and ow2[0] == [] and ow2[2] == []
    _close(name, path + ' feats', cap.cpt_feats.cpu(), P2.cpt, W_TOL)


# ----------------------------------------------------------------------------- b. / c. one XE training iteration
def _note_grads(name, path, worst):
    assert len(worst) >= 28, sorted(worst)             # (the rest: softmax-shift-invariant biases, true gradient 0)
    for k, (err, tol) in worst.items():
        assert tol == GRAD_RTOL, (k, tol)
        _note(name, path, err, tol)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('pair', [True, False], ids=['pair', 'two_calls'])
@pytest.mark.parametrize('name', Wd.SMALL)
def test_b_xe_training_iteration(name, pair, mode, h3_mode):
    st, w, d, s2s = Wd.setup(name)
    h3_mode(mode)
    hip = _hip_iteration(w, Wd.V, st, d, s2s, pair=pair)
    worst = _compare(hip, _oracle_iter(name), widen=False)
    _note_grads(name, 'b iteration %s h3=%d grads' % ('pair' if pair else 'two calls', mode), worst)


@pytest.mark.parametrize('pair', [True, False, None], ids=['pair', 'two_calls_one_entry', 'two_calls'])
def test_c_training_mode_iteration_with_explicit_dropout_masks(pair):
    """The keep-mask shapes depend on E, A and H separately: fc [B,E], att [B,R,E], label [B,W], out<t> [B,H]; cpt [S,E],
    words [S,Mw,W]."""
    name = 'all_differ'
    st, w, d, s2s = Wd.setup(name)
    E, H, Wdim = st['feat_emb_dim'], st['rnn_hid_dim'], st['word_emb_dim']
    assert len({E, H, st['att_hid_dim']}) == 3
    g = torch.Generator().manual_seed(23)
    Mw = np.asarray(s2s['senti_words']).shape[1] + 1

    def keep(*shape):
        return (torch.rand(*shape, generator=g) >= st['dropout_p']).to(torch.uint8)
    om = dict(fc=keep(Wd.B, E), att=keep(Wd.B, Wd.R, E), label=keep(Wd.B, Wdim), out=keep(T, Wd.B, H))
    os_ = dict(cpt=keep(Wd.S2S_B, E), words=keep(Wd.S2S_B, Mw, Wdim), label=keep(Wd.S2S_B, Wdim), out=keep(T, Wd.S2S_B, H))

    def product_form(m):
        out = {k: v for k, v in m.items() if k != 'out'}
        out.update({'out%d' % t: m['out'][t] for t in range(T)})
        return out
    key = ('iter_masks', name)
    if key not in _memo:
        _memo[key] = _oracle_iteration(w, Wd.V, d, s2s, dtype=torch.float64, masks=om, s_masks=os_, p_drop=st['dropout_p'])
    hip = _hip_iteration(w, Wd.V, st, d, s2s, pair=pair, masks=product_form(om), s_masks=product_form(os_), train=True)
    worst = _compare(hip, _memo[key], widen=False)
    _note_grads(name, 'c dropout iteration grads', worst)
    # the masks matter: the eval-mode iteration's loss is another one
    assert abs(_memo[key][0][0] - _oracle_iter(name)[0][0]) > 1e-3


# ----------------------------------------------------------------------------- d. greedy roll-out
GREEDY = [(n, b) for n in Wd.SMALL for b in (9, 4)] + [(n, b) for n in Wd.LARGE for b in (4, 7)]


def _rl_args(d, rows):
    return [_dev(d, k, rows) for k in Wd.RL_KEYS]


def _greedy_vs_oracle(name, path, cap, out, rows, weights=True):
    seq, lp, mk = (x.cpu() for x in out)
    oseq, olp, omk, P, ow, margins = Wd.oracle_greedy(name, rows)
    n = trusted_prefix(margins.numpy(), omk.numpy(), Wd.MARGIN)
    assert (n == T).all()                              # test_widths_host.py: every live step is trusted
    assert torch.equal(seq, oseq), (name, path)
    assert torch.equal(mk.double(), omk), (name, path)
    steps = olp.shape[1]                               # (the oracle leaves its loop once every row has ended)
    _close(name, path + ' logp', lp[:, :steps], olp, LOGP_TOL)
    if weights:
        for attr, ref in zip(('cont_weights', 'senti_weights', 'cont_senti_weights'), ow):
            _close(name, path + ' weights', getattr(cap, attr).cpu(), ref, W_TOL)
        _close(name, path + ' feats', cap.fc_feats.cpu(), P.fc_raw, W_TOL)
        _close(name, path + ' feats', cap.cpt_feats.cpu(), P.cpt, W_TOL)
    return seq, lp, mk


@pytest.mark.parametrize('mode', [0, 1, 3])
@pytest.mark.parametrize('name,rows', GREEDY)
def test_d_greedy_rollout(name, rows, mode, h3_mode):
    st, w, d, _ = Wd.setup(name)
    cap = _cap(name)
    h3_mode(mode)
    eligible = Wd.WIDTHS[name]['rows_step']
    a = _rl_args(d, rows)
    path = 'd greedy B=%d h3=%d' % (rows, mode)

    def eager_first_call(tag):
        cap.enable_rollout_graphs(True)                # an empty cache: eager, capture, replay
        n0 = _n()
        with torch.no_grad():
            out = cap.forward_rl(*a, T, 1)
        torch.cuda.synchronize()
        # the route the table claims: five few-row launches per step / the row scan kernel behind the fused gate / neither
        assert _n() - n0 == ((5 * T if rows <= 8 else T) if eligible else 0), (name, rows, _n() - n0)
        return out, _greedy_vs_oracle(name, path + tag, cap, out, rows)
    try:
        # relu(Emb) W_x^T [V, 4H] (cut from Wih[:, H + E:]) serves the fed token once a call has rows * T >= V / 4 token
        # steps, and stays cached; before that a step contracts relu(Emb[token]) [rows, W] itself: both, in that order
        cap.__dict__.pop('_tab_cache', None)
        no_table_yet = rows * T < Wd.V // 4
        first, base = eager_first_call('')
        with torch.no_grad(), ops.h3_weights_scope(DEV):
            assert (cap._embedding_table(cap._p(), build=False) is None) == no_table_yet
            if no_table_yet:
                assert cap._embedding_table(cap._p(), build=True) is not None
        if no_table_yet:
            first, tabled = eager_first_call(' token table')
            assert torch.equal(tabled[0], base[0]) and torch.equal(tabled[2], base[2])
        if rows == 4:
            for _ in range(2):
                with torch.no_grad():
                    again = cap.forward_rl(*a, T, 1)
                for x, y in zip(again, first):
                    assert torch.equal(x, y)
            assert any(isinstance(e, tuple) for e in cap._rollout_graphs.values())     # it was captured
            _greedy_vs_oracle(name, path + ' graph', cap, again, rows)
        cap.enable_rollout_graphs(False)               # (a graph is keyed on shapes and weights, not on these switches)
        for switch in ('rows_step', 'gate_fused'):
            setattr(cap, switch, False)
            n0 = _n()
            with torch.no_grad():
                out = cap.forward_rl(*a, T, 1)
            torch.cuda.synchronize()
            if switch == 'gate_fused' or not eligible:
                assert _n() == n0
            else:
                assert _n() - n0 == T                  # general kernels, fused gate on the row scan kernel
            got = _greedy_vs_oracle(name, path + ' %s off' % switch, cap, out, rows)
            assert torch.equal(got[0], base[0]) and torch.equal(got[2], base[2])
            _close(name, path + ' %s off vs on' % switch, got[1], base[1], LOGP_TOL)
            setattr(cap, switch, True)
    finally:
        cap.rows_step = cap.gate_fused = True
        cap.enable_rollout_graphs(True)


# ----------------------------------------------------------------------------- e. sampled roll-out with gradients
@pytest.mark.parametrize('name', Wd.SMALL)
def test_e_sampled_rollout_gradients(name):
    from oracle import captioner_oracle as O
    st, w, d, _ = Wd.setup(name)
    cap = Captioner(Wd.idx2word(), synth.SENTIMENT_CATEGORIES, dict(st, dropout_p=0.0))
    cap.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    cap.to(DEV).train()
    g = torch.Generator().manual_seed(31)
    draws = torch.randint(4, Wd.V, (Wd.B, T), generator=g)
    for b in range(1, Wd.B, 2):                        # some rows end early, row 0 never
        draws[b, 2 + b % 6] = cap.eos_id
    reward = torch.randn(Wd.B, T, generator=g)
    cap.zero_grad()
    seq, lp, mk = cap.forward_rl(*_rl_args(d, Wd.B), T, 0, _replay=draws.to(DEV))
    assert lp.requires_grad
    loss = RewardCriterion()(lp, mk, reward.to(DEV))
    loss.backward()
    hg = {k: q.grad.detach().cpu().numpy().copy() for k, q in cap.named_parameters() if q.grad is not None}
    f64 = torch.float64
    p = O.to_params(w, dtype=f64, requires_grad=True)
    oseq, olp, omk, _, _, _ = O.forward_rl(p, Wd.oracle_ids(), *[Wd.cpu(d, k, dtype=f64) for k in Wd.RL_KEYS], T,
                                           sample_max=0, replay=draws)
    assert olp.shape[1] == T and 0 < float(omk.sum()) < Wd.B * T
    oloss = O.reward_criterion(olp, omk, reward.double())
    oloss.backward()
    og = {k: q.grad.numpy() for k, q in p.items() if q.grad is not None}
    assert torch.equal(seq.cpu(), oseq) and torch.equal(mk.cpu().double(), omk)
    _close(name, 'e sampled roll-out logp', lp.detach().cpu(), olp.detach(), LOGP_TOL)
    assert len(og) >= 36 and set(og) <= set(hg), sorted(set(og) - set(hg))
    for k in set(hg) - set(og):                        # (a tensor the oracle's graph does not reach has no gradient)
        assert np.abs(hg[k]).max() == 0.0, k
    worst = _compare(((float(loss.detach()),), {k: hg[k] for k in og}, {}), ((float(oloss.detach()),), og, {}),
                     n_expected=len(og), widen=False)
    _note_grads(name, 'e sampled roll-out grads', worst)


# ----------------------------------------------------------------------------- f. beam search
@pytest.mark.parametrize('name', Wd.SMALL + ('h_768',))
def test_f_beam_search(name):
    st, w, d, _ = Wd.setup(name)
    cap = _cap(name)
    eligible = Wd.WIDTHS[name]['rows_step']
    fc, att, sw, lab = (_dev(d, k) for k in ('fc_feats', 'att_feats', 'senti_words', 'senti_labels'))
    ref = []
    for i in range(3):                                 # the CPU facts the exact comparison rests on
        caps64, s64, i64 = Wd.oracle_beams(name, i)
        assert Wd.oracle_beams(name, i, dtype=torch.float32)[2] == i64
        assert (np.abs(np.diff(np.asarray(s64))) > Wd.MARGIN).all()
        ref.append((caps64, s64, i64))
    cap.enable_beam_graphs(True)                       # an empty cache: eager, capture, replay
    n0 = _n()
    per_image = []
    for i in (0, 1):
        calls = [cap.sample(fc[i], att[i], sw[i], lab[i:i + 1], 3, 1, T) for _ in range(3)]
        if i == 0:
            assert (_n() > n0) == eligible             # few-row step (counted on the eager call) / general kernels
        for caps, scores in calls:
            assert caps == ref[i][0], (name, i)
            assert caps == calls[0][0] and scores == calls[0][1]        # graph replays: the same bits
        _close(name, 'f beam scores', calls[0][1], ref[i][1], BEAM_SCORE_TOL)
        per_image.append(calls[0])
    assert any(isinstance(e, tuple) for e in cap._beam_graphs.values())
    batch = [cap.sample_batch(fc[:3], att[:3], sw[:3], lab[:3], 3, 1, T) for _ in range(3)]
    for caps, scores, ids in batch:
        assert caps == batch[0][0] and scores == batch[0][1] and ids == batch[0][2]
    caps, scores, ids = batch[0]
    for i in range(3):
        assert [list(x) for x in ids[i]] == ref[i][2], (name, i)
        assert caps[i] == ref[i][0]
        _close(name, 'f beam scores', scores[i], ref[i][1], BEAM_SCORE_TOL)
    for i in (0, 1):                                   # images are independent
        assert caps[i] == per_image[i][0]
        _close(name, 'f beam batch vs image', scores[i], per_image[i][1], 1e-4)


# ----------------------------------------------------------------------------- g. grouped sampled roll-out
@pytest.mark.parametrize('name', ['all_differ', 'h_wide'])
def test_g_grouped_rollout_is_the_repeated_rollout(name):
    from oracle import captioner_oracle as O
    st, w, d, _ = Wd.setup(name)
    cap = _cap(name)
    I, n = 3, 3
    a = _rl_args(d, I)
    tok = torch.randint(4, Wd.V, (I * n, T), generator=torch.Generator().manual_seed(5))
    tok[1, 3] = tok[5, 6] = cap.eos_id
    g, r = _both_forms(cap, a, n, T, _replay=tok.to(DEV))
    _assert_replay_forms_agree(g, r, I * n, T)
    f64 = torch.float64
    with torch.no_grad():
        oseq, olp, omk, _, ow, _ = O.forward_rl(
            O.to_params(w, dtype=f64), Wd.oracle_ids(),
            *[Wd.cpu(d, k, I, f64).repeat_interleave(n, 0) for k in Wd.RL_KEYS], T, sample_max=0, replay=tok)
    assert torch.equal(g[0].cpu(), oseq) and torch.equal(g[2].cpu().double(), omk)
    _close(name, 'g grouped roll-out logp', g[1].cpu(), olp, LOGP_TOL)
    for x, ref in zip(g[3:], ow):
        _close(name, 'g grouped roll-out weights', x.cpu(), ref, W_TOL)


# ----------------------------------------------------------------------------- h. the measured ratios
def test_zz_report_the_measured_ratios():
    """Prints, per width set and path, the worst error this file measured as a fraction of its bound (pytest -s)."""
    print()
    for (name, path), ratio in sorted(RATIOS.items()):
        print('WORST %-14s %-44s %.3f' % (name, path, ratio))
    assert all(v <= 1.0 for v in RATIOS.values())
