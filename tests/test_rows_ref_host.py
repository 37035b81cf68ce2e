"""The staged reference of the few-row decode step (tests/_rows_ref.py) on the host: composed end to end it is the
oracle's forward step (oracle/captioner_oracle.py) in fp64 on one tiny model - with the token table and with the xt
segment, with a source-row index, and with the rows grouped per image and per label group - and its tile helpers keep the
rule the kernels document (ties to the smaller id)."""
import numpy as np
import torch

import _fwd_ref as FR
import _rows_ref as RR
from insenticap_model_amd import synth
from oracle import captioner_oracle as O

F32, F64 = RR.F32, RR.F64
ST = dict(word_emb_dim=8, fc_feat_dim=12, att_feat_dim=20, feat_emb_dim=8, dropout_p=0.5, rnn_hid_dim=12, att_hid_dim=8)
V, R, MW = 23, 5, 3


def _model(B, seed=1):
    w = synth.make_weights(V, ST, seed=seed)
    d = synth.make_inputs(B, V, ST, regions=R, seq_len=4, seed=seed + 1)
    p = O.to_params(w, dtype=F64)
    ids = O.Ids(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES)
    t = lambda k: torch.from_numpy(np.asarray(d[k]))
    P = O.prologue(p, ids, 'rl', t('fc_feats').double(), t('att_feats').double(), t('cpt_words'), t('senti_words')[:, :MW - 1],
                   t('senti_labels'))
    return p, P


def _stage_inputs(p, P, h, c):
    """The step's tensors the way the library wants them, from the oracle's prologue (fp64)."""
    H, E = ST['rnn_hid_dim'], ST['feat_emb_dim']
    Wih1 = p['att_lstm.weight_ih']
    w = {'Wih1': Wih1, 'Whh1': p['att_lstm.weight_hh'], 'Wih2': p['lang_lstm.weight_ih'], 'Whh2': p['lang_lstm.weight_hh'],
         'b_ih2': p['lang_lstm.bias_ih'], 'b_hh2': p['lang_lstm.bias_hh'],
         'W_h2att': p['attention.cont_att.h2att.weight'], 'b_h2att': p['attention.cont_att.h2att.bias'],
         'W_h2word': p['attention.senti_att.h2word.weight'], 'b_h2word': p['attention.senti_att.h2word.bias'],
         'W_gh': p['attention.h2att.weight'], 'b_gh': p['attention.h2att.bias'],
         'w_alpha_c': p['attention.cont_att.att_alpha.weight'], 'b_alpha_c': p['attention.cont_att.att_alpha.bias'],
         'w_alpha_s': p['attention.senti_att.word_alpha.weight'], 'b_alpha_s': p['attention.senti_att.word_alpha.bias'],
         'b_gc': p['attention.cont2att.bias'], 'b_gs': p['attention.senti2att.bias'],
         'w_gate': p['attention.att_alpha.weight'], 'b_gate': p['attention.att_alpha.bias'],
         'W_cls': p['classifier.weight'], 'b_cls': p['classifier.bias']}
    pre1 = (P.fc_e @ Wih1[:, H:H + E].t() + P.label_e @ Wih1[:, H + E:].t() + p['att_lstm.bias_ih'] + p['att_lstm.bias_hh'])
    st = {'h1_prev': h[0], 'h2_prev': h[1], 'c1_prev': c[0], 'c2_prev': c[1], 'pre1': pre1, 'att_p': P.p_att, 'att_e': P.att_e,
          'Gc': P.att_e @ p['attention.cont2att.weight'].t(), 'words_p': P.p_words, 'words_e': P.words_e,
          'Gs': P.words_e @ p['attention.senti2att.weight'].t()}
    q2 = P.label_e @ p['attention.senti_att.label2word.weight'].t() + p['attention.senti_att.label2word.bias']
    tab = torch.relu(p['word_embed.0.weight']) @ Wih1[:, H + E:].t()
    return w, st, q2, tab


def _state(B, seed=3):
    g = torch.Generator().manual_seed(seed)
    H = ST['rnn_hid_dim']
    return (torch.rand(2, B, H, generator=g, dtype=F64) - 0.5, torch.rand(2, B, H, generator=g, dtype=F64) - 0.5,
            torch.randint(4, V, (B,), generator=g))


def _same(a, b, what):
    assert a.shape == b.shape, what
    np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=0, atol=1e-13, err_msg=what)


def _check(o, logp, state, wts, what):
    _same(o['h1'], state[0][0], what + ' h1')
    _same(o['c1'], state[1][0], what + ' c1')
    _same(o['h2'], state[0][1], what + ' h2')
    _same(o['c2'], state[1][1], what + ' c2')
    _same(o['alpha_c'], wts['cont'], what + ' alpha_c')
    _same(o['alpha_s'], wts['senti'], what + ' alpha_s')
    _same(o['beta'], wts['gate'], what + ' beta')
    _same(torch.log_softmax(o['logits'], 1), logp, what + ' logp')


def _oracle_step(p, P, tok, h, c, rows=None):
    sel = (lambda x: x) if rows is None else (lambda x: x[rows])
    with torch.no_grad():
        return O.step(p, tok, (h, c), sel(P.fc_e), sel(P.att_e), sel(P.p_att), sel(P.words_e), sel(P.p_words), sel(P.label_e))


def test_the_staged_reference_composed_is_the_oracles_step():
    B = 4
    p, P = _model(B)
    h, c, tok = _state(B)
    w, st, q2, tab = _stage_inputs(p, P, h, c)
    logp, state, wts = _oracle_step(p, P, tok, h, c)
    _check(RR.step_ref(F64, w, st, tab=tab, tok=tok, q2=q2), logp, state, wts, 'table')
    xt = torch.relu(p['word_embed.0.weight'][tok])
    _check(RR.step_ref(F64, w, st, xt=xt, q2=q2), logp, state, wts, 'xt')
    # float32 evaluation: same keys and shapes, close
    o32 = RR.step_ref(F32, w, st, tab=tab, tok=tok, q2=q2)
    o64 = RR.step_ref(F64, w, st, tab=tab, tok=tok, q2=q2)
    for k in o64:
        assert o32[k].dtype == F32 and o64[k].dtype == F64 and o32[k].shape == o64[k].shape
        assert float((o32[k].double() - o64[k]).abs().max()) < 1e-4, k


def test_source_rows_index_the_recurrent_state_only():
    B = 4
    p, P = _model(B)
    h, c, tok = _state(B)
    w, st, q2, tab = _stage_inputs(p, P, h, c)
    src = torch.tensor([2, 2, 0, 3])
    logp, state, wts = _oracle_step(p, P, tok, h[:, src], c[:, src])
    _check(RR.step_ref(F64, w, st, src=src, tab=tab, tok=tok, q2=q2), logp, state, wts, 'src')


def test_rows_grouped_per_image_and_per_label_group():
    """6 rows = 1 image x 2 label groups x 3 rows: image tensors one entry, sentiment tensors one entry per group, the
    sentiment features gathered from a table by the group's word ids."""
    p, P = _model(2)
    rows, row_div, senti_div = 6, 6, 3
    h, c, tok = _state(rows)
    img = torch.zeros(rows, dtype=torch.int64)              # every row reads image 0 ...
    grp = torch.arange(rows) // senti_div                   # ... and the sentiment side of entry 0 / 1
    w, st, q2, tab = _stage_inputs(p, P, h, c)
    H, E = ST['rnn_hid_dim'], ST['feat_emb_dim']
    Wih1 = p['att_lstm.weight_ih']
    pre1 = (P.fc_e[:1].expand(2, -1) @ Wih1[:, H:H + E].t() + P.label_e @ Wih1[:, H + E:].t() + p['att_lstm.bias_ih']
            + p['att_lstm.bias_hh'])
    # table form of the sentiment side: rows of both groups stacked, the ids point into the stack
    ids = torch.arange(2 * MW).view(2, MW).flip(0)          # group 0 reads the second entry's words
    flat = lambda x: x.reshape(2 * MW, -1)
    st2 = dict(st, pre1=pre1, att_p=P.p_att[:1], att_e=P.att_e[:1], Gc=st['Gc'][:1], words_p=flat(P.p_words),
               words_e=flat(P.words_e), Gs=flat(st['Gs']))
    o = RR.step_ref(F64, w, st2, tab=tab, tok=tok, q2=q2, ids=ids, row_div=row_div, senti_div=senti_div)
    words = 1 - grp                                          # the entry whose words a row reads
    with torch.no_grad():
        logp, state, wts = O.step(p, tok, (h, c), P.fc_e[img], P.att_e[img], P.p_att[img], P.words_e[words], P.p_words[words],
                                  P.label_e[grp])
    _check(o, logp, state, wts, 'groups')


def test_candidates_take_the_smaller_id_on_ties_and_tile_statistics_at_any_width():
    x = torch.tensor([[1.0, 3.0, 3.0, -2.0, 3.0, 0.5, 3.0, 3.0, 1.5, 3.0]])
    banned = torch.zeros_like(x, dtype=torch.bool)
    banned[0, 1] = True
    vals, ids = RR.masked_candidates(x, 4, 3, banned)
    assert ids.tolist() == [[[2, 0, 3], [4, 6, 7], [9, 8, 0]]]
    assert vals[0, 0].tolist() == [3.0, 1.0, -2.0] and vals[0, 2, 2] == -np.inf
    pm, ps, pi = FR.tile_stats(x, 4)
    assert pi.tolist() == [[1, 4, 9]] and pm.tolist() == [[3.0, 3.0, 3.0]]
    np.testing.assert_allclose(ps.numpy(), [[2 + np.exp(-2.0) + np.exp(-5.0), 3 + np.exp(-2.5), 1 + np.exp(-1.5)]], rtol=1e-6)
    pm128, _, pi128 = FR.tile_stats(x)
    assert pi128.tolist() == [[1]] and pm128.shape == (1, 1)
