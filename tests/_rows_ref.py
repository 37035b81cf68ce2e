"""fp64 references of the few-row decode step (csrc/rows.hip, isc_rows_step_fwd), stage by stage, for
tests/test_gpu_rows_kernels.py (checked on the host against oracle/captioner_oracle.py by tests/test_rows_ref_host.py).

One function per launch of the step, each of that launch's OWN inputs, written once over a dtype as in tests/_bwd_ref.py:
float64 = the reference, float32 = err32, the float32 tanh in common.h's form.  The bound and the comparison are
_bwd_ref.check_output's: atol = 8 * max(err32, 2^-23 * max|ref|).

Layouts are the library's: LSTM gates (i, f, g, o) in blocks of H; Wih1 [4H, H + E + W] over cat[h_lang, fc, xt] with the
fc / label / bias terms hoisted into pre1; Wih2 [4H, E + H] over cat[f, h_att]; the recurrent state behind an optional
source-row index (a beam's re-ordering); the sentiment half of the scan per label group (senti_div rows), the content half
per image (row_div rows)."""
import numpy as np
import torch

from _bwd_ref import F32, F64, _c, both, tanh_           # noqa: F401  (re-exported to the tests)


def _ids(x):
    return None if x is None else x.detach().cpu().to(torch.int64)


def _src(x, src):
    return x if src is None else x[_ids(src)]


def _cell(dt, gates, c_prev, H):
    """isc_lstm_cell: c' = sig(f) c + sig(i) tanh(g), h' = sig(o) tanh(c')."""
    i, f, g, o = gates[:, :H], gates[:, H:2 * H], gates[:, 2 * H:3 * H], gates[:, 3 * H:]
    c = torch.sigmoid(f) * c_prev + torch.sigmoid(i) * tanh_(g)
    return torch.sigmoid(o) * tanh_(c), c


def att_lstm_ref(dt, h2_prev, h1_prev, c1_prev, Wih1, Whh1, pre1, E, src=None, xt=None, tab=None, tok=None, senti_div=1):
    """gates = h2_prev[src] Wih1[:, :H]^T + (xt Wih1[:, H+E:]^T | tab[tok]) + h1_prev[src] Whh1^T + pre1[m // senti_div]"""
    H = h1_prev.shape[1]
    M = (xt if tok is None else tok).shape[0]
    Wi, Wh = _c(Wih1, dt), _c(Whh1, dt)
    g = _src(_c(h2_prev, dt), src) @ Wi[:, :H].t() + _src(_c(h1_prev, dt), src) @ Wh.t()
    g = g + (_c(tab, dt)[_ids(tok)] if tok is not None else _c(xt, dt) @ Wi[:, H + E:].t())
    if pre1 is not None:
        g = g + _c(pre1, dt)[torch.arange(M) // max(int(senti_div), 1)]
    h1, c1 = _cell(dt, g, _src(_c(c1_prev, dt), src), H)
    return {'h1': h1, 'c1': c1}


def proj_ref(dt, h1, W_h2att, b_h2att, W_h2word, b_h2word, W_gh, b_gh):
    """qa = h2att(h1), qw = h2word(h1), z = the gate's h-term"""
    h = _c(h1, dt)
    return {'qa': h @ _c(W_h2att, dt).t() + _c(b_h2att, dt), 'qw': h @ _c(W_h2word, dt).t() + _c(b_h2word, dt),
            'z': h @ _c(W_gh, dt).t() + _c(b_gh, dt)}


def gated_scan_ref(dt, att_p, att_e, Gc, words_p, words_e, Gs, qa, qw, zh, wc, bc, ws, bs, b_gc, b_gs, wg, bg, q2=None,
                   ids=None, row_div=1, senti_div=1):
    """e_c = wc . tanh(att_p + qa) + bc, e_s = ws . tanh(words_p + qw + q2) + bs; alpha = softmax(e);
    v = alpha_c att_e, s = alpha_s words_e; z = zh + (alpha_c Gc + b_gc) + (alpha_s Gs + b_gs) with the PRE-PROJECTED rows
    Gc = cont2att(att_e), Gs = senti2att(words_e) (no bias); beta = sigmoid(wg . tanh(z) + bg); f = beta v + (1 - beta) s.
    att_* / Gc: [images, R, A], row m reads image m // row_div.  Sentiment half: per group [groups, Mw, A] (row m reads group
    m // senti_div, q2 = label_w [groups, A] as well), or - ids [groups, Mw] - tables [n, A] gathered by the group's ids."""
    rows = qa.shape[0]
    im = torch.arange(rows) // max(int(row_div), 1)
    gr = torch.arange(rows) // max(int(senti_div), 1)
    Pc, Vc, Gcc = _c(att_p, dt)[im], _c(att_e, dt)[im], _c(Gc, dt).reshape(att_e.shape)[im]
    if ids is not None:
        idx = _ids(ids)[gr]
        Ps, Vs, Gss = _c(words_p, dt)[idx], _c(words_e, dt)[idx], _c(Gs, dt)[idx]
    else:
        Ps, Vs, Gss = _c(words_p, dt)[gr], _c(words_e, dt)[gr], _c(Gs, dt).reshape(words_e.shape)[gr]
    qq = _c(qw, dt) if q2 is None else _c(qw, dt) + _c(q2, dt)[gr]

    def one(x):
        return 0.0 if x is None else _c(x, dt).reshape(())
    ec = (tanh_(Pc + _c(qa, dt).unsqueeze(1)) * _c(wc, dt).reshape(-1)).sum(-1) + one(bc)
    es = (tanh_(Ps + qq.unsqueeze(1)) * _c(ws, dt).reshape(-1)).sum(-1) + one(bs)
    ac, as_ = torch.softmax(ec, -1), torch.softmax(es, -1)
    v, s = (ac.unsqueeze(-1) * Vc).sum(1), (as_.unsqueeze(-1) * Vs).sum(1)
    z = (_c(zh, dt) + ((ac.unsqueeze(-1) * Gcc).sum(1) + _c(b_gc, dt))) + ((as_.unsqueeze(-1) * Gss).sum(1) + _c(b_gs, dt))
    beta = torch.sigmoid((tanh_(z) * _c(wg, dt).reshape(-1)).sum(-1, keepdim=True) + one(bg))
    return {'alpha_c': ac, 'alpha_s': as_, 'beta': beta, 'f': beta * v + (1 - beta) * s}


def lang_lstm_ref(dt, f, h1, h2_prev, c2_prev, Wih2, Whh2, b_ih2, b_hh2, src=None):
    """gates = cat[f, h1] Wih2^T + h2_prev[src] Whh2^T + (b_ih2 + b_hh2)"""
    H = h1.shape[1]
    g = torch.cat([_c(f, dt), _c(h1, dt)], 1) @ _c(Wih2, dt).t() + _src(_c(h2_prev, dt), src) @ _c(Whh2, dt).t()
    g = g + (_c(b_ih2, dt) + _c(b_hh2, dt))
    h2, c2 = _cell(dt, g, _src(_c(c2_prev, dt), src), H)
    return {'h2': h2, 'c2': c2}


def classifier_ref(dt, h2, W_cls, b_cls):
    return {'logits': _c(h2, dt) @ _c(W_cls, dt).t() + _c(b_cls, dt)}


def lse_ref(dt, logits, pmax, psum):
    """The row's log-sum-exp folded from tile statistics, and straight from the logits it must equal."""
    pm, ps = _c(pmax, dt), _c(psum, dt)
    gmax = pm.max(1).values
    return {'lse': gmax + torch.log((ps * torch.exp(pm - gmax[:, None])).sum(1))}


def lse_of_logits(dt, logits):
    return {'lse': torch.logsumexp(_c(logits, dt), 1)}


def tiles(x, tw, fill=-np.inf):
    """float32 rows [M, V] -> [M, n_tile, tw], padded with `fill`"""
    x = x.detach().cpu()
    M, V = x.shape
    nt = (V + tw - 1) // tw
    pad = torch.full((M, nt * tw), fill, dtype=x.dtype)
    pad[:, :V] = x
    return pad.view(M, nt, tw)


def masked_candidates(x, tw, k, banned):
    """The per-tile candidates of the stored float32 logits x [M, V]: the k largest of every tile after `banned` [M, V]
    (bool) went to -inf, descending, ties to the SMALLER id (a stable sort of the negated values); slots a tile cannot
    fill (the last tile's columns past V) hold (-inf, id 0), as the kernel leaves them.  (values [M, nt, k],
    ids [M, nt, k] int64)"""
    x = x.detach().cpu().clone()
    x[banned] = -np.inf
    t = tiles(x, tw)
    M, nt, _ = t.shape
    order = torch.sort(-t.double(), dim=2, stable=True).indices[:, :, :k]
    vals = t.gather(2, order)
    ids = order + (torch.arange(nt) * tw)[None, :, None]
    ids[ids >= x.shape[1]] = 0                              # a slot past the last column: (-inf, id 0)
    return vals, ids


def step_ref(dt, w, st, src=None, tab=None, tok=None, xt=None, q2=None, ids=None, row_div=1, senti_div=1):
    """The five stages composed (each on the previous one's output): w = the weights, st = the step's tensors."""
    E = w['Wih2'].shape[1] - w['Whh2'].shape[1]
    o = att_lstm_ref(dt, st['h2_prev'], st['h1_prev'], st['c1_prev'], w['Wih1'], w['Whh1'], st['pre1'], E, src, xt, tab, tok,
                     senti_div)
    o.update(proj_ref(dt, o['h1'], w['W_h2att'], w['b_h2att'], w['W_h2word'], w['b_h2word'], w['W_gh'], w['b_gh']))
    o.update(gated_scan_ref(dt, st['att_p'], st['att_e'], st['Gc'], st['words_p'], st['words_e'], st['Gs'], o['qa'], o['qw'],
                            o['z'], w['w_alpha_c'], w['b_alpha_c'], w['w_alpha_s'], w['b_alpha_s'], w['b_gc'], w['b_gs'],
                            w['w_gate'], w['b_gate'], q2, ids, row_div, senti_div))
    o.update(lang_lstm_ref(dt, o['f'], o['h1'], st['h2_prev'], st['c2_prev'], w['Wih2'], w['Whh2'], w['b_ih2'], w['b_hh2'],
                           src))
    o.update(classifier_ref(dt, o['h2'], w['W_cls'], w['b_cls']))
    return o
