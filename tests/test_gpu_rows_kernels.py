"""The few-row decode kernels (csrc/rows.hip) one by one against fp64: rows_lstm_kernel, rows_linear_kernel,
rows_scan_gate_kernel and rows_vocab_kernel, each held to the reference of ITS stage (tests/_rows_ref.py) evaluated on
the device's own upstream outputs, so that a kernel answers for its own error only.

The plans are built by hand from plain tensors (no Captioner, no synth): widths and counts are free.  Every output buffer
is pre-filled with _bwd_ref.SENTINEL, has one row more than the step owns and - alpha_c, alpha_s, beta, logits - a leading
dimension wider than its row; everything outside what the step owns must keep the sentinel.  Floating outputs are held by
_bwd_ref.check_output's rule, atol = 8 * max(err32, 2^-23 max|ref|), and nothing else; tile maxima, arg-maxima and the
beam candidates are exact functions of the STORED logits.  The route of every launch (isc_rows_routes) is asserted against
the geometry restated here, and the last test holds the union of the routes seen to the instantiation table of DESIGN.md.

The ratio err_kernel / max(err32, 2^-23 max|ref|) of every output is printed by `pytest -m gpu -s` (the WORST lines of
test_zz_report...); the docstrings give what an MI355X measured (the largest of all: 4.45, the content alpha of the lone
scan at R = 72; no output needed a bound of its own, and no kernel was found wrong: the defect this file's work closed
is the gate's, tests/test_rows_gate_host.py).  pytest -m gpu."""
import ctypes as C
import functools
import os
import re

import pytest
import torch

import _fwd_ref as FR
import _rows_ref as RR
import _split_f16 as S16
from _bwd_ref import SENTINEL as SENT, WORST, check_output
from insenticap_model_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ISENT = -77
KC = 8                       # ROWS_KC: candidate slots per (row, tile)
SEEN = {}                    # instantiation -> the tests that launched it
DONE = set()                 # the launching tests (with their parameters) that ran to their end in this process


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def sent(*shape, dtype=torch.float32):
    return torch.full(shape, SENT if dtype.is_floating_point else ISENT, device=DEV, dtype=dtype)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ routes
def _mr(M):
    return 2 if M <= 2 else 4 if M <= 4 else 6 if M <= 6 else 8


def lstm_route(Ks, M, H, nt):
    """rows_lstm's geometry: slices of 256 per segment, S <= 8 in flight, U = J * UPW units per workgroup."""
    MR, nsl = _mr(M), sum(cdiv(k, 256) for k in Ks)
    S, want = min(nsl, 8), max(cdiv(H, 256), 1)
    J, upw = max(8 // S, 1), 1
    if J > want:
        J = want
    if J < want:
        upw = 2
    while J > 1 and J * upw * MR > 64:
        J -= 1
    if J * upw * MR > 64:
        upw = 1
    return ('lstm', MR, upw, int(nt), 0, S, J, nsl)


def linear_route(K, M, Ntot):
    nsl = cdiv(K, 128 if K >= 256 else 256)
    S = min(nsl, 8)
    J = max(8 // S, 1)
    while J > 1 and cdiv(Ntot // 4, J) < 192:
        J -= 1
    return ('linear', _mr(M), 1, 0, 0, S, J, nsl)


def vocab_route(M, V, K, nt, ban):
    tw = ops.rows_stats_tile(V)
    nsl, passes = cdiv(K, 256), cdiv(tw, 4)
    S = min(nsl, 8)
    J = min(max(8 // S, 1), 4, passes)
    np_ = cdiv(passes, J)
    assert np_ <= 4 and 16 * np_ >= tw
    return ('vocab', _mr(M), np_, int(nt), int(ban), S, J, nsl)


def scan_route(R, Mw):
    return ('scan', 0, int(R <= 36 and Mw <= 12), 0, 0, 0, 0, 0)


def instantiation(r):
    b = lambda x: 'true' if x else 'false'
    if r[0] == 'lstm':
        return 'rows_lstm_kernel<%d, %d, %s>' % (r[1], r[2], b(r[3]))
    if r[0] == 'linear':
        return 'rows_linear_kernel<%d>' % r[1]
    if r[0] == 'scan':
        return 'rows_scan_gate_kernel'
    return 'rows_vocab_kernel<%d, %d, %s, %s>' % (r[1], r[2], b(r[3]), b(r[4]))


class routes:
    """with routes(test, [expected...]): the launches inside are exactly these, in this order."""

    def __init__(self, test, want):
        self.test, self.want = test, list(want)

    def __enter__(self):
        self.n0 = ops.rows_routes(0)[0]
        self.l0 = ops._lib.load().isc_rows_launches()
        return self

    def __exit__(self, et, ev, tb):
        if et is not None:
            return False
        total, recs = ops.rows_routes(len(self.want))
        assert total - self.n0 == len(self.want) == ops._lib.load().isc_rows_launches() - self.l0, (total - self.n0, self.want)
        assert recs == self.want, (recs, self.want)
        for r in recs:
            SEEN.setdefault(instantiation(r), set()).add(self.test)
        return False


class nt_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = ops.set_rows_nt(self.mode)

    def __exit__(self, *exc):
        ops.set_rows_nt(self.prev)
        return False


# ------------------------------------------------------------------------------------------------ the step
# name -> H, A (= E = W), R, Mw, V, row_div, senti_div, gather (words by ids from a table), rows
STEP = {
    'tiny': dict(H=4, A=4, R=1, Mw=1, V=37, rows=(1,)),
    'ragged': dict(H=260, A=132, R=37, Mw=12, V=300, rows=(3,)),
    'upw2': dict(H=516, A=260, R=73, Mw=13, V=300, rows=(4, 5)),
    'h768': dict(H=768, A=32, R=7, Mw=5, V=300, rows=(1, 7)),
    'slices12': dict(H=1280, A=260, R=12, Mw=4, V=300, rows=(8,)),
    'groups': dict(H=64, A=32, R=13, Mw=3, V=130, rows=(6,), row_div=6, senti_div=3, gather=True),
    'wide8': dict(H=64, A=32, R=13, Mw=3, V=130, rows=(8,)),
}
STEP_RUNS = [(k, r) for k, c in STEP.items() for r in c['rows']]


@functools.lru_cache(maxsize=2)
def _weights(name):
    c = STEP[name]
    H, A, V = c['H'], c['A'], c['V']
    g = gen(sum(map(ord, name)))
    w = dict(Wih1=rn(g, 4 * H, H + 2 * A, scale=1.5 * (H + 2 * A) ** -0.5), Whh1=rn(g, 4 * H, H, scale=1.5 * H ** -0.5),
             Wih2=rn(g, 4 * H, A + H, scale=1.5 * (A + H) ** -0.5), Whh2=rn(g, 4 * H, H, scale=1.5 * H ** -0.5),
             b_ih2=rn(g, 4 * H, scale=0.3), b_hh2=rn(g, 4 * H, scale=0.3),
             W_h2att=rn(g, A, H, scale=H ** -0.5), b_h2att=rn(g, A, scale=0.3),
             W_h2word=rn(g, A, H, scale=H ** -0.5), b_h2word=rn(g, A, scale=0.3),
             W_gh=rn(g, A, H, scale=H ** -0.5), b_gh=rn(g, A, scale=0.3),
             w_alpha_c=rn(g, A, scale=0.5), b_alpha_c=rn(g, 1), w_alpha_s=rn(g, A, scale=0.5), b_alpha_s=rn(g, 1),
             b_gc=rn(g, A, scale=0.3), b_gs=rn(g, A, scale=0.3), w_gate=rn(g, A, scale=0.5), b_gate=rn(g, 1),
             W_cls=rn(g, V, H, scale=2.0 * H ** -0.5), b_cls=rn(g, V), tab=rn(g, V, 4 * H, scale=0.5))
    return w, {k: v.to(DEV) for k, v in w.items()}


def _step_tensors(name, rows, seed):
    c = STEP[name]
    H, A, R, Mw, V = c['H'], c['A'], c['R'], c['Mw'], c['V']
    row_div, senti_div = c.get('row_div', 1), c.get('senti_div', 1)
    n_img, n_grp = rows // row_div, rows // senti_div
    g = gen(seed)
    st = dict(h1_prev=rn(g, rows, H, scale=0.5), c1_prev=rn(g, rows, H, scale=0.7), h2_prev=rn(g, rows, H, scale=0.5),
              c2_prev=rn(g, rows, H, scale=0.7), pre1=rn(g, n_grp, 4 * H, scale=0.5),
              att_p=torch.relu(rn(g, n_img, R, A)), att_e=torch.relu(rn(g, n_img, R, A)), Gc=rn(g, n_img, R, A, scale=0.5),
              label_w=rn(g, n_grp, A, scale=0.5), xt=torch.relu(rn(g, rows, A)),
              tok=torch.randint(4, V, (rows, 3), generator=g), last=torch.randint(4, V, (rows,), generator=g),
              src=torch.randint(0, rows, (rows,), generator=g))
    if rows > 2:
        st['src'][1] = st['src'][0]                              # a row repeated (and with it, one dropped)
    if c.get('gather'):
        n = 20
        st.update(words_p=torch.relu(rn(g, n, A)), words_e=torch.relu(rn(g, n, A)), Gs=rn(g, n, A, scale=0.5),
                  ids=torch.randint(0, n, (n_grp, Mw + 2), generator=g))
    else:
        st.update(words_p=torch.relu(rn(g, n_grp, Mw, A)), words_e=torch.relu(rn(g, n_grp, Mw, A)),
                  Gs=rn(g, n_grp, Mw, A, scale=0.5), ids=None)
    return st


def _run_step(name, rows, st, wd, use_tab, use_src, live=None):
    """One isc_rows_step_fwd: returns the output buffers (each one row longer than the step owns, all sentinels before)."""
    c = STEP[name]
    H, A, R, Mw, V = c['H'], c['A'], c['R'], c['Mw'], c['V']
    tw = ops.rows_stats_tile(V)
    nt = cdiv(V, tw)
    sd = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in st.items()}
    o = dict(h1=sent(rows + 1, H), c1=sent(rows + 1, H), h2=sent(rows + 1, H), c2=sent(rows + 1, H),
             qa=sent(rows + 1, A), qw=sent(rows + 1, A), z=sent(rows + 1, A), f=sent(rows + 1, A),
             alpha_c=sent(rows + 1, R + 3), alpha_s=sent(rows + 1, Mw + 2), beta=sent(rows + 1, 3),
             logits=sent(rows + 1, V + 5), pmax=sent(rows + 1, nt), psum=sent(rows + 1, nt),
             pidx=sent(rows + 1, nt, dtype=torch.int32), cand_val=sent(rows + 1, nt, KC),
             cand_idx=sent(rows + 1, nt, KC, dtype=torch.int32))
    p = _lib.StepPlan()
    p.rows, p.H, p.E, p.A, p.W, p.V, p.R, p.Mw = rows, H, A, A, A, V, R, Mw
    for k in ('Wih1', 'Whh1', 'Wih2', 'Whh2', 'b_ih2', 'b_hh2', 'W_h2att', 'b_h2att', 'W_h2word', 'b_h2word', 'W_gh', 'b_gh',
              'w_alpha_c', 'b_alpha_c', 'w_alpha_s', 'b_alpha_s', 'b_gc', 'b_gs', 'w_gate', 'b_gate', 'W_cls', 'b_cls'):
        setattr(p, k, wd[k].data_ptr())
    for k in ('pre1', 'att_p', 'att_e', 'words_p', 'words_e', 'label_w', 'h1_prev', 'c1_prev', 'h2_prev', 'c2_prev'):
        setattr(p, k, sd[k].data_ptr())
    p.gate_Gc, p.gate_Gs = sd['Gc'].data_ptr(), sd['Gs'].data_ptr()
    if sd['ids'] is not None:
        p.words_ids, p.words_ids_ld = sd['ids'].data_ptr(), sd['ids'].stride(0)
    if use_tab:
        p.tab, p.tok, p.tok_stride = wd['tab'].data_ptr(), sd['tok'].data_ptr(), sd['tok'].stride(0)
    else:
        p.xt = sd['xt'].data_ptr()
    for k in ('h1', 'c1', 'h2', 'c2', 'qa', 'qw', 'z', 'f', 'alpha_c', 'alpha_s', 'beta', 'logits', 'pmax', 'psum', 'pidx'):
        setattr(p, k, o[k].data_ptr())
    p.alpha_c_ld, p.alpha_s_ld, p.beta_ld, p.ld_logits = R + 3, Mw + 2, 3, V + 5
    x = _lib.RowsExt()
    x.stats_tile, x.beam = tw, 5
    x.pad_id, x.sos_id, x.unk_id, x.mask_special, x.decoding_constraint = 0, 1, 3, 1, 1
    x.last_word, x.cand_val, x.cand_idx = sd['last'].data_ptr(), o['cand_val'].data_ptr(), o['cand_idx'].data_ptr()
    x.row_div, x.senti_div = c.get('row_div', 1), c.get('senti_div', 0)
    if use_src:
        x.src_row = sd['src'].data_ptr()
    if live is not None:
        x.live_in = live.data_ptr()
    assert ops.rows_step_supported(p)
    ops.rows_step_fwd(p, x)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def _step_routes(name, rows, use_tab, mode=1):
    """The five launches of a step under cache-policy mode `mode` (2: the LSTMs non-temporal; >= 1: the classifier)."""
    c = STEP[name]
    H, A = c['H'], c['A']
    return [lstm_route([H, H] if use_tab else [H, A, H], rows, H, mode == 2), linear_route(H, rows, 3 * A),
            scan_route(c['R'], c['Mw']), lstm_route([A, H, H], rows, H, mode == 2),
            vocab_route(rows, c['V'], H, mode >= 1, False)]


def _check_classifier(tag, lg, pm, ps, pi, cv, ci, tw, banned, n):
    """Statistics and candidates as exact functions of the stored logits `lg` [n, V] (float32, host); psum by the rule."""
    t = RR.tiles(lg, tw)
    nt = t.shape[1]
    FR.check_exact(pm[:n], t.max(2).values, tag + ' pmax')
    col = torch.arange(tw).expand_as(t)
    first = torch.where(t == t.max(2, keepdim=True).values, col, torch.full_like(col, tw)).min(2).values
    FR.check_exact(pi[:n], first + torch.arange(nt)[None, :] * tw, tag + ' pidx: the smallest id of the tile maximum')
    ref, ev = RR.both(_psum_ref, lg, tw)
    check_output(ps, ref['psum'], ev['psum'], 'rows:vocab/psum' + tag)
    if cv is not None:
        vals, ids = RR.masked_candidates(lg, tw, KC, banned)
        FR.check_exact(cv[:n], vals, tag + ' candidate values')
        FR.check_exact(ci[:n], ids, tag + ' candidate ids')
        assert bool((cv[n:] == SENT).all()) and bool((ci[n:] == ISENT).all()), tag
    assert bool((pm[n:] == SENT).all()) and bool((pi[n:] == ISENT).all()), tag


def _psum_ref(dt, x, tw):
    t = RR.tiles(x, tw).to(dt)
    return {'psum': torch.exp(t - t.max(2, keepdim=True).values).sum(2)}


def _banned(lg, last=None, lists=None):
    n, V = lg.shape
    b = torch.zeros(n, V, dtype=torch.bool)
    b[:, [0, 1, 3]] = True
    if last is not None:
        b[torch.arange(n), last] = True
    if lists is not None:
        ids, cnt = lists
        for m in range(n):
            for e in ids[m, :int(cnt[m])].tolist():
                if 0 <= e < V:
                    b[m, e] = True
    return b


def _check_step(name, rows, st, w, o, use_tab, use_src, tag):
    c = STEP[name]
    A, V = c['A'], c['V']
    tw = ops.rows_stats_tile(V)
    src = st['src'] if use_src else None
    senti_div = c.get('senti_div', 1)
    n = rows
    K = lambda s: 'rows:%s%s' % (s, tag)
    ref, ev = RR.both(RR.att_lstm_ref, st['h2_prev'], st['h1_prev'], st['c1_prev'], w['Wih1'], w['Whh1'], st['pre1'], A, src,
                      None if use_tab else st['xt'], w['tab'] if use_tab else None, st['tok'][:, 0] if use_tab else None,
                      senti_div)
    for k in ('h1', 'c1'):
        check_output(o[k], ref[k], ev[k], K('lstm/att_' + k))
    h1 = o['h1'][:n]
    ref, ev = RR.both(RR.proj_ref, h1, w['W_h2att'], w['b_h2att'], w['W_h2word'], w['b_h2word'], w['W_gh'], w['b_gh'])
    for k in ('qa', 'qw', 'z'):
        check_output(o[k], ref[k], ev[k], K('linear/' + k))
    ids = None if st['ids'] is None else st['ids'][:, :c['Mw']]
    ref, ev = RR.both(RR.gated_scan_ref, st['att_p'], st['att_e'], st['Gc'], st['words_p'], st['words_e'], st['Gs'], o['qa'][:n],
                      o['qw'][:n], o['z'][:n], w['w_alpha_c'], w['b_alpha_c'], w['w_alpha_s'], w['b_alpha_s'], w['b_gc'],
                      w['b_gs'], w['w_gate'], w['b_gate'], st['label_w'], ids, c.get('row_div', 1), senti_div)
    for k in ('alpha_c', 'alpha_s', 'beta'):
        check_output(o[k], ref[k], ev[k], K('scan/' + k), pad='sentinel')
    check_output(o['f'], ref['f'], ev['f'], K('scan/f'))
    ref, ev = RR.both(RR.lang_lstm_ref, o['f'][:n], h1, st['h2_prev'], st['c2_prev'], w['Wih2'], w['Whh2'], w['b_ih2'],
                      w['b_hh2'], src)
    for k in ('h2', 'c2'):
        check_output(o[k], ref[k], ev[k], K('lstm/lang_' + k))
    ref, ev = RR.both(RR.classifier_ref, o['h2'][:n], w['W_cls'], w['b_cls'])
    check_output(o['logits'], ref['logits'], ev['logits'], K('vocab/logits'), pad='sentinel')
    lg = o['logits'][:n, :V].contiguous()
    _check_classifier(tag, lg, o['pmax'], o['psum'], o['pidx'], o['cand_val'], o['cand_idx'], tw, _banned(lg, st['last']), n)


@pytest.mark.parametrize('name,rows', STEP_RUNS)
def test_step_stage_by_stage_vs_fp64(name, rows):
    """isc_rows_step_fwd, five launches, each output against its own stage's fp64 reference on the device's upstream
    outputs: with the token table and with the xt segment, each plain and behind a source-row index that repeats and drops
    rows (one set of weights per case).  The cases are the smallest shapes that reach: one float4 everywhere (tiny);
    ragged 256 + 4 slices, na4 = 33, region 36 alone in the scan's second trip with 12 words (ragged); UPW = 2 at MR 4 /
    6, a third slice of 4 floats, na4 = 65, the sentiment waves walking at Mw = 13, a second softmax chunk at R = 73
    (upw2); UPW = 2 at MR 2 / 8 with the seven-slice xt form (h768); 12 LSTM slices against the 8 in flight, 10
    projection slices (slices12); rows grouped per image and per label group with gathered words (groups); UPW = 1 at
    MR 8 (wide8).
    Measured (MI355X, worst ratio over the 36 runs): att-LSTM h1 1.48, c1 1.21; qa 0.76, qw 0.80, z 0.82; alpha_c 3.10,
    alpha_s 1.81, beta 2.82, f 1.99; lang-LSTM h2 1.22, c2 0.82; logits 0.64, psum 0.93."""
    test = 'test_step_stage_by_stage_vs_fp64'
    w, wd = _weights(name)
    st = _step_tensors(name, rows, 100 + rows)
    for use_tab in (True, False):
        for use_src in (False, True):
            tag = '[%s,M%d,%s%s]' % (name, rows, 'tab' if use_tab else 'xt', ',src' if use_src else '')
            with routes(test, _step_routes(name, rows, use_tab)):
                o = _run_step(name, rows, st, wd, use_tab, use_src)
            _check_step(name, rows, st, w, o, use_tab, use_src, tag)
    DONE.add('%s[%s-%d]' % (test, name, rows))


@pytest.mark.parametrize('name,rows', STEP_RUNS)
def test_step_cache_policies_and_live_flag_agree_in_bits(name, rows):
    """The three cache-policy modes (isc_set_rows_nt 0 / 1 / 2: the loads differ in policy only) give every output of
    the step in the same bits; so does isc_rows_ext.live_in -> 1; live_in -> 0 leaves every buffer at its sentinel."""
    test = 'test_step_cache_policies_and_live_flag_agree_in_bits'
    w, wd = _weights(name)
    st = _step_tensors(name, rows, 100 + rows)
    outs = {}
    for mode in (0, 1, 2):
        with nt_mode(mode):
            with routes(test, _step_routes(name, rows, True, mode)):
                outs[mode] = _run_step(name, rows, st, wd, True, True)
    for mode in (0, 2):
        for k in outs[1]:
            assert torch.equal(outs[mode][k], outs[1][k]), (mode, k)
    one, zero = torch.ones(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    with routes(test, _step_routes(name, rows, True)):
        o1 = _run_step(name, rows, st, wd, True, True, live=one)
    for k in o1:
        assert torch.equal(o1[k], outs[1][k]), k
    o0 = _run_step(name, rows, st, wd, True, True, live=zero)       # (the launches are issued and return at once)
    for k, v in o0.items():
        assert bool((v == (SENT if v.dtype.is_floating_point else ISENT)).all()), k
    DONE.add('%s[%s-%d]' % (test, name, rows))


# ------------------------------------------------------------------------------------------------ the scan alone
# B, R, Mw, A, gather, q2, w_bias, planes, row_div
SCAN = [(1, 12, 1, 4, False, False, False, False, 1),
        (3, 13, 4, 252, True, True, True, False, 1),
        (2, 36, 12, 256, False, True, True, True, 1),
        (3, 37, 12, 260, True, True, False, False, 1),
        (2, 64, 5, 512, False, False, True, True, 1),
        (4, 65, 1, 260, True, False, True, False, 2),
        (2, 72, 4, 252, False, True, False, False, 1),
        (3, 73, 12, 256, True, True, True, True, 1),
        (2, 109, 5, 4, False, True, True, False, 2),
        (5, 36, 5, 260, False, False, False, False, 1),
        (1, 37, 1, 512, True, True, True, False, 1),
        (2, 65, 12, 4, False, True, False, False, 1),
        # the row-kernel shapes of test_gated_scan_odd_shapes_vs_fp64 (tests/test_gpu_parity.py)
        (3, 1, 1, 64, False, True, True, False, 1),
        (5, 196, 3, 256, True, True, True, False, 1),
        (1, 36, 11, 512, True, True, True, False, 1)]


@pytest.mark.parametrize('B,R,Mw,A,gather,with_q2,with_bias,planes,row_div', SCAN)
def test_scan_gate_row_kernel_vs_fp64(B, R, Mw, A, gather, with_q2, with_bias, planes, row_div):
    """rows_scan_gate_kernel through isc_attn_scan_gate_fwd (exactly one rows launch): the last region of a trip and the
    first of the next (R = 36 / 37, 72 / 73, 109 = 36 * 3 + 1), the 64-lane softmax chunk edge (R = 64 / 65), 12 / 13
    regions (one / two regions in some waves), A / 4 = 1, 63, 64, 65 and 128 float4 lanes, 1 ... 12 words, per-row and
    gathered sentiment features, q2 and the two score biases on and off, rows grouped per image (row_div = 2), the f16
    planes of f against tests/_split_f16.py.
    Measured (MI355X, worst ratio over the 15 cases): alpha_c 4.45 (R = 72, A = 252), alpha_s 2.00, beta 1.76, f 1.99."""
    test = 'test_scan_gate_row_kernel_vs_fp64'
    g = gen(1000 * R + 10 * Mw + A)
    nb = B // row_div                                                  # entries of the per-image / per-group tensors
    x = dict(att_p=torch.relu(rn(g, nb, R, A)), att_e=torch.relu(rn(g, nb, R, A)), Gc=rn(g, nb, R, A, scale=0.5),
             qa=rn(g, B, A), qw=rn(g, B, A), zh=rn(g, B, A), q2=rn(g, nb, A) if with_q2 else None,
             wc=rn(g, A, scale=0.4), ws=rn(g, A, scale=0.4), wg=rn(g, A, scale=0.4),
             bc=rn(g, 1) if with_bias else None, bs=rn(g, 1) if with_bias else None, bg=rn(g, 1) if with_bias else None,
             b_gc=rn(g, A, scale=0.3), b_gs=rn(g, A, scale=0.3))
    if gather:
        nw = 23
        x.update(words_p=torch.relu(rn(g, nw, A)), words_e=torch.relu(rn(g, nw, A)), Gs=rn(g, nw, A, scale=0.5),
                 ids=torch.randint(0, nw, (nb, Mw + 2), generator=g))
    else:
        x.update(words_p=torch.relu(rn(g, nb, Mw, A)), words_e=torch.relu(rn(g, nb, Mw, A)), Gs=rn(g, nb, Mw, A, scale=0.5),
                 ids=None)
    xd = {k: (None if v is None else v.to(DEV)) for k, v in x.items()}
    out_v, out_s = sent(B, A), sent(B, A)
    aC, aS, beta, f = sent(B + 1, R + 3), sent(B + 1, Mw + 2), sent(B + 1, 3), sent(B + 1, A)
    pl_flat = torch.full((2 * (B + 1) * A,), SENT, device=DEV, dtype=torch.float16) if planes else None
    pl_view = pl_flat[:2 * B * A].view(2, B, A) if planes else None
    ids_view = None if xd['ids'] is None else xd['ids'][:, :Mw]
    scans = [ops.scan_problem(xd['att_p'], xd['att_e'], xd['qa'], xd['wc'], xd['bc'], out_v, aC[:B, :R], row_div=row_div),
             ops.scan_problem(xd['words_p'], xd['words_e'], xd['qw'], xd['ws'], xd['bs'], out_s, aS[:B, :Mw], q2=xd['q2'],
                              row_ids=ids_view, row_div=row_div)]
    with routes(test, [scan_route(R, Mw)]):
        ops.attn_scan_gate_fwd(scans, (xd['Gc'], xd['Gs']), xd['zh'], xd['b_gc'],
                               xd['b_gs'], xd['wg'], xd['bg'], f[:B], beta[:B, :1], f_planes=pl_view)
        torch.cuda.synchronize()
    tag = '[B%d,R%d,Mw%d,A%d%s%s%s,div%d]' % (B, R, Mw, A, ',ids' if gather else '', ',q2' if with_q2 else '',
                                              ',bias' if with_bias else '', row_div)
    ref, ev = RR.both(RR.gated_scan_ref, x['att_p'], x['att_e'], x['Gc'], x['words_p'], x['words_e'], x['Gs'], x['qa'], x['qw'],
                      x['zh'], x['wc'], x['bc'], x['ws'], x['bs'], x['b_gc'], x['b_gs'], x['wg'], x['bg'], x['q2'],
                      None if x['ids'] is None else x['ids'][:, :Mw], row_div, row_div)
    check_output(aC, ref['alpha_c'], ev['alpha_c'], 'rows:scan1/alpha_c' + tag, pad='sentinel')
    check_output(aS, ref['alpha_s'], ev['alpha_s'], 'rows:scan1/alpha_s' + tag, pad='sentinel')
    check_output(beta, ref['beta'], ev['beta'], 'rows:scan1/beta' + tag, pad='sentinel')
    check_output(f, ref['f'], ev['f'], 'rows:scan1/f' + tag)
    assert bool((out_v == SENT).all()) and bool((out_s == SENT).all())         # v and s on their own are not this form's
    if planes:
        assert torch.equal(pl_view.cpu(), S16.planes(f[:B].cpu())), tag
        assert bool((pl_flat[pl_view.numel():] == SENT).all()), tag
    DONE.add('%s[%d-%d-%d-%d]' % (test, B, R, Mw, A))


# ------------------------------------------------------------------------------------------------ the classifier alone
VOCAB = [(130, 64), (300, 516), (300, 2308), (4100, 32), (8196, 32), (12292, 32), (5000, 768), (8192, 1024)]


@functools.lru_cache(maxsize=1)
def _vocab_weights(V, K):
    g = gen(V + K)
    W, bias = rn(g, V, K, scale=2.0 * K ** -0.5), rn(g, V)
    return W, bias, W.to(DEV), bias.to(DEV)


def _run_vocab(test, h_d, Wd, bd, M, V, K, last_d, ban=None, live=None, nt=1, want_route=True):
    tw = ops.rows_stats_tile(V)
    nt_ = cdiv(V, tw)
    o = dict(pmax=sent(M + 1, nt_), psum=sent(M + 1, nt_), pidx=sent(M + 1, nt_, dtype=torch.int32),
             logits=sent(M + 1, V + 5), cand_val=sent(M + 1, nt_, KC), cand_idx=sent(M + 1, nt_, KC, dtype=torch.int32))
    x = _lib.RowsExt()
    x.stats_tile, x.beam = tw, 5
    x.pad_id, x.sos_id, x.unk_id, x.mask_special, x.decoding_constraint = 0, 1, 3, 1, 1
    x.last_word, x.cand_val, x.cand_idx = last_d.data_ptr(), o['cand_val'].data_ptr(), o['cand_idx'].data_ptr()
    if live is not None:
        x.live_in = live.data_ptr()
    b = None
    if ban is not None:
        b = _lib.RowsBan()
        b.ids, b.cnt, b.ld = ban[0].data_ptr(), ban[1].data_ptr(), ban[0].stride(0)
    assert ops.rows_vocab_supported(M, V, K)
    with nt_mode(nt):
        with routes(test, [vocab_route(M, V, K, nt >= 1, ban is not None)]):
            ops.rows_vocab_fwd(h_d, Wd, bd, o['pmax'], o['psum'], o['pidx'], x, o['logits'][:M], ban=b)
            torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


@pytest.mark.parametrize('M', [1, 4, 5, 8])
@pytest.mark.parametrize('V,K', VOCAB)
def test_classifier_alone_vs_fp64(V, K, M):
    """rows_vocab_kernel through isc_rows_vocab_fwd / isc_rows_vocab_banned_fwd: NP = 1 ... 4 with four column groups
    (K <= 512), NP = 2 ... 4 with two (K = 516 ... 1024) and NP = 4 with one (K = 2308: ten slices, the second trip of the
    eight slice waves, a ragged last slice of 4 floats), at MR 2 / 4 / 6 / 8, without and with ban lists (0, 8 and 9
    entries per row - more than 8 walks the list from memory - and ids outside [0, V), which ban nothing), logits in rows
    V + 5 wide.  Each launch again under the other two cache policies: same bits.
    Measured (MI355X, worst ratio over the 64 launches): logits 0.93 (V = 4100, K = 32), psum 0.93, the folded
    log-sum-exp 0.47."""
    test = 'test_classifier_alone_vs_fp64'
    W, bias, Wd, bd = _vocab_weights(V, K)
    g = gen(7 * V + K + M)
    h = rn(g, M, K)
    last = torch.randint(4, V, (M,), generator=g)
    ref, ev = RR.both(RR.classifier_ref, h, W, bias)
    # the lists hold the ids that matter: the row's best unmasked ids at entries 8 (reached only by the walk of more than
    # 8 entries; beyond the count of the rows with 8), 0 and 7 (the first and the last lane-held entry)
    top = ref['logits'].clone()
    top[:, [0, 1, 3]] = -float('inf')
    top[torch.arange(M), last] = -float('inf')
    top = top.topk(3, dim=1).indices
    ids = torch.randint(4, V, (M, 12), generator=g)
    ids[:, 2], ids[:, 5] = -1, V                                       # outside [0, V): nothing is banned
    ids[:, 8], ids[:, 0], ids[:, 7] = top[:, 0], top[:, 1], top[:, 2]
    cnt = torch.tensor([(9, 0, 8)[m % 3] for m in range(M)], dtype=torch.int32)
    h_d, last_d, ban = h.to(DEV), last.to(DEV), (ids.to(DEV), cnt.to(DEV))
    tw = ops.rows_stats_tile(V)
    for lists in (None, ban):
        tag = '[V%d,K%d,M%d%s]' % (V, K, M, ',ban' if lists else '')
        o = _run_vocab(test, h_d, Wd, bd, M, V, K, last_d, lists)
        check_output(o['logits'], ref['logits'], ev['logits'], 'rows:vocab1/logits' + tag, pad='sentinel')
        lg = o['logits'][:M, :V].contiguous()
        _check_classifier(tag, lg, o['pmax'], o['psum'], o['pidx'], o['cand_val'], o['cand_idx'], tw,
                          _banned(lg, last, (ids, cnt) if lists else None), M)
        r2, e2 = RR.both(RR.lse_of_logits, lg)
        got = RR.lse_ref(RR.F32, lg, o['pmax'][:M], o['psum'][:M])['lse']
        check_output(got, r2['lse'], e2['lse'], 'rows:vocab1/lse' + tag)
        for mode in (0, 2):
            o2 = _run_vocab(test, h_d, Wd, bd, M, V, K, last_d, lists, nt=mode)
            for k in o:
                assert torch.equal(o[k], o2[k]), (tag, mode, k)
    DONE.add('%s[%d-%d-%d]' % (test, V, K, M))


TIES = [(300, 64, 3), (4100, 32, 5), (5000, 768, 8)]


@pytest.mark.parametrize('V,K,M', TIES)
def test_classifier_ties_take_the_smaller_id(V, K, M):
    """Duplicate weight rows and biases: equal logits (in bits: every column is contracted in the same order) at several
    ids of one tile - more of them than the ROWS_KC = 8 candidate slots hold - and in two tiles.  pidx, the candidate ids
    and their order then take the smaller id, exactly; the values past the eighth equal one are cut, not a smaller id."""
    test = 'test_classifier_ties_take_the_smaller_id'
    g = gen(V + M)
    tw = ops.rows_stats_tile(V)
    W, bias = rn(g, V, K, scale=K ** -0.5), rn(g, V, scale=0.1)
    big = rn(g, K, scale=3.0 * K ** -0.5)
    t0, t1 = 2 * tw, 5 * tw
    dup0 = [t0 + c for c in (1, 2, 4, 5, 7, 8, 9, 11, 13, 15)]         # ten equal columns in tile 2: two are cut
    dup1 = [t1 + c for c in (3, 14)] + [t1 + tw + 0]                   # and the same value in tiles 5 and 6
    W[dup0 + dup1], bias[dup0 + dup1] = big, 0.25
    W[7], bias[7] = W[6], bias[6]                                      # an ordinary pair in tile 0
    h = big[None, :] * torch.linspace(1.0, 2.0, M)[:, None] + rn(g, M, K, scale=0.01)      # the duplicates win every row
    last = torch.full((M,), dup0[0], dtype=torch.int64)                # ... and the first of them is the row's last word
    o = _run_vocab(test, h.to(DEV), W.to(DEV), bias.to(DEV), M, V, K, last.to(DEV))
    lg = o['logits'][:M, :V].contiguous()
    assert bool((lg[:, dup0] == lg[:, dup0[:1]]).all()) and bool((lg[:, dup1] == lg[:, dup0[:1]]).all())
    assert bool((lg[:, 7] == lg[:, 6]).all())
    assert bool((lg[:, dup0[0]] > lg[:, :t0].max(1).values).all())
    _check_classifier('[ties,V%d]' % V, lg, o['pmax'], o['psum'], o['pidx'], o['cand_val'], o['cand_idx'], tw,
                      _banned(lg, last), M)
    assert o['pidx'][:M, 2].tolist() == [dup0[0]] * M and o['pidx'][:M, 5].tolist() == [dup1[0]] * M
    assert o['cand_idx'][:M, 2].tolist() == [dup0[1:9]] * M            # the last word is masked; then the eight smallest ids
    assert o['cand_idx'][:M, 5, :2].tolist() == [dup1[:2]] * M and o['cand_idx'][:M, 6, 0].tolist() == [dup1[2]] * M
    DONE.add('%s[%d-%d-%d]' % (test, V, K, M))


def test_classifier_live_flag():
    """isc_rows_ext.live_in on a lone classifier launch: -> 0 nothing is written, -> 1 the bits of the call without it."""
    test = 'test_classifier_live_flag'
    V, K, M = 300, 516, 5
    W, bias, Wd, bd = _vocab_weights(V, K)
    g = gen(5)
    h_d, last_d = rn(g, M, K).to(DEV), torch.randint(4, V, (M,), generator=g).to(DEV)
    base = _run_vocab(test, h_d, Wd, bd, M, V, K, last_d)
    o1 = _run_vocab(test, h_d, Wd, bd, M, V, K, last_d, live=torch.ones(1, dtype=torch.int32, device=DEV))
    o0 = _run_vocab(test, h_d, Wd, bd, M, V, K, last_d, live=torch.zeros(1, dtype=torch.int32, device=DEV))
    for k in base:
        assert torch.equal(o1[k], base[k]), k
        assert bool((o0[k] == (SENT if o0[k].dtype.is_floating_point else ISENT)).all()), k
    DONE.add(test)


def test_default_shape_keeps_its_route():
    """H = 512, V = 10000 (the shape bench.py's searches decode at): S = 2, J = 4, NP = 3, non-temporal, at MR 6."""
    test = 'test_default_shape_keeps_its_route'
    V, K, M = 10000, 512, 5
    assert vocab_route(M, V, K, True, False) == ('vocab', 6, 3, 1, 0, 2, 4, 2)
    W, bias, Wd, bd = _vocab_weights(V, K)
    g = gen(9)
    h = rn(g, M, K)
    o = _run_vocab(test, h.to(DEV), Wd, bd, M, V, K, torch.randint(4, V, (M,), generator=g).to(DEV))
    ref, ev = RR.both(RR.classifier_ref, h, W, bias)
    check_output(o['logits'], ref['logits'], ev['logits'], 'rows:vocab1/logits[V10000,K512,M5]', pad='sentinel')
    DONE.add(test)


# ------------------------------------------------------------------------------------------------ the report
def _every_launching_test():
    steps = ['[%s-%d]' % kr for kr in STEP_RUNS]
    return set(['test_step_stage_by_stage_vs_fp64' + x for x in steps]
               + ['test_step_cache_policies_and_live_flag_agree_in_bits' + x for x in steps]
               + ['test_scan_gate_row_kernel_vs_fp64[%d-%d-%d-%d]' % c[:4] for c in SCAN]
               + ['test_classifier_alone_vs_fp64[%d-%d-%d]' % (V, K, M) for V, K in VOCAB for M in (1, 4, 5, 8)]
               + ['test_classifier_ties_take_the_smaller_id[%d-%d-%d]' % c for c in TIES]
               + ['test_classifier_live_flag', 'test_default_shape_keeps_its_route'])


def _design_table():
    """instantiation -> test, from the table of DESIGN.md ("The few-row kernels: which shape reaches which instantiation")."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'DESIGN.md')).read()
    return dict(re.findall(r'^\| `(rows_[a-z_]+kernel(?:<[^>]*>)?)` \| `(test_[a-z0-9_]+)` \|', src, flags=re.M))


def test_zz_report_the_measured_ratios_and_the_routes():
    """Prints the worst ratio of every output this file measured and the instantiations it launched (pytest -s); every
    ratio is within the rule's 8, and - when every launching test of the file ran - the instantiations launched are exactly
    the table of DESIGN.md: 16 rows_lstm_kernel, 4 rows_linear_kernel, 64 rows_vocab_kernel, rows_scan_gate_kernel."""
    mine = {k: v for k, v in WORST.items() if k.startswith('rows:')}
    for k in sorted(mine):
        err, err32, ratio, name = mine[k]
        print('WORST %-28s ratio %5.2f  err_kernel %.3e  err32 %.3e  at %s' % (k, ratio, err, err32, name))
    for k in sorted(SEEN):
        print('ROUTE | `%s` | `%s` |' % (k, '`, `'.join(sorted(SEEN[k]))))
    assert all(v[2] <= FR.FACTOR for v in mine.values())
    table = _design_table()
    assert len(table) == 16 + 4 + 64 + 1
    assert set(SEEN) <= set(table), sorted(set(SEEN) - set(table))
    if _every_launching_test() <= DONE:
        assert set(SEEN) == set(table), sorted(set(table) - set(SEEN))
        wrong = sorted(k for k, t in table.items() if t not in SEEN[k])
        assert not wrong, wrong
