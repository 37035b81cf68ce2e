"""The two sibling unrolls of one training iteration as ONE step chain.

The reference runs the XE unroll (image regions, `forward_xe`, captioner.py:194-240) and the seq2seq unroll (sentiment
words, `forward_seq2seq`, captioner.py:242-288) of an iteration as two separate chains of per-step op launches
(train_xe.py:160-181, models/decoder.py:138-157).  Both go through the same `forward_step` (captioner.py:168-186) with
the same att-LSTM / lang-LSTM / classifier / word-embedding weights; only the attention differs (content attention over
the regions vs sentiment attention over the words, no gate in either).  At the reference's batch sizes (128 + 80 rows)
every launch of a step is latency-bound, so two chains cost twice the launches and nothing overlaps (two streams of
one-workgroup-per-CU kernels share nothing but the queue).

Here the rows of both calls form one row block per time step - XE rows first, seq2seq rows after them:
  * both LSTM cells, the classifier, every dX contraction of the reverse sweep and every dW contraction after it run
    ONCE over all rows;
  * the two h-projections are two problems of one launch, the two attention scans the two problems of one scan launch
    (isc_step_plan.pair_rows_c / isc_step_bwd_plan.pair_rows_c);
  * time-stacked activations are [T, B1 + B2, .]; what belongs to one branch only (its attention weights, scores,
    projections) stays in per-branch tensors.
Captions of different lengths (T1 != T2): steps past the shorter unroll run on the longer branch's rows alone; the
all-row contractions then see zeros in the idle rows (the stacks are zero-initialised in that case).

The step loops are the single form's (autograd.py): `_Rows` gives each step's row range [r0, r1) and active branches,
`_unroll` / `_step_fwd` run the forward steps, `_sweep` / `_step_bwd` the reverse ones.  The merged sweep always
accumulates into zeroed recurrent-gradient buffers (no `first` step): x + 0 == x, so a branch that joins the sweep late
(the shorter unroll) needs nothing special.
"""
import torch

from . import ops
from .autograd import (NN, _Grads, _Rows, _Saved, _classifier_bwd, _classify, _content_att_grads, _cpt2fc_bwd, _cpt_bwd,
                       _dims, _dlogits, _dropout_bwd, _dx_bwd, _fc_embed_bwd, _feed, _forward_buffers,
                       _has_keep, _keep_mask, _lstm_dw, _nn, _pad32, _region_embed_bwd, _scan_bwd, _senti2att_bwd,
                       _senti_att_grads, _senti_words_bwd, _step_bwd_plan, _sweep, _sweep_buffers, _unroll,
                       _weights_scope)


def use_pair(cap, in_graph):
    """Whether an iteration's two unrolls go through the merged step chain.  `captioner.pair_unrolls` (or the environment
    variable ISC_PAIR_UNROLLS = 0 / 1, for A/B runs) forces it; None = by measurement (MI355X, B = 128 + 80, V = 10k):
      eager steps         merged 4.9 ms   vs 6.4 ms one chain per unroll on two streams (the host enqueues ~600 launches)
      from HIP graphs     merged 5.3 ms   vs 4.85 ms two chains as two branches of the graph
    - the step kernels at 208 rows are two rounds of 32 x 32 tiles bound by operand traffic, so one chain saves launches,
    not kernel time, and a graph's two branches fill each other's tails.  Hence: merged when the host issues the
    launches, two branches when a graph does."""
    import os
    env = os.environ.get('ISC_PAIR_UNROLLS')
    v = getattr(cap, 'pair_unrolls', None)
    if env in ('0', '1'):
        v = env == '1'
    if v is None:
        return not in_graph
    return bool(v)


def pair_applicable(cap, masks1, masks2):
    """Both branches must agree on whether h_lang is dropped out (one keep-mask tensor and scale serve all rows)."""
    if ops.TIMER.armed or ops.TIMER.arm_step is not None:
        return False
    return _has_keep(cap, [masks1]) == _has_keep(cap, [masks2])


# ------------------------------------------------------------------------------ forward
def _pair_forward(cap, xe, s2s, lazy=None):
    """xe = (fc, att, cpt_words, tokens_in [B1,T1], senti_labels, ss_prob, masks); s2s = (cpt_words, senti_words,
    tokens_in [B2,T2], senti_labels, ss_prob, masks).  Returns (logp1 [B1,T1,V], logp2 [B2,T2,V], S) - or, with
    lazy = (targets1 [B1,T1], targets2 [B2,T2]) (Captioner.token_logprobs), log p(target) [B1,T1] / [B2,T2] straight from
    the raw logits: the two [B,T,V] log-prob tensors are then never formed (autograd._train_forward, `lazy`)."""
    p = cap._p()
    H, V = cap.settings['rnn_hid_dim'], cap.vocab_size
    fc, att, cpt1, tok1, lab1, ss1, masks1 = xe
    cpt2, sw2, tok2, lab2, ss2, masks2 = s2s
    (B1, T1), (B2, T2) = tok1.shape, tok2.shape
    Bt = B1 + B2
    S = _Saved()
    S.p, S.B1, S.B2, S.T1, S.T2 = p, B1, B2, T1, T2
    pre1 = cap._new(Bt, 4 * H)
    P1 = cap._prologue(p, 'xe', fc, att, cpt1, None, lab1, masks1, pre1_out=pre1[:B1])
    S.fc_feats1, S.cpt_feats1 = cap.fc_feats, cap.cpt_feats
    P2 = cap._prologue(p, 'seq2seq', None, None, cpt2, sw2, lab2, masks2, pre1_out=pre1[B1:])
    S.cpt_feats2 = cap.cpt_feats
    P1.fc_pre, P1.cpt_pre = S.fc_feats1, S.cpt_feats1
    P2.fc_pre, P2.cpt_pre = None, S.cpt_feats2
    S.P1, S.P2, S.pre1 = P1, P2, pre1
    # captions of different lengths: steps past the shorter unroll run on the longer one's rows alone (L.short)
    L = S.L = _Rows([(0, B1, T1), (B1, B2, T2)])
    T = L.T
    sched = cap.training and (ss1 > 0.0 or ss2 > 0.0)
    _forward_buffers(cap, S, L, [P1, P2], _has_keep(cap, [masks1, masks2]), sched)
    _keep_mask(cap, S, L, [masks1, masks2])
    emb = p['word_embed.0.weight']
    ss = _feed(cap, S, L, [tok1, tok2], [ss1, ss2], emb)

    # plans: both branches / XE rows alone / seq2seq rows alone (the last two only past the shorter unroll)
    Pm = type(P1)()
    Pm.B, Pm.R, Pm.Mw = Bt, P1.R, P2.Mw
    Pm.att_e3, Pm.att_p3 = P1.att_e3, P1.att_p3
    Pm.words_e3, Pm.words_p3, Pm.label_w = P2.words_e3, P2.words_p3, P2.label_w
    Pm.pre1 = pre1
    plans = {(True, True): cap._make_plan(p, Pm, Bt)}
    plans[(True, True)].pair_rows_c = B1
    if T1 != T2:
        Pc = type(P1)()
        Pc.B, Pc.R, Pc.att_e3, Pc.att_p3, Pc.pre1 = B1, P1.R, P1.att_e3, P1.att_p3, pre1[:B1]
        Ps = type(P1)()
        Ps.B, Ps.Mw, Ps.words_e3, Ps.words_p3, Ps.label_w, Ps.pre1 = B2, P2.Mw, P2.words_e3, P2.words_p3, P2.label_w, pre1[B1:]
        plans[(True, False)] = cap._make_plan(p, Pc, B1)
        plans[(False, True)] = cap._make_plan(p, Ps, B2)
    out1, out2 = (cap._new(B1, T1, V), cap._new(B2, T2, V)) if lazy is None else (cap._new(B1, T1), cap._new(B2, T2))
    with _weights_scope(cap):
        # (a per-step classifier only when a step's logits feed the next draw)
        raw = cap._new(T, Bt, V) if sched else None       # raw logits, time-major: normalised per branch afterwards
        _unroll(cap, S, L, plans, raw, ss)
        if not sched:
            raw = _classify(cap, S, L)
        S.lazy = None
        if lazy is None:
            ops.logsoftmax_apply_steps(out1, S.pm[:T1, :B1], S.ps[:T1, :B1], src_tbv=raw[:T1, :B1], step_rows=Bt)
            ops.logsoftmax_apply_steps(out2, S.pm[:T2, B1:], S.ps[:T2, B1:], src_tbv=raw[:T2, B1:], step_rows=Bt)
        else:                                  # log p(target) per row from the raw logits; the backward reads them again
            S.lazy = (raw, S.pm, S.ps, lazy[0].contiguous(), lazy[1].contiguous())
            ops.gather_logp_raw(raw, V, Bt * V, B1, T1, V, S.pm, S.ps, Bt, S.lazy[3], out1)
            ops.gather_logp_raw(raw[0, B1:], V, Bt * V, B2, T2, V, S.pm[0, B1:], S.ps[0, B1:], Bt, S.lazy[4], out2)
    del raw
    S.pm = S.ps = S.pi = None                  # (the lazy backward reads its statistics through S.lazy)
    # the state the reference's attributes are in after its second call (forward_seq2seq): sentiment weights only
    cap._set_weights(None, S.aS, None, T2)
    S.logp1, S.logp2 = out1, out2
    return out1, out2, S


# ------------------------------------------------------------------------------ backward
def _pair_backward(cap, S, d1, d2, sparse1, sparse2, d_fc_feats1, d_cpt_feats1, d_cpt_feats2):
    """{param name: gradient} of both unrolls.  d1 / d2: dense d log-prob of the two outputs (None when the criteria
    handed theirs over sparse: sparse1 / sparse2 = [(ids, coef)]); optional gradients of the attribute tensors.  The
    stages around the reverse sweep are autograd._backward's, called once per branch where a branch's rows differ.

    With a gradient sink on the captioner (`cap._grad_sink`, dp.GradSink: the data-parallel step) every gradient is
    written straight into its view of the flat arena, the parameters are finished bucket by bucket - classifier (before
    the sweep), lang-LSTM + attention, att-LSTM + projections, embeddings + fc - and each bucket's all-reduce starts as
    soon as its last contraction is enqueued; the returned dictionary is then empty.  Same kernels, same values."""
    p, P1, P2, L = S.p, S.P1, S.P2, S.L
    B1, B2, T1, T2 = S.B1, S.B2, S.T1, S.T2
    Bt, T = L.Bt, L.T
    E, _, H, Wd, V = _dims(cap)
    new, zeros = cap._new, cap._zeros
    TB = T * Bt
    g = _Grads(cap, p, getattr(cap, '_grad_sink', None))
    if (P1.label_e is None) != (P2.label_e is None):
        raise ValueError('merged unrolls: sentiment labels for both calls or for neither')

    # ---- gradient scale: one power of two for everything that enters the sweep
    # the sweep always accumulates (no `first` step): its recurrent gradients, running sums, per-row partials of the
    # alpha weights and the h-projection gradients of each branch padded to all rows come out of the one fill
    # (dG1_sum: rows padded to a multiple of 32 with zeros: its two dW contractions - over the B1 + B2 rows, e.g. 208 - then
    # run on the split-f16 kernels, whose contraction length is a multiple of 32; 190 us on the fp32 tiles otherwise)
    Bp = (Bt + 31) // 32 * 32
    D = _sweep_buffers(cap, g, S, L, True, Bp)
    scale, (d_fc_feats1, d_cpt_feats1, d_cpt_feats2) = g.scale(
        D.gs_z, [c for _, c in list(sparse1) + list(sparse2)], (d_fc_feats1, d_cpt_feats1, d_cpt_feats2), (d1, d2))

    # ---- classifier + log-softmax over all T*Bt rows (time-major)
    Vp = _pad32(V)
    idle1, idle2 = d1 is None and not sparse1, d2 is None and not sparse2
    dlogits = zeros(TB, Vp) if (L.short or idle1 or idle2) else new(TB, Vp)
    # (lazy: d1 / d2 arrived as [B,T] coefficients of the target columns - DecodePairFn)
    lz = S.lazy
    for d, sp, idle, lo, Bx, Tx, logp in ((d1, sparse1, idle1, 0, B1, T1, S.logp1),
                                          (d2, sparse2, idle2, B1, B2, T2, S.logp2)):
        if not idle:
            _dlogits(lz and (lz[0][0, lo:], V, Bt * V, lz[1][0, lo:], lz[2][0, lo:]), d, logp, sp, dlogits[lo:], Bx, Tx,
                     V, Bt, scale)
    dhd = _classifier_bwd(cap, g, dlogits, (S.hdrop if S.hdrop is not None else S.h2[1:]).reshape(TB, H))
    g.bucket_done(3)                    # classifier: its exchange runs behind the whole reverse sweep
    _dropout_bwd(S, dhd)

    plans = {}
    for act in set(a for _, _, a in L.steps):
        plans[act] = _step_bwd_plan(cap, p, P1 if act[0] else None, P2 if act[1] else None)
        plans[act].pair_rows_c = B1 if all(act) else 0
    h1_prev, h1_cur, h2_prev, xt_tb, feat_tb = _sweep(cap, S, L, plans, D, dhd.view(T, Bt, H), False)
    dG1f, dG2f, dG1_sum = D.dG1, D.dG2, D.dG1_sum[:Bt]

    # ---- bucket 2: lang-LSTM and the attention's own parameters - one contraction over all T*Bt rows each
    _lstm_dw(g, None, dG2f, h1_prev, h1_cur, h2_prev, xt_tb, feat_tb, None, None, None)
    _content_att_grads(g, D.dqa, h1_cur, D.dwc_rows)
    d_label_w = _senti_att_grads(cap, g, D.dqw, h1_cur, D.dws_rows, P2.label_e, lo=B1)
    g.bucket_done(2)

    # ---- bucket 1: att-LSTM, region embedding + projection (XE branch), sentiment-word projection (seq2seq branch)
    pad = [_const_zeros(cap, Bp - Bt, E)] if Bp > Bt else []
    fc_e_all = torch.cat([P1.fc_e, P2.fc_e] + pad)
    label_e_all = None
    if P1.label_e is not None:
        label_e_all = torch.cat([P1.label_e, P2.label_e] + ([_const_zeros(cap, Bp - Bt, Wd)] if Bp > Bt else []))
    _lstm_dw(g, dG1f, None, h1_prev, h1_cur, h2_prev, xt_tb, feat_tb, D.dG1_sum, fc_e_all, label_e_all)
    dP_att, dV_att = _scan_bwd(cap, P1.att_p3, P1.att_e3, S.aC, S.qa, D.d_feat[:T1, :B1], D.de_c,
                               p['attention.cont_att.att_alpha.weight'], step_rows=Bt)
    dP_w, dV_w = _scan_bwd(cap, P2.words_p3, P2.words_e3, S.aS, S.qw, D.d_feat[:T2, B1:], D.de_s,
                           p['attention.senti_att.word_alpha.weight'], step_rows=Bt, q2=P2.label_w)
    _region_embed_bwd(cap, g, P1, dP_att, dV_att)
    dzw = _senti2att_bwd(cap, g, P2, dP_w)
    g.bucket_done(1)

    # ---- bucket 0: the word / label embeddings, fc_embed, cpt2fc
    d_fc_e, d_label_e, dEmb = _dx_bwd(cap, g, dG1f, dG1_sum, S.tok.view(-1), label_e_all is not None)
    if d_label_w is not None:
        ops.gemm_bwd([_nn([(d_label_w, p['attention.senti_att.label2word.weight'])], d_label_e[B1:], True)], NN)
    if d_label_e is not None:
        dL = g.gout('senti_label_embed.0.weight')
        for P, lo, hi in ((P1, 0, B1), (P2, B1, Bt)):
            ops.embed_relu_bwd(p['senti_label_embed.0.weight'], P.label_ids, d_label_e[lo:hi], dL, hi - lo,
                               keep_mask=P.m_label, mask_scale=P.sc)
    _senti_words_bwd(cap, g, P2, dzw, dV_w, dEmb)
    # fc_embed (XE rows) and cpt2fc (XE rows: only through the cpt_feats attribute; seq2seq rows: fc_e := dropout(cpt))
    _fc_embed_bwd(cap, g, P1, d_fc_e[:B1], d_fc_feats1)
    d_cpt = zeros(Bt, E) if d_cpt_feats1 is None else new(Bt, E)
    if d_cpt_feats1 is not None:
        _cpt_bwd(cap, P1, None, d_cpt_feats1, d_cpt[:B1])
    _cpt_bwd(cap, P2, d_fc_e[B1:], d_cpt_feats2, d_cpt[B1:])
    _cpt2fc_bwd(cap, g, d_cpt, (P1, P2), dEmb)
    g.bucket_done(0)
    return g.finish()


def _const_zeros(cap, rows, width):
    """A read-only block of zeros, kept per captioner (padding rows of the merged dW contractions): no fill per call."""
    cache = cap.__dict__.setdefault('_zero_blocks', {})
    key = (rows, width, str(cap._dev))
    z = cache.get(key)
    if z is None:
        z = cache[key] = torch.zeros(rows, width, dtype=torch.float32, device=cap._dev)
    return z


class DecodePairFn(torch.autograd.Function):
    """(xe inputs, seq2seq inputs, *params) -> (logp_xe, cpt_feats_xe, fc_feats_xe, logp_s2s, cpt_feats_s2s)."""
    LOGP_SLOTS = (0, 3)          # output numbers of the two log-prob tensors (the criteria's sparse side channels)

    @staticmethod
    def forward(ctx, cap, xe, s2s, names, lazy, *params):
        with torch.no_grad():
            out1, out2, S = _pair_forward(cap, xe, s2s, lazy)
        ctx.cap, ctx.S, ctx.names = cap, S, names
        ctx._isc_sparse = {0: [], 3: []}          # per log-prob output (autograd.sparse_channel)
        ctx.set_materialize_grads(False)
        return out1, S.cpt_feats1.clone(), S.fc_feats1.clone(), out2, S.cpt_feats2.clone()

    @staticmethod
    def backward(ctx, d1, d_cpt1, d_fc1, d2, d_cpt2):
        cap, S = ctx.cap, ctx.S
        sp, ctx._isc_sparse = ctx._isc_sparse, {0: [], 3: []}
        with torch.no_grad():
            if S.lazy is not None:             # d1 / d2 = d log p(target) [B,T]: one column per row
                if d1 is not None:
                    sp[0], d1 = [(S.lazy[3], d1.contiguous())], None
                if d2 is not None:
                    sp[3], d2 = [(S.lazy[4], d2.contiguous())], None
            G = _pair_backward(cap, S, d1.contiguous() if d1 is not None else None,
                               d2.contiguous() if d2 is not None else None, sp[0], sp[3], d_fc1, d_cpt1, d_cpt2)
        ctx.S = None
        return (None,) * 5 + tuple(G.get(n) for n in ctx.names)


def pair_with_grad(cap, fc, att, cpt_words, captions, senti_labels, ss_prob, s_captions, s_cpt_words, s_senti_words,
                   s_senti_labels, s_ss_prob, masks, s_masks, targets=None, s_targets=None):
    """forward_xe + forward_seq2seq of one iteration through one step chain.  Returns (logp_xe, logp_s2s, cpt_feats of
    the seq2seq call); captioner.fc_feats / .cpt_feats are left as the XE call leaves them (what the domain-align loss
    reads, train_xe.py:163)."""
    fc, att = cap._f32(fc), cap._f32(att)          # (as autograd.xe_with_grad: fp32 once, in front of the prologue)
    names = [n for n, q in cap.named_parameters() if q.requires_grad]
    params = [q for _, q in cap.named_parameters() if q.requires_grad]
    ids1, ids2 = cap._ids(captions), cap._ids(s_captions)
    tok1, tok2 = ids1[:, :-1].contiguous(), ids2[:, :-1].contiguous()
    xe = (fc, att, cpt_words, tok1, senti_labels, float(ss_prob), masks)
    s2s = (s_cpt_words, s_senti_words, tok2, s_senti_labels, float(s_ss_prob), s_masks)
    lazy = None
    if cap.__dict__.get('_token_logprobs'):
        lazy = (ids1[:, 1:].contiguous() if targets is None else cap._ids(targets).contiguous(),
                ids2[:, 1:].contiguous() if s_targets is None else cap._ids(s_targets).contiguous())
    outs = DecodePairFn.apply(cap, xe, s2s, names, lazy, *params)
    cap.cpt_feats, cap.fc_feats = outs[1], outs[2]
    return outs[0], outs[3], outs[4]
