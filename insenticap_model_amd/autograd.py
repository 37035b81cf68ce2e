"""Training path: forward with saved activations + hand-written BPTT on the HIP kernels.

The reference relies on stock torch autograd through its per-step op graph
(train_xe.py:189-190, decoder.py:164-165).  Here one `torch.autograd.Function` covers a whole
call (prologue + T-step unroll): its forward writes every per-step activation straight into
time-stacked buffers [T(+1), B, ...], and its backward is a reverse sweep in which
  * the recurrence only runs input-gradient contractions (isc_gemm_bwd NN) and the
    pointwise / scan backward kernels, and
  * every weight gradient is ONE contraction over all T*B rows after the sweep (isc_gemm_bwd TN)
    - weights are shared across time, so nothing is lost by deferring them.
torch is used for memory, the autograd hook-up and (train mode) random numbers only.
"""
import itertools
import math

import torch

from . import _lib, ops

NN, TN = ops.NN, ops.TN


class _Saved:
    xt = hdrop = keep = qa = aC = qw = aS = v = s = z = bG = None      # (what an unroll has no use for stays None)



def _weights_scope(cap):
    """Weights scope keyed by the parameter VALUES (Captioner._weights_key): the forward unrolls of one training
    iteration (sampled roll-out, XE, the greedy baseline in between) and its backward sweeps all see the same weights,
    so the f16 planes - forward layout and transposes - are built once per iteration and stream, not once per scope
    (91 -> ~40 split launches per RL iteration at B=512)."""
    return ops.h3_weights_scope(cap._dev, key=cap._weights_key())


def _pad32(v):
    return (v + 31) // 32 * 32


# ------------------------------------------------------------------------------ the step loops of both forms
# (_train_forward / _backward below and autograd_pair's merged unroll run the same loops; only the data differ)
class _Rows:
    """Row layout of a training unroll: [T, Bt, .] stacks; block k = (lo, B_k, T_k) owns rows [lo, lo + B_k) for steps
    < T_k (single form: one block; merged form: XE rows, then seq2seq rows); `counts` (ragged, one block): step t runs
    rows [0, counts[t]).  steps[t] = (r0, r1, active blocks); short: some step runs fewer than Bt rows (or ragged)."""

    def __init__(self, blocks, counts=None):
        self.blocks, self.Bt, self.T = blocks, sum(b[1] for b in blocks), max(b[2] for b in blocks)
        self.steps = []
        for t in range(self.T):
            act = tuple(t < Tk for _, _, Tk in blocks)
            on = [(lo, lo + Bk) for (lo, Bk, _), a in zip(blocks, act) if a]
            self.steps.append((on[0][0], on[-1][1] if counts is None else counts[t], act))
        self.short = counts is not None or any(r1 - r0 < self.Bt for r0, r1, _ in self.steps)


def _at(x, row=None):
    """(address of x[t] per t, bytes per row) of a [T, rows, .] view: at the step's first row r0, or at a fixed `row`."""
    e = x.element_size()
    b = x.data_ptr() + (row or 0) * x.stride(1) * e
    return [b + t * x.stride(0) * e for t in range(x.shape[0])], (x.stride(1) * e if row is None else 0)


def _steps(L, plans, common, blocks, ts, launch):
    """Step t of `ts`: its active blocks' plan gets rows r1 - r0 and the {field: _at(..)} pointers; then launch(t, plan)."""
    walks = {act: {**common, **{f: v for k, a in enumerate(act) if a for f, v in blocks[k].items()}} for act in plans}
    for t in ts:
        r0, r1, act = L.steps[t]
        pl = plans[act]
        pl.rows = r1 - r0
        for field, (bases, pitch) in walks[act].items():
            setattr(pl, field, bases[t] + r0 * pitch)
        launch(t, pl)


def _lds(pl, S):
    """Leading dimensions of the attention weights and the gate's beta (a plan without that attention ignores them)."""
    pl.alpha_c_ld, pl.alpha_s_ld, pl.beta_ld = [0 if x is None else x.stride(0) for x in (S.aC, S.aS, S.bG)]


def _has_keep(cap, masks):
    """Whether h_lang is dropped out: explicit mask dicts (one per block) with out<t> keys, or train mode."""
    if any(m is not None for m in masks):
        return any(k.startswith('out') for m in masks if m is not None for k in m)
    return cap.training and cap.drop.p > 0.0


def _forward_buffers(cap, S, L, Ps, keep, zero_xt, extra=()):
    """The saved tensors (blocks from the prologues Ps): h / c [T+1, Bt, H] from a fill, the stacks (from one more fill
    when L.short) and the tile statistics.  Returns zero tensors for the (shape, dtype) specs `extra`."""
    E, A, H, Wd, V = _dims(cap)
    T, Bt = L.T, L.Bt
    S.att = {}
    st = {'feat': (T, Bt, E), 'hdrop': (T, Bt, H) if keep else None, 'xt': (T, Bt, Wd) if zero_xt and L.short else None}
    for k, ((lo, Bk, Tk), P) in enumerate(zip(L.blocks, Ps)):
        if P.att_e3 is not None:
            S.att['c'] = (k, lo)
            st.update(qa=(Tk, Bk, A), aC=(Bk, Tk, P.R))
        if P.words_e3 is not None:
            S.att['s'] = (k, lo)
            st.update(qw=(Tk, Bk, A), aS=(Bk, Tk, P.Mw))
        if P.att_e3 is not None and P.words_e3 is not None:
            st.update(v=(T, Bt, E), s=(T, Bt, E), z=(T, Bt, A), bG=(Bk, Tk))
    st = {k: sh for k, sh in st.items() if sh is not None}
    S.h1, S.c1, S.h2, S.c2 = cap._zeros(4, T + 1, Bt, H).unbind(0)
    vals = cap._zeros_many(*[(sh, torch.float32) for sh in st.values()]) if L.short else [cap._new(*sh) for sh in st.values()]
    S.__dict__.update(zip(st, vals))
    out = cap._zeros_many(*extra) if extra else []        # (their own fill: they outlive S)
    if S.xt is None:
        S.xt = cap._new(T, Bt, Wd)
    S.g1, S.g2 = cap._new(T, Bt, 4 * H), cap._new(T, Bt, 4 * H)      # (read back by the same step's rows only)
    S.tok = torch.full((T, Bt), cap.pad_id, dtype=torch.int64, device=cap._dev) if any(b[2] < T for b in L.blocks) \
        else torch.empty(T, Bt, dtype=torch.int64, device=cap._dev)
    n_tile = (V + 127) // 128
    S.pm, S.ps, S.pi = cap._new(T, Bt, n_tile), cap._new(T, Bt, n_tile), cap._new(T, Bt, n_tile, dtype=torch.int32)
    return out


def _keep_mask(cap, S, L, masks):
    """Dropout on h_lang (captioner.py:182): ONE [T, Bt, H] keep-mask (S.keep, S.out_scale) - drawn in one launch, or
    from explicit dicts (tests replay the reference's), which then hold out<t> for every step of their block."""
    H, p_drop = cap.settings['rnn_hid_dim'], cap.drop.p
    S.out_scale = 1.0 / (1.0 - p_drop) if p_drop < 1.0 else 0.0
    if S.hdrop is None:
        S.out_scale = 1.0
    elif all(m is None for m in masks):
        S.keep = torch.empty(L.T, L.Bt, H, dtype=torch.uint8, device=cap._dev).bernoulli_(1.0 - p_drop)
    else:
        S.keep = torch.ones(L.T, L.Bt, H, dtype=torch.uint8, device=cap._dev)
        for (lo, Bk, Tk), m in zip(L.blocks, masks):
            for t in range(Tk):
                mk, S.out_scale = cap._mask_source(m)('out%d' % t, Bk, H)
                if mk is None:
                    raise ValueError('explicit dropout masks: out%d is missing' % t)
                S.keep[t, lo:lo + Bk] = mk


def _feed(cap, S, L, toks, probs, emb):
    """Tokens of every block ([B_k, T_k] ids).  Known up front: one copy per block, one gather; returns None.  Scheduled
    sampling (captioner.py:219-228, on for some block): step 0 fed, the uniforms of every later step in ONE launch;
    returns what _unroll's per-step draws read: (ground-truth ids [T, Bt], uniforms, probability per block)."""
    if not (cap.training and any(q > 0.0 for q in probs)):
        for (lo, Bk, Tk), tk in zip(L.blocks, toks):
            S.tok[:Tk, lo:lo + Bk].copy_(tk.t())
        ops.embed_relu_fwd(emb, S.tok.view(-1), S.xt.view(L.T * L.Bt, -1))
        return None
    if len(toks) == 1 and tuple(toks[0].shape) == (L.Bt, L.T):
        base = toks[0].t()            # (one block covering every row and step: its ids serve as they are, no copy)
    else:
        base = torch.full((L.T, L.Bt), cap.pad_id, dtype=torch.int64, device=cap._dev)
        for (lo, Bk, Tk), tk in zip(L.blocks, toks):
            base[:Tk, lo:lo + Bk].copy_(tk.t())
    S.tok[0].copy_(base[0])
    ops.embed_relu_fwd(emb, S.tok[0], S.xt[0])
    return base, torch.rand(max(L.T - 1, 1), 2, L.Bt, device=cap._dev), probs


def _unroll(cap, S, L, plans, lg, sched=None, after=None):
    """The forward step loop of both forms: scheduled-sampling draws (sched: _feed's), isc_step_fwd, after(t).  lg: the
    [T, Bt, V] raw logits the steps write when a draw reads them, else None (the classifier runs after the loop)."""
    emb = S.p['word_embed.0.weight']
    common = dict(xt=_at(S.xt), h1_prev=_at(S.h1), c1_prev=_at(S.c1), h2_prev=_at(S.h2), c2_prev=_at(S.c2),
                  h1=_at(S.h1[1:]), c1=_at(S.c1[1:]), h2=_at(S.h2[1:]), c2=_at(S.c2[1:]), g1=_at(S.g1), g2=_at(S.g2))
    if S.keep is not None:
        common.update(out_mask=_at(S.keep), hdrop=_at(S.hdrop))
    if lg is not None:
        common.update(logits=_at(lg), pmax=_at(S.pm), psum=_at(S.ps), pidx=_at(S.pi))
    blocks = [{} for _ in L.blocks]
    if S.aC is not None:
        k, lo = S.att['c']
        blocks[k].update(qa=_at(S.qa, 0), v=_at(S.feat if S.v is None else S.v, lo), alpha_c=_at(S.aC.transpose(0, 1), 0))
    if S.aS is not None:
        k, lo = S.att['s']
        blocks[k].update(qw=_at(S.qw, 0), s=_at(S.feat if S.s is None else S.s, lo), alpha_s=_at(S.aS.transpose(0, 1), 0))
    if S.z is not None:
        blocks[0].update(z=_at(S.z), f=_at(S.feat), beta=_at(S.bG.t()))
    for pl in plans.values():
        _lds(pl, S)
        pl.out_scale, pl.ld_logits = S.out_scale, 0 if lg is None else lg.stride(1)

    def launch(t, pl):
        r0, r1, _ = L.steps[t]
        if sched is not None and t >= 1:
            draw(t, r0, r1)
        ops.step_fwd(pl)
        if after is not None:
            after(t)

    def draw(t, r0, r1):
        base, u_all, probs = sched
        u, spans = u_all[t - 1], []
        for (lo, Bk, Tk), prob in zip(L.blocks, probs):         # (neighbouring blocks with one probability: one span)
            if t < Tk:
                if spans and spans[-1][1] == lo and spans[-1][2] == prob:
                    spans[-1][1] = lo + Bk
                else:
                    spans.append([lo, lo + Bk, prob])
        for lo, hi, prob in spans:
            ops.sched_sample(lg[t - 1, lo:hi], S.pm[t - 1, lo:hi], S.ps[t - 1, lo:hi], S.pi[t - 1, lo:hi],
                             u[0, lo:hi], u[1, lo:hi], prob, base[t, lo:hi], S.tok[t, lo:hi], raw=True)
        ops.embed_relu_fwd(emb, S.tok[t, r0:r1], S.xt[t, r0:r1])
    _steps(L, plans, common, blocks, range(L.T), launch)


def _classify(cap, S, L):
    """The classifier ONCE over every step's h_lang [T*Bt, H]: raw logits [T, Bt, V], statistics into S.pm / ps / pi."""
    p, TB, V = S.p, L.T * L.Bt, cap.vocab_size
    hs = S.hdrop if S.hdrop is not None else S.h2[1:]
    raw = cap._new(L.T, L.Bt, V)                      # (every row is written: no fill in the ragged form)
    n_tile = S.pm.shape[2]
    ops.vocab_fwd(hs.reshape(TB, -1), p['classifier.weight'], p['classifier.bias'], S.pm.view(TB, n_tile),
                  S.ps.view(TB, n_tile), S.pi.view(TB, n_tile), raw.view(TB, V))
    return raw


# ------------------------------------------------------------------------------ forward
def _train_forward(cap, mode, fc, att, cpt_words, senti_words, tokens_in, senti_labels, ss_prob, masks, lazy=None,
                   group=1):
    """group = n > 1 (forward_xe captions_per_image): the prologue runs on the I images, the unroll on the I*n rows of
    tokens_in; the step plans carry row_div = n.  With the sampled roll-out (mode 'rl', forward_rl captions_per_image)
    EVERYTHING step-invariant is per image - label_e, label_w and the hoisted att-LSTM term pre1 included (the image's
    label serves all of its rows: the step reads pre1 at row // n) - and the unroll runs on I*n rows.
    Returns (logp [B,T,V], S). tokens_in [B,T]: ground-truth inputs (column 0 = <SOS>) - or, for the sampled
    roll-out with gradients, a dict {'T', 'u' (uniforms [B,T]) or 'forced' (raw draws [B,T])}: every step then
    draws its own next token on the device (isc_rollout_finalize) while the activations the backward pass
    needs are kept, so sampling and the differentiable forward are ONE unroll (captioner.py:290-349 does the
    same inside autograd).  The draws land in S.sample = (seq, masks, raw, alive).
    lazy: None, or the [B,T] int64 ids whose log-probs the caller's criterion reads (XECriterion's targets; True for the
    sampled roll-out: its own draws): the [B,T,V] log-probs are then NOT formed - the first return value is log p(id)
    [B,T] straight from the raw logits + tile statistics (isc_gather_logp_raw; the bits the tensor would have held), and
    the backward recomputes the softmax term from them (isc_logsoftmax_bwd_raw)."""
    p = cap._p()
    sampling = isinstance(tokens_in, dict)
    P = cap._prologue(p, mode, fc, att, cpt_words, senti_words, senti_labels, masks, group=1 if sampling else group)
    if sampling and group > 1:
        P.row_div = group                     # (pre_rows stays False: pre1 [I,4H], one row per image)
    Wd, V = cap.settings['word_emb_dim'], cap.vocab_size
    B, T = (P.B * group, tokens_in['T']) if sampling else tokens_in.shape
    sched = not sampling and cap.training and ss_prob > 0.0
    S = _Saved()
    S.p, S.P, S.mode, S.B, S.T = p, P, mode, B, T
    # Ragged unroll (Captioner.row_counts): the batch is sorted by caption length (the reference's collates,
    # dataloader.py:17,37,68,124), so the rows still inside their caption at step t are the prefix [0, counts[t]) - step t
    # runs on those rows only.  The criteria never read a position behind a caption's end (XECriterion's mask,
    # captioner.py:431-436), and its gradient is exactly zero: same loss, same gradients.  The [T,B] layout stays; what a
    # skipped row would have written must read as ZERO (gradients) or at least finite (activations next to a zero
    # gradient in the contractions over all T*B rows) - every buffer such a row belongs to comes out of a fill.
    counts = cap.__dict__.get('_row_counts')
    # (captions per image: the rows are image-major, not sorted by length - the full unroll, same loss and gradients)
    if counts is not None and (sampling or lazy is None or sched or len(counts) != T or counts[0] != B or group > 1):
        counts = None
    S.row_counts = counts
    L = S.L = _Rows([(0, B, T)], counts)
    extra = [((B, T), torch.int64), ((B, T), torch.float32), ((B, T), torch.float32), ((B, T), torch.int64),
             ((T + 1,), torch.int32)] if sampling else []
    flt = tokens_in.get('flt') if sampling else None
    if flt is not None:
        # filtered draws (temperature / top_k / top_p, or constraints with the sampling log-probs wanted): the sampling
        # log-probs and what their backward reads - K*, the largest allowed logit, log Z - per (b, t); zero behind the
        # early break (the finalize returns before writing)
        extra += [((B, T), torch.float32), ((B, T), torch.int64), ((B, T), torch.float32), ((B, T), torch.float32)]
    extra = _forward_buffers(cap, S, L, [P], _has_keep(cap, [masks]), False, extra)
    step_cls = sampling or sched                  # a draw reads each step's raw logits: the classifier runs per step
    out = None if (lazy is not None and not step_cls) else cap._new(B, T, V)   # (lazy, tokens known: raw logits only)
    emb = p['word_embed.0.weight']
    plans = {(True,): cap._make_plan(p, P, B)}
    after = None
    if sampling:
        from ._lib import RolloutStep
        seq, seq_lp, seq_masks, raw, alive = extra[:5]
        slp = saved = None
        if flt is not None:
            slp = extra[5]
            saved = dict(zip(('kstar', 'gmax', 'logz'), extra[6:9]))
            if tokens_in.get('cons') is not None:       # the row's banned ids, -1: unused (an unconstrained step writes none)
                saved['ban'] = torch.full((B, T, 10), -1, dtype=torch.int32, device=cap._dev)
        unfinished = torch.ones(B, dtype=torch.int32, device=cap._dev)
        alive[0:1].fill_(B)                     # a fill kernel (a scalar assignment would be a pageable H2D copy)
        forced, sample_u = tokens_in.get('forced'), tokens_in.get('u')
        rs = RolloutStep()
        rs.B, rs.V, rs.T, rs.n_tile, rs.W = B, V, T, S.pm.shape[2], Wd
        rs.ld_logits = out.stride(0)
        rs.forced, rs.sample_u, rs.eos_id = ops.ptr(forced), ops.ptr(sample_u), cap.eos_id
        rs.seq, rs.seq_logprobs, rs.seq_masks = seq.data_ptr(), seq_lp.data_ptr(), seq_masks.data_ptr()
        rs.unfinished, rs.alive, rs.raw_tokens = unfinished.data_ptr(), alive.data_ptr(), raw.data_ptr()
        rs.emb, rs.xt_add = emb.data_ptr(), None
        S.tok[0] = cap.sos_id
        ops.embed_relu_fwd(emb, S.tok[0], S.xt[0])

        def after(t):                                 # draw on the raw logits (normalised after the loop)
            rs.t, rs.logits = t, out[:, t].data_ptr()
            rs.part_max, rs.part_sum, rs.part_idx = S.pm[t].data_ptr(), S.ps[t].data_ptr(), S.pi[t].data_ptr()
            rs.xt_next = S.xt[t + 1].data_ptr() if t + 1 < T else None
            # (constraints: the draw runs over the allowed ids)
            ops.rollout_finalize_step(rs, tokens_in.get('cons'), flt, slp, saved)
            if t + 1 < T:
                S.tok[t + 1].copy_(seq[:, t])         # it * unfinished, written by this finalize
    _keep_mask(cap, S, L, [masks])
    ss = None if sampling else _feed(cap, S, L, [tokens_in], [ss_prob], emb)
    with _weights_scope(cap):
        _unroll(cap, S, L, plans, out.transpose(0, 1) if step_cls else None, ss, after)
        S.lazy = S.packed = None
        if not step_cls and counts is not None and sum(counts) < T * B:
            S.packed = _packed_classifier(cap, S, counts, lazy)
        elif not step_cls:
            rawl = _classify(cap, S, L)
            if lazy is not None:
                S.lazy = (rawl, V, B * V)                     # raw logits time-major: row (b,t) at b*V + t*B*V
            else:
                ops.logsoftmax_apply_steps(out, S.pm, S.ps, src_tbv=rawl)
            del rawl
        elif lazy is not None:
            S.lazy = (out, out.stride(0), out.stride(1))      # raw logits [B,T,V]: row (b,t) at b*T*V + t*V
        else:
            ops.logsoftmax_apply_steps(out, S.pm, S.ps)       # in place: [B,T,V] raw logits -> log-probs
    S.flt = None
    if sampling:
        S.sample = (seq, seq_masks, raw, alive)
        if flt is not None:
            S.flt = dict(saved, slp=slp, inv_tau=1.0 / flt['temperature'])
    cap._set_weights(S.aC, S.aS, S.bG, T)
    S.pi = None                             # (the tile statistics: only the lazy forms' backward reads them)
    if S.lazy is None:
        S.pm = S.ps = None
    if S.packed is not None:
        S.logp, S.lazy_ids, S.lazy_live = None, lazy.contiguous(), None
        return S.packed.pop('tlp'), S
    if S.lazy is not None:
        S.lazy_live = None
        if sampling:      # log p(drawn token) * live (captioner.py:336; zero after the reference's early break)
            S.lazy_ids = raw
            S.lazy_live = (alive[:T] > 0).to(torch.float32)
        else:
            S.lazy_ids = lazy.contiguous()
        tlp = cap._new(B, T)
        rl, ld_b, ld_t = S.lazy
        ops.gather_logp_raw(rl, ld_b, ld_t, B, T, V, S.pm, S.ps, B, S.lazy_ids, tlp, live=S.lazy_live)
        S.logp = None
        return tlp, S
    S.logp = out
    return out, S


def _packed_classifier(cap, S, counts, lazy):
    """Ragged: the classifier and everything behind it see the N = sum(counts) rows inside their captions only - h_lang
    gathered into packed time-major order (row n = (t, b), b < counts[t]), the statistics, raw logits, log p(target) and
    - in the backward - d logits, d h and the classifier's gradients over N rows (the row indices are built on the device
    from the T counts: a host-built index would travel through a freshly pinned buffer every iteration; N is known here,
    so nonzero needs no read-back)."""
    p, B, T, H, V = S.p, S.B, S.T, cap.settings['rnn_hid_dim'], cap.vocab_size
    N = int(sum(counts))
    cnt = ops.to_device(torch.tensor(counts, dtype=torch.int64), cap._dev)
    live = torch.arange(B, device=cap._dev).unsqueeze(0) < cnt.unsqueeze(1)              # [T,B]
    i_tb = torch.nonzero_static(live.reshape(-1), size=N).reshape(-1)                    # t*B + b, time-major
    idx = torch.stack([i_tb, (i_tb % B) * T + i_tb // B])
    # (N rounded up to whole tiles / k-blocks of the split-f16 kernels - the row count is the contraction length of
    # the classifier's dW; the pad rows are zero in h_lang and in d logits)
    Np = (N + 255) // 256 * 256
    hs = cap._zeros(Np, H)
    torch.index_select((S.hdrop if S.hdrop is not None else S.h2[1:]).reshape(T * B, H), 0, idx[0], out=hs[:N])
    n_tile = S.pm.shape[2]
    pm_p, ps_p = cap._new(Np, n_tile), cap._new(Np, n_tile)
    pi_p = cap._new(Np, n_tile, dtype=torch.int32)
    rawl = cap._new(Np, V)
    ops.vocab_fwd(hs, p['classifier.weight'], p['classifier.bias'], pm_p, ps_p, pi_p, rawl)
    ids_p = lazy.reshape(-1).index_select(0, idx[1]).contiguous()
    tlp_p = cap._new(N)
    ops.gather_logp_raw(rawl, V, 0, N, 1, V, pm_p, ps_p, N, ids_p, tlp_p)
    tlp = cap._zeros(B * T).index_copy_(0, idx[1], tlp_p).view(B, T)
    return dict(N=N, Np=Np, idx_tb=idx[0], idx_bt=idx[1], hs=hs, raw=rawl, pm=pm_p, ps=ps_p, tlp=tlp)


# ------------------------------------------------------------------------------ backward: stages of both forms
# (_backward below and autograd_pair._pair_backward: one reverse sweep each, the same stages around it)
# gradients that start from zero: the attention scores' biases (softmax is shift invariant) and the two embeddings
# (accumulated into, row by row)
_ZEROED = ('attention.cont_att.att_alpha.bias', 'attention.senti_att.word_alpha.bias', 'senti_label_embed.0.weight',
           'word_embed.0.weight')


def _dims(cap):
    st = cap.settings
    return st['feat_emb_dim'], st['att_hid_dim'], st['rnn_hid_dim'], st['word_emb_dim'], cap.vocab_size


def _nn(segs, out, acc=False):
    return ops.gemm_problem(segs, out, NN, accumulate=acc)


def _tn(segs, out, acc=False):
    return ops.gemm_problem(segs, out, TN, accumulate=acc)


class _Grads:
    """Where a backward pass puts its parameter gradients.  Without a sink they fill the {param name: gradient}
    dictionary the backward returns.  With one (`cap._grad_sink`, dp.GradSink: the data-parallel step) every gradient is
    written straight into its view of the flat arena (zeroed before the backward), and bucket_done(b) starts bucket b's
    all-reduce as soon as its last contraction is enqueued.  Bias gradients are column sums, deferred: every sum of a
    bucket goes out in one isc_colsum_multi.
    Gradient scale: the sweep is linear in what enters it, so everything entering is multiplied by a power of two S
    (isc_grad_scale: the largest entering |gradient| -> 2^-4..2^-3) and the parameter gradients by 1/S at the end - both
    exact - which keeps the f16 planes of the split-f16 contractions in their normal range."""

    def __init__(self, cap, p, sink=None):
        self.cap, self.p, self.sink = cap, p, sink
        self.G, self.sums, self.gs, self.zeroed = {}, [], None, {}

    def fill(self, specs, zeroed=_ZEROED):
        """Zero tensors for (shape, dtype) `specs` and for the gradients named in `zeroed` out of ONE fill (each fill is a
        launch of its own, ~4.5 us at any size); under a sink those gradients are the arena's."""
        names = list(zeroed) if self.sink is None else []
        out = self.cap._zeros_many(*specs, *[(self.p[n].shape, torch.float32) for n in names])
        self.zeroed = dict(zip(names, out[len(specs):]))
        return out[:len(specs)]

    def scale(self, gs_z, sources, feats, dense=()):
        """Picks S from `sources`, the attribute gradients `feats` and the dense log-prob gradients `dense` (their
        maxima: one extra pass each) into the zeroed float32[4] gs_z.  Returns (S as a [1] device tensor or None when
        scaling is off, `feats` times S)."""
        if not getattr(self.cap, 'grad_scaling', True):
            return None, feats
        srcs = list(sources) + [x.contiguous() if x is not None else None for x in feats]
        ops.grad_scale(srcs, gs_z, [d.abs().amax().reshape(1) for d in dense if d is not None])
        self.gs = gs_z
        return gs_z[0:1], [x * gs_z[0] if x is not None else None for x in feats]

    def gout(self, name, *shape):
        """The tensor parameter `name`'s gradient is computed into, viewed as `shape` (default: the parameter's); zero
        for the fill's `zeroed`."""
        if self.sink is not None:
            t = self.sink.out(name)
        else:                           # (parameter-shaped: autograd checks the shape of what the node returns)
            t = self.G[name] = self.zeroed.pop(name) if name in self.zeroed else self.cap._new(*self.p[name].shape)
        if not shape:
            return t
        assert t.numel() == math.prod(shape), (name, tuple(t.shape), shape)
        return t.view(*shape)

    def put(self, name, t):
        """Gradient `name` computed elsewhere: t itself, or under a sink a copy in the arena."""
        if self.sink is not None:
            self.sink.out(name).copy_(t)
        else:
            self.G[name] = t

    def tn(self, a, w, name):
        out = self.gout(name, a.shape[1], w.shape[1])
        ops.gemm_bwd([_tn([(a, w)], out)], TN)
        return out

    def csum(self, x, *names):
        """Column sum of x into the gradient(s) `names` (several: tied biases share one reduction), deferred."""
        self.sums.append((x, [self.gout(n, x.shape[1]) for n in names], False))

    def bucket_done(self, b):
        """Every gradient of bucket b (dp.GradSink.STARTS) is enqueued: its bias sums go out, then - under a sink - the
        bucket is unscaled in one launch and its all-reduce starts."""
        ops.colsum_multi(self.sums)
        del self.sums[:]
        if self.sink is not None:
            self.sink.ready(b, unscale=self.gs[1] if self.gs is not None else None)

    def finish(self):
        """The last bias sums, the gradients x 1/S (without a sink); returns the dictionary."""
        ops.colsum_multi(self.sums)
        del self.sums[:]
        if self.sink is None and self.gs is not None:
            torch._foreach_mul_(list(self.G.values()), self.gs[1])
        return self.G


def _step_bwd_plan(cap, p, Pc, Ps):
    """isc_step_bwd_plan of a reverse sweep: the weights, the split-K workspace and the prologue operands of the content
    attention (from Pc) and of the sentiment attention (from Ps); None: that attention is not in the plan's rows."""
    bp = _lib.StepBwdPlan()
    E, A, H, Wd, _ = _dims(cap)
    bp.H, bp.E, bp.A, bp.W = H, E, A, Wd
    for field, key in (('Wih1', 'att_lstm.weight_ih'), ('Whh1', 'att_lstm.weight_hh'),
                       ('Wih2', 'lang_lstm.weight_ih'), ('Whh2', 'lang_lstm.weight_hh'),
                       ('W_h2att', 'attention.cont_att.h2att.weight'),
                       ('w_alpha_c', 'attention.cont_att.att_alpha.weight'),
                       ('W_h2word', 'attention.senti_att.h2word.weight'),
                       ('w_alpha_s', 'attention.senti_att.word_alpha.weight'),
                       ('W_gh', 'attention.h2att.weight'), ('W_gc', 'attention.cont2att.weight'),
                       ('W_gs', 'attention.senti2att.weight'), ('w_gate', 'attention.att_alpha.weight')):
        setattr(bp, field, p[key].data_ptr())
    if Pc is not None:
        bp.R, bp.att_p, bp.att_e = Pc.R, Pc.att_p3.data_ptr(), Pc.att_e3.data_ptr()
        bp.row_div = Pc.row_div if Pc.row_div > 1 else 0       # rows = images x row_div: att_p / att_e one entry per image
    if Ps is not None:
        bp.Mw, bp.words_p, bp.words_e = Ps.Mw, Ps.words_p3.data_ptr(), Ps.words_e3.data_ptr()
        bp.label_w = ops.ptr(Ps.label_w)
    skws = ops.splitk_ws(cap._dev)
    bp.splitk_ws, bp.splitk_ws_floats = skws.data_ptr(), skws.numel()
    return bp


def _dlogits(lazy, d, logp, sparse, out, B, T, V, step_rows, scale, flt=None):
    """d logits of one call's B x T positions into `out`, time-major at step_rows rows per step: the softmax term from
    the log-probs logp, or - lazy = (raw, ld_b, ld_t, part_max, part_sum) - from the raw logits and their statistics.
    flt (lazy only): the filtered term - the gradient of the sampled distribution's log-probability - in the same pass."""
    if flt is not None:
        raw, ld_b, ld_t, pm, ps = lazy
        ops.logsoftmax_bwd_raw_filtered(raw, ld_b, ld_t, B, T, V, pm, ps, step_rows, list(sparse), flt, out, scale=scale,
                                        out_step_rows=step_rows)
    elif lazy is not None:
        raw, ld_b, ld_t, pm, ps = lazy
        ops.logsoftmax_bwd_raw(raw, ld_b, ld_t, B, T, V, pm, ps, step_rows, list(sparse), out, scale=scale,
                               out_step_rows=step_rows)
    else:
        ops.logsoftmax_bwd_sparse(d, logp, list(sparse), out, B * T, V, remap_T=T, scale=scale, out_step_rows=step_rows)


def _classifier_bwd(cap, g, dlogits, hs):
    """The classifier behind d logits [n, Vp] (zero-padded to Vp = _pad32(V) columns) and its input h_lang hs [n, H]:
    W_c's and the bias's gradients into g; returns d h [n, H]."""
    V, (n, H) = cap.vocab_size, hs.shape
    Vp = dlogits.shape[1]
    Wc = g.p['classifier.weight']
    dhd = cap._new(n, H)
    # d h = d logits . W_c contracts over the vocabulary; the split-f16 kernels want a multiple of 32
    Vm = V // 32 * 32
    if Vp != V and n >= 8192:
        # d logits is already zero-padded to Vp columns: give W_c the matching zero rows (a 20 MB copy; worth it from
        # ~100 GFLOP on, where the large kernels run the contraction)
        # NOT inside the weights scope: a scope keeps (pointer, planes) of every W operand it sees and the optimizer
        # re-splits them all after its step - from the pointer.  This copy dies with the call; its planes are built in
        # the workspace (one split launch).
        Wc_k = cap._zeros(Vp, H)
        Wc_k[:V].copy_(Wc)
        ops.gemm_bwd([_nn([(dlogits, Wc_k)], dhd)], NN)
    elif Vm != V and Vm >= 4096:
        # fewer rows (B = 128: [2560 x 512] over K = 10 000): the first Vm vocabulary rows on the K-split skinny tile,
        # the last V - Vm (< 32) on the fp32 tiles, accumulating
        with _weights_scope(cap):
            ops.gemm_bwd([_nn([(dlogits[:, :Vm], Wc[:Vm])], dhd)], NN)
        ops.gemm_bwd([_nn([(dlogits[:, Vm:], Wc[Vm:])], dhd, True)], NN)
    else:
        with _weights_scope(cap):
            ops.gemm_bwd([_nn([(dlogits, Wc)], dhd)], NN)
    if V % 4 == 0:
        g.tn(dlogits[:, :V], hs, 'classifier.weight')
    else:            # vocabulary not a multiple of 4: contract on the zero-padded columns, then trim
        dWp = cap._new(Vp, H)
        ops.gemm_bwd([_tn([(dlogits, hs)], dWp)], TN)
        g.put('classifier.weight', dWp[:V])
    ops.colsum(dlogits[:, :V], g.gout('classifier.bias'))
    return dhd


def _lstm_dw(g, dG1, dG2, h1_prev, h1_cur, h2_prev, xt, feat, dG1_sum, fc_e, label_e):
    """Both LSTM cells' weight and bias gradients, one contraction over all rows of the gate gradients dG1 (att-LSTM) /
    dG2 (lang-LSTM) each - either None: that cell is left for another call.  Problems grouped by their dY operand:
    isc_gemm_bwd splits a shared dY once and runs the group as one launch."""
    H = h2_prev.shape[1]
    if dG1 is not None:
        gW1 = g.gout('att_lstm.weight_ih')
        E = fc_e.shape[1]
        ops.gemm_bwd([_tn([(dG1, h2_prev)], gW1[:, 0:H]), _tn([(dG1, xt)], gW1[:, H + E:]),
                      _tn([(dG1, h1_prev)], g.gout('att_lstm.weight_hh'))], TN)
    if dG2 is not None:
        gW2 = g.gout('lang_lstm.weight_ih')
        E = feat.shape[1]
        ops.gemm_bwd([_tn([(dG2, feat)], gW2[:, 0:E]), _tn([(dG2, h1_cur)], gW2[:, E:]),
                      _tn([(dG2, h2_prev)], g.gout('lang_lstm.weight_hh'))], TN)
    if dG1 is not None:
        # xt = relu(Emb[tok]) + label_e: the per-step part contracted over the rows above, the label part (and fc_e) once
        # per caption here - dG1_sum = sum_t dG1[t]
        once = [_tn([(dG1_sum, fc_e)], gW1[:, H:H + E])]
        if label_e is not None:
            once.append(_tn([(dG1_sum, label_e)], gW1[:, H + E:], True))
        ops.gemm_bwd(once, TN)
        g.csum(dG1, 'att_lstm.bias_ih', 'att_lstm.bias_hh')
    if dG2 is not None:
        g.csum(dG2, 'lang_lstm.bias_ih', 'lang_lstm.bias_hh')


def _dx_bwd(cap, g, dG1, dG1_sum, tok, with_label):
    """Inputs of the att-LSTM: d fc_e and d label_e (rows of dG1_sum), d xt over the rows of dG1 - and through
    xt = relu(Emb[tok]) into the word embedding's gradient (its first accumulation).  Returns (d_fc_e, d_label_e, dEmb)."""
    p, new = g.p, cap._new
    E, _, H, Wd, _ = _dims(cap)
    Wih1 = p['att_lstm.weight_ih']
    d_fc_e = new(dG1_sum.shape[0], E)
    d_label_e = new(dG1_sum.shape[0], Wd) if with_label else None
    dxt = new(dG1.shape[0], Wd)
    probs = [_nn([(dG1_sum, Wih1[:, H:H + E])], d_fc_e), _nn([(dG1, Wih1[:, H + E:])], dxt)]
    if d_label_e is not None:
        probs.append(_nn([(dG1_sum, Wih1[:, H + E:])], d_label_e))
    with _weights_scope(cap):      # dX over all rows: split-f16 on planes of the W_ih slices' transposes
        ops.gemm_bwd(probs, NN)
    dEmb = g.gout('word_embed.0.weight')
    # nn.Embedding(padding_idx=pad_id): the <PAD> row never gets a gradient - every accumulation into dEmb skips it
    ops.embed_relu_bwd(p['word_embed.0.weight'], tok, dxt, dEmb, dG1.shape[0], skip_id=cap.pad_id)
    return d_fc_e, d_label_e, dEmb


def _content_att_grads(g, dqa, h1_cur, dwc_rows):
    """Content attention's own parameters from the sweep's dqa [T, n, A] (h2att over all rows) and alpha partials."""
    dqaf = dqa.view(-1, dqa.shape[2])
    g.tn(dqaf, h1_cur, 'attention.cont_att.h2att.weight')
    g.csum(dqaf, 'attention.cont_att.h2att.bias')
    g.csum(dwc_rows, 'attention.cont_att.att_alpha.weight')
    g.gout('attention.cont_att.att_alpha.bias')          # softmax is shift invariant


def _senti_att_grads(cap, g, dqw, h1_cur, dws_rows, label_e, lo=0, d_label_e=None, group=1):
    """Sentiment attention's own parameters from the sweep's dqw [T, n, A] (the branch's rows: [lo, n) - the others are
    zero) and alpha partials.  label2word(label_e) enters every step's score: d label_w = sum_t dqw[t], returned (None
    without labels) and, given d_label_e, accumulated into it.  group > 1: label_e / label_w hold one entry per image -
    d label_w is summed over the image's rows, in row order."""
    T, n, A = dqw.shape
    dqwf = dqw.view(T * n, A)
    g.tn(dqwf, h1_cur, 'attention.senti_att.h2word.weight')
    g.csum(dqwf, 'attention.senti_att.h2word.bias')
    g.csum(dws_rows, 'attention.senti_att.word_alpha.weight')
    g.gout('attention.senti_att.word_alpha.bias')
    if label_e is None:
        return None
    d_label_w = cap._new(n * A)
    ops.colsum(dqw.view(T, n * A), d_label_w)
    d_label_w = d_label_w.view(n, A)[lo:]
    if group > 1:
        d_label_w = _group_sum(d_label_w, group)
    g.tn(d_label_w, label_e, 'attention.senti_att.label2word.weight')
    g.csum(d_label_w, 'attention.senti_att.label2word.bias')
    if d_label_e is not None:
        ops.gemm_bwd([_nn([(d_label_w, g.p['attention.senti_att.label2word.weight'])], d_label_e, True)], NN)
    return d_label_w


def _scan_bwd(cap, p3, e3, alpha, q, dfeat, de, w, step_rows=0, q2=None, group=1):
    """An attention's dV = sum_t alpha_t x d feat_t and dP from every step's d e, formed once after the sweep (dfeat:
    [T, B, D], or the rows of a [T, step_rows, D] stack).  Returns (dP, dV), shaped as the projections p3 / e3 - with
    group = n > 1 those hold one entry per image and the sums run over the image's n rows as well."""
    dP, dV = cap._new(*p3.shape), cap._new(*e3.shape)
    ops.attn_dv_from_alpha(alpha, dfeat, dV, step_rows=step_rows, group=group)
    ops.attn_dp_from_de(p3, q, w, de, dP, q2=q2, group=group)
    return dP, dV


def _region_embed_bwd(cap, g, P, dP, dV):
    """att2att -> att_embed of the regions."""
    B, R, A = P.att_p3.shape
    E, BR = P.att_e3.shape[2], B * R
    att_e, att_p = P.att_e3.view(BR, E), P.att_p3.view(BR, A)
    dzp = cap._new(BR, A)
    ops.relu_mask_bwd(dP.view(BR, A), att_p, dzp)
    g.tn(dzp, att_e, 'att2att.0.weight')
    g.csum(dzp, 'att2att.0.bias')
    dVa = dV.view(BR, E)
    ops.gemm_bwd([_nn([(dzp, g.p['att2att.0.weight'])], dVa, True)], NN)
    dze = cap._new(BR, E)
    ops.relu_mask_bwd(dVa, att_e, dze, keep_mask=P.m_att, scale=P.sc)
    g.tn(dze, P.x_att, 'att_embed.0.weight')
    g.csum(dze, 'att_embed.0.bias')


def _senti2att_bwd(cap, g, P, dP):
    """senti2att of the sentiment words; returns d of its pre-activation [B*Mw, A] (for _senti_words_bwd)."""
    B, Mw, A = P.words_p3.shape
    dzw = cap._new(B * Mw, A)
    ops.relu_mask_bwd(dP.view(B * Mw, A), P.words_p3.view(B * Mw, A), dzw)
    g.tn(dzw, P.words_e3.view(B * Mw, -1), 'senti2att.0.weight')
    g.csum(dzw, 'senti2att.0.bias')
    return dzw


def _senti_words_bwd(cap, g, P, dzw, dV, dEmb):
    """The sentiment words' embedding rows: dV plus senti2att's input gradient, accumulated into dEmb."""
    B, Mw, Wd = dV.shape
    dVw = dV.view(B * Mw, Wd)
    ops.gemm_bwd([_nn([(dzw, g.p['senti2att.0.weight'])], dVw, True)], NN)
    ops.embed_relu_bwd(g.p['word_embed.0.weight'], P.sw_ids, dVw, dEmb, B * Mw, pad_first=Mw, pad_id=cap.pad_id,
                       keep_mask=P.m_words, mask_scale=P.sc, skip_id=cap.pad_id)


# P.fc_pre / P.cpt_pre: the tensors the `fc_feats` / `cpt_feats` attributes expose (pre-dropout; equal to the post-dropout
# ones in sign wherever the keep-mask is 1, and their gradients ignore the mask).  fc_pre is None in seq2seq, where
# fc_e := dropout(cpt_feats) (captioner.py:250-251).
def _fc_embed_bwd(cap, g, P, d_fc_e, d_fc_feats):
    """fc_embed (xe / rl): from d fc_e and the fc_feats attribute's gradient."""
    dzf = cap._new(*d_fc_e.shape)
    ops.relu_mask_bwd(d_fc_e, P.fc_e, dzf, keep_mask=P.m_fc, scale=P.sc)
    if d_fc_feats is not None:
        extra = cap._new(*d_fc_e.shape)
        ops.relu_mask_bwd(d_fc_feats.contiguous(), P.fc_pre, extra)
        dzf = dzf + extra
    g.tn(dzf, P.x_fc, 'fc_embed.0.weight')
    g.csum(dzf, 'fc_embed.0.bias')


def _cpt_bwd(cap, P, d_fc_e, d_cpt_feats, out):
    """d cpt (cpt2fc's output) of one call's rows into `out`: the cpt_feats attribute's gradient, and in seq2seq the
    path through fc_e."""
    if P.fc_pre is not None:
        ops.relu_mask_bwd(d_cpt_feats.contiguous(), P.cpt, out)
        return
    ops.relu_mask_bwd(d_fc_e, P.cpt, out, keep_mask=P.m_cpt, scale=P.sc)
    if d_cpt_feats is not None:
        extra = cap._new(*out.shape)
        ops.relu_mask_bwd(d_cpt_feats.contiguous(), P.cpt_pre, extra)
        out += extra


def _cpt2fc_bwd(cap, g, d_cpt, Ps, dEmb):
    """cpt2fc and the concept words' mean embedding (accumulated into dEmb) over the rows of d_cpt: the rows of the
    prologues Ps, in order."""
    def rows(xs):
        return xs[0] if len(xs) == 1 else torch.cat(xs)
    p = g.p
    g.tn(d_cpt, rows([P.cmean for P in Ps]), 'cpt2fc.0.weight')
    g.csum(d_cpt, 'cpt2fc.0.bias')
    dcm = cap._new(d_cpt.shape[0], p['cpt2fc.0.weight'].shape[1])
    ops.gemm_bwd([_nn([(d_cpt, p['cpt2fc.0.weight'])], dcm)], NN)
    C = Ps[0].cpt_ids.shape[1]
    if any(P.cpt_ids.shape[1] != C for P in Ps):
        raise ValueError('merged unrolls: the two calls carry different numbers of concept words')
    ops.embed_relu_bwd(p['word_embed.0.weight'], rows([P.cpt_ids for P in Ps]).view(-1), dcm, dEmb, d_cpt.shape[0] * C,
                       rows_per_grad=C, scale=1.0 / C, skip_id=cap.pad_id)


def _sweep_buffers(cap, g, S, L, zero_rec, sum_rows, packed_rows=0):
    """The reverse sweep's buffers; from g's ONE fill: gs_z, dG1_sum [sum_rows, 4H], what the sweep accumulates into when
    zero_rec, every gradient stack when L.short - but packed dG1 / dG2 [packed_rows, 4H] (_sweep zeroes their pad)."""
    E, A, H, _, _ = _dims(cap)
    T, Bt = L.T, L.Bt
    rec, big = {'rec': (7, Bt, H)}, {'d_feat': (T, Bt, E)}
    for q, de, dw, x in (('dqa', 'de_c', 'dwc_rows', S.aC), ('dqw', 'de_s', 'dws_rows', S.aS)):
        if x is not None:
            rec.update({q: (T, Bt, A), dw: (x.shape[0], A)})
            big[de] = (x.shape[1], x.shape[0], x.shape[2])
    if S.z is not None:
        rec.update(dwg_rows=(Bt, A), dbg_rows=(Bt, 1))
        big.update(dv=(T, Bt, E), ds=(T, Bt, E), dz=(T, Bt, A))
    dG = (packed_rows or T * Bt, 4 * H)
    zeroed = dict(gs_z=(4,), dG1_sum=(sum_rows, 4 * H), **(rec if zero_rec else {}), **(big if L.short else {}))
    if L.short and not packed_rows:
        zeroed.update(dG1=dG, dG2=dG)
    D = _Saved()
    D.__dict__.update(zip(zeroed, g.fill([(sh, torch.float32) for sh in zeroed.values()])))
    D.__dict__.update({k: cap._new(*sh) for k, sh in dict(rec, **big, dG1=dG, dG2=dG).items() if k not in zeroed})
    return D


def _sweep(cap, S, L, plans, D, dhd, first, packed=False):
    """The reverse step loop of both forms, t = T-1 down; `first`: no incoming recurrent gradients at T-1 (else the
    filled buffers are accumulated into).  packed: step t's dG1 / dG2 rows follow the earlier steps' rows directly.
    Returns h1_prev, h1_cur, h2_prev, xt, feat as [T*Bt, .] rows."""
    T, Bt, rec = L.T, L.Bt, D.rec
    dG_rows = list(itertools.accumulate((r1 - r0 for r0, r1, _ in L.steps), initial=0)) if packed else None

    def rows(x):                          # [Bt, .] buffers: the step's rows, whichever the step
        return _at(x.unsqueeze(0).expand(T, *x.shape))

    def alt(i, step):                     # cell-state gradients: two buffers, swapped every step
        return [rec[i + ((t + step) & 1)].data_ptr() for t in range(T)], rec.stride(1) * 4
    common = dict(g1=_at(S.g1), c1_prev=_at(S.c1), c1=_at(S.c1[1:]), g2=_at(S.g2), c2_prev=_at(S.c2), c2=_at(S.c2[1:]),
                  dhd=_at(dhd), d_feat=_at(D.d_feat), dG1_sum=rows(D.dG1_sum[:Bt]), dh1=rows(rec[6]),
                  dh2_rec=rows(rec[0]), dh1_rec=rows(rec[1]), dc1_in=alt(2, 1), dc1_out=alt(2, 0), dc2_in=alt(4, 1),
                  dc2_out=alt(4, 0))
    for name in ('dG1', 'dG2'):
        x = getattr(D, name)
        if dG_rows is None:
            common[name] = _at(x.view(T, Bt, -1))
        else:                             # (packed: the pad rows behind the last step's block are zero)
            x[dG_rows[-1]:].zero_()
            common[name] = [x[o].data_ptr() for o in dG_rows[:T]], 0
    blocks = [{} for _ in L.blocks]
    if S.aC is not None:
        k, lo = S.att['c']
        blocks[k].update(qa=_at(S.qa, 0), v=_at(S.feat if S.v is None else S.v, lo), alpha_c=_at(S.aC.transpose(0, 1), 0),
                         dqa=_at(D.dqa, lo), de_c=_at(D.de_c, 0))
    if S.aS is not None:
        k, lo = S.att['s']
        blocks[k].update(qw=_at(S.qw, 0), s=_at(S.feat if S.s is None else S.s, lo), alpha_s=_at(S.aS.transpose(0, 1), 0),
                         dqw=_at(D.dqw, lo), de_s=_at(D.de_s, 0))
    if S.z is not None:
        blocks[0].update(dv=_at(D.dv), ds=_at(D.ds), z=_at(S.z), beta=_at(S.bG.t()), dz=_at(D.dz))
    for bp in plans.values():
        _lds(bp, S)
        for name in ('dwc_rows', 'dws_rows', 'dwg_rows', 'dbg_rows'):
            setattr(bp, name, ops.ptr(getattr(D, name, None)))

    def launch(t, bp):
        bp.first, bp.last = int(first and t == T - 1), int(t == 0)
        ops.step_bwd(bp)
    # the weights do not change during the sweep: few-row launches take the one-launch skinny split-f16 kernel on
    # planes of W^T built once here (isc_gemm_bwd, NN layout), instead of fp32 split-K slabs + a reduce kernel per GEMM
    with _weights_scope(cap):
        _steps(L, plans, common, blocks, range(T - 1, -1, -1), launch)
    return [x.reshape(T * Bt, -1) for x in (S.h1[:T], S.h1[1:], S.h2[:T], S.xt, S.feat)]


def _dropout_bwd(S, dhd):
    """nn.Dropout on h_lang (captioner.py:182): d h_lang [T*Bt, H] through the keep-mask, in place."""
    if S.keep is not None:
        ops.relu_mask_bwd(dhd, None, dhd, keep_mask=S.keep.view(dhd.shape), scale=S.out_scale)


def _group_sum(x, n):
    """[I*n, C] per-row gradients -> [I, C] per image: row j = 0 .. n-1 of an image added in that order, whatever n (a
    chain of n - 1 elementwise additions on [I, C]: a few KB, not a hot path, and the order is the documented one)."""
    x3 = x.view(-1, n, x.shape[1])
    out = x3[:, 0].clone()
    for j in range(1, n):
        out += x3[:, j]
    return out


# ------------------------------------------------------------------------------ backward
def _backward(cap, S, dlogp, d_fc_feats, d_cpt_feats, sparse=(), flt=None):
    """Returns {param name: gradient}.  The gradient of the log-probs arrives as `dlogp` [B,T,V] (contiguous; None when
    every consumer handed its part over sparse) plus `sparse` = [(ids [B,T] int64, coef [B,T] fp32)]: coef at column ids
    of each row (XELossFn / GatherLogpFn below).  Optional gradients of the `fc_feats` (pre-dropout) and `cpt_feats`
    attributes.  flt: the filtered term of a sampled roll-out under sampling controls (DecodeFn.backward) - (tok, coef) of
    the SAMPLING log-probabilities and what the forward saved for them; it enters d logits in the same launch.
    Gradient scale and outputs: _Grads."""
    p, P, B, T, L = S.p, S.P, S.B, S.T, S.L
    E, A, H, _, V = _dims(cap)
    new, zeros = cap._new, cap._zeros
    has_c, has_s = P.att_e3 is not None, P.words_e3 is not None
    gate = has_c and has_s
    TB = T * B
    g = _Grads(cap, p)

    # ---- classifier + log-softmax: outside the recurrence, all T*B rows at once (time-major rows)
    Vp = _pad32(V)
    pk = getattr(S, 'packed', None)
    dlogits = new(TB if pk is None else pk['Np'], Vp)
    # ragged unroll (see _train_forward): step t sweeps rows [0, counts[t]); everything a skipped row would have written
    # - its gradients, and the carries a row reads at the LAST step of its caption - is zero from the fill, and the sweep
    # has no "first" step (a row's own last step is wherever its caption ends).  Packed: step t's gate gradients at rows
    # [offs[t], offs[t] + counts[t]) - the contractions over all rows behind the sweep (both LSTM cells' dW groups, dxt,
    # the bias sums) see N rows, no gather
    D = _sweep_buffers(cap, g, S, L, L.short, B, 0 if pk is None else pk['Np'])
    scale, (d_fc_feats, d_cpt_feats) = g.scale(D.gs_z, [c for _, c in sparse] + ([flt['coef']] if flt else []),
                                               (d_fc_feats, d_cpt_feats), [dlogp])
    if pk is not None:
        # ragged, packed classifier block (see _train_forward): d logits over the N rows inside their captions
        N = pk['N']
        sp = [(i.reshape(-1).index_select(0, pk['idx_bt']).contiguous(), c.reshape(-1).index_select(0, pk['idx_bt']).contiguous())
              for i, c in sparse]
        if sp:
            _dlogits((pk['raw'], V, 0, pk['pm'], pk['ps']), None, None, sp, dlogits, N, 1, V, N, scale)
            if pk['Np'] > N:
                dlogits[N:].zero_()
        else:
            dlogits.zero_()
    elif dlogp is None and not sparse and flt is None:
        dlogits.zero_()
    else:                       # (lazy: the log-probs were never formed - softmax from raw logits + stats)
        lazy = getattr(S, 'lazy', None)
        _dlogits(lazy and (*lazy, S.pm, S.ps), dlogp, S.logp, sparse, dlogits, B, T, V, B, scale, flt)
    hdrop_tb = (S.hdrop if S.hdrop is not None else S.h2[1:]).reshape(TB, H) if pk is None else pk['hs']
    dhd = _classifier_bwd(cap, g, dlogits, hdrop_tb)
    if pk is not None:          # d h_lang back in [T,B] order, zero behind the captions' ends
        dhd = zeros(TB, H).index_copy_(0, pk['idx_tb'], dhd[:pk['N']])
    _dropout_bwd(S, dhd)
    h1_prev, h1_cur, h2_prev, xt_tb, feat_tb = _sweep(
        cap, S, L, {(True,): _step_bwd_plan(cap, p, P if has_c else None, P if has_s else None)}, D, dhd.view(T, B, H),
        not L.short, pk is not None)
    dG1_sum = D.dG1_sum
    # captions per image, everything per image (the sampled roll-out): an image's rows of sum_t dG1 added in row order -
    # what follows (the once-per-caption dW partners fc_e / label_e, d fc_e, d label_e) is then per image as it stands
    per_image = P.row_div > 1 and not P.pre_rows
    if per_image:
        dG1_sum = _group_sum(dG1_sum, P.row_div)
    if has_c:
        dP_att, dV_att = _scan_bwd(cap, P.att_p3, P.att_e3, S.aC, S.qa, D.dv if gate else D.d_feat, D.de_c,
                                   p['attention.cont_att.att_alpha.weight'], group=P.row_div)
    if has_s:
        # (P.row_div > 1 with sentiment words: the sampled roll-out - words_p / words_e / label_w per image)
        dP_w, dV_w = _scan_bwd(cap, P.words_p3, P.words_e3, S.aS, S.qw, D.ds if gate else D.d_feat, D.de_s,
                               p['attention.senti_att.word_alpha.weight'], q2=P.label_w, group=P.row_div)

    # ---- weight gradients: one contraction over all T*B rows each
    tok_tb = S.tok.view(-1)
    h1_cur_l = h1_cur               # (the LSTM groups' copy: the attention contractions below stay on [T,B] rows)
    dG1f, dG2f = D.dG1, D.dG2       # ([T*B or the packed rows, 4H])
    if pk is not None:
        # packed gate gradients: their partners gathered to the same rows (pad rows zero / <PAD>)
        def pack(x):
            out = new(pk['Np'], x.shape[1], dtype=x.dtype)
            torch.index_select(x, 0, pk['idx_tb'], out=out[:pk['N']])
            if pk['Np'] > pk['N']:
                out[pk['N']:].zero_()
            return out
        h1_prev, h1_cur_l, h2_prev, feat_tb, xt_tb = pack(h1_prev), pack(h1_cur), pack(h2_prev), pack(feat_tb), pack(xt_tb)
        tok_tb = pack(tok_tb.view(TB, 1)).view(-1)
        if pk['Np'] > pk['N']:
            tok_tb[pk['N']:].fill_(cap.pad_id)
    # (captions per image: dG1_sum is per row - its partner is fc_e with each image's row repeated, and d fc_e [I*n, E]
    # sums over an image's n rows, in row order, into the per-image [I, E])
    _lstm_dw(g, dG1f, dG2f, h1_prev, h1_cur_l, h2_prev, xt_tb, feat_tb, dG1_sum, P.fc_e if P.fc_rows is None else P.fc_rows,
             P.label_e)
    d_fc_e, d_label_e, dEmb = _dx_bwd(cap, g, dG1f, dG1_sum, tok_tb, P.label_e is not None)
    if P.row_div > 1 and not per_image:
        d_fc_e = _group_sum(d_fc_e, P.row_div)
    if has_c:
        _content_att_grads(g, D.dqa, h1_cur, D.dwc_rows)
    if has_s:
        _senti_att_grads(cap, g, D.dqw, h1_cur, D.dws_rows, P.label_e, d_label_e=d_label_e,
                         group=P.row_div if per_image else 1)
    if gate:
        dzf = D.dz.view(TB, A)
        g.tn(dzf, S.v.view(TB, E), 'attention.cont2att.weight')
        g.tn(dzf, S.s.view(TB, E), 'attention.senti2att.weight')
        g.tn(dzf, h1_cur, 'attention.h2att.weight')
        g.csum(dzf, 'attention.cont2att.bias', 'attention.senti2att.bias', 'attention.h2att.bias')
        g.csum(D.dwg_rows, 'attention.att_alpha.weight')
        g.csum(D.dbg_rows, 'attention.att_alpha.bias')

    # ---- prologue backward
    if d_label_e is not None:
        ops.embed_relu_bwd(p['senti_label_embed.0.weight'], P.label_ids, d_label_e, g.gout('senti_label_embed.0.weight'),
                           d_label_e.shape[0], keep_mask=P.m_label, mask_scale=P.sc)
    if has_c:
        _region_embed_bwd(cap, g, P, dP_att, dV_att)
    if has_s:
        _senti_words_bwd(cap, g, P, _senti2att_bwd(cap, g, P, dP_w), dV_w, dEmb)
    if P.fc_pre is not None:
        _fc_embed_bwd(cap, g, P, d_fc_e, d_fc_feats)
    if P.fc_pre is None or d_cpt_feats is not None:
        d_cpt = new(P.B, E)
        _cpt_bwd(cap, P, d_fc_e, d_cpt_feats, d_cpt)
        _cpt2fc_bwd(cap, g, d_cpt, (P,), dEmb)
    return g.finish()


class DecodeFn(torch.autograd.Function):
    """(mode, inputs, *params) -> (logp, cpt_feats[, fc_feats])."""

    @staticmethod
    def forward(ctx, cap, mode, fc, att, cpt_words, senti_words, tokens_in, senti_labels, ss_prob, masks,
                names, lazy, *params):
        group = 1
        if isinstance(mode, tuple):                  # ('xe' | 'rl', n): forward_xe / forward_rl with captions_per_image = n
            mode, group = mode
        with torch.no_grad():
            logp, S = _train_forward(cap, mode, fc, att, cpt_words, senti_words, tokens_in, senti_labels,
                                     ss_prob, masks, lazy, group)
        S.P.fc_pre = cap.fc_feats if mode != 'seq2seq' else None
        S.P.cpt_pre = cap.cpt_feats
        cap._last_sample = getattr(S, 'sample', None)
        ctx.cap, ctx.S, ctx.names = cap, S, names
        # side channel for the criteria: XELossFn / GatherLogpFn find this node as `logp.grad_fn` and append their
        # (ids, coef) pairs here in THEIR backward (which precedes this node's) instead of returning a [B,T,V] tensor
        ctx._isc_sparse = []
        ctx.set_materialize_grads(False)
        outs = [logp, cap.cpt_feats]
        if mode != 'seq2seq':
            outs.append(cap.fc_feats)
        if S.flt is not None:               # the sampling log-probs [B,T]: a differentiable output of their own
            outs.append(S.flt.pop('slp'))
        # the attribute tensors alias internal buffers: hand autograd distinct objects
        return tuple(o if i == 0 else o.clone() for i, o in enumerate(outs))

    @staticmethod
    def backward(ctx, dlogp, d_cpt, d_fc=None, d_slp=None):
        cap, S = ctx.cap, ctx.S
        sparse, ctx._isc_sparse = ctx._isc_sparse, []
        with torch.no_grad():
            flt = None
            if d_slp is not None:
                # d log q(drawn token) [B,T], one coefficient per row like the model's below - times `live`: behind the
                # early break the output is the constant zero.  No [B,T,V] tensor: the decode node's d logits kernel
                # rebuilds the kept set from what the forward saved (isc_logsoftmax_bwd_raw_filtered)
                flt = dict(S.flt, tok=S.lazy_ids, coef=(d_slp * S.lazy_live).contiguous())
            if getattr(S, 'lazy', None) is not None or getattr(S, 'packed', None) is not None:
                # dlogp is d log p(id) [B,T]: one column per row
                if dlogp is not None:
                    coef = dlogp.contiguous() if S.lazy_live is None else (dlogp * S.lazy_live).contiguous()
                    sparse, dlogp = [(S.lazy_ids, coef)], None
            G = _backward(cap, S, dlogp.contiguous() if dlogp is not None else None, d_fc, d_cpt, sparse, flt)
        grads = tuple(G.get(n) for n in ctx.names)
        ctx.S = None
        return (None,) * 12 + grads


def xe_with_grad(cap, mode, fc, att, cpt_words, senti_words, captions, senti_labels, ss_prob, masks, targets=None,
                 group=1):
    # a backward will run: float16 features become fp32 once, here - forward and backward read that copy (the dW
    # contractions and the exact engine read fp32), so losses and gradients are those of feats.float()
    fc, att = (None if x is None else cap._f32(x) for x in (fc, att))
    names = [n for n, q in cap.named_parameters() if q.requires_grad]
    params = [q for _, q in cap.named_parameters() if q.requires_grad]
    ids = cap._ids(captions)
    tokens_in = ids[:, :-1].contiguous()
    # inside `with captioner.token_logprobs():` (the package's own training steps) the call returns log p(target) [B,T]
    # instead of the [B,T,V] log-probs - XECriterion takes either (captioner.py:427-440 reads one column per row)
    lazy = None
    if cap.__dict__.get('_token_logprobs'):
        lazy = ids[:, 1:].contiguous() if targets is None else cap._ids(targets).contiguous()
    outs = DecodeFn.apply(cap, mode if group == 1 else (mode, group), fc, att, cpt_words, senti_words, tokens_in,
                          senti_labels, ss_prob, masks, names, lazy, *params)
    logp = outs[0]
    cap.cpt_feats = outs[1]
    if mode != 'seq2seq':
        cap.fc_feats = outs[2]
    return logp


def rollout_with_grad(cap, fc, att, cpt_words, senti_words, senti_labels, T, replay, masks, cons=None, group=1,
                      filt=None):
    """Sampled roll-out with REINFORCE gradients (captioner.py:290-349, sample_max=0, train mode): one unroll
    that samples each next token on the device and keeps the activations for the backward pass; the returned
    log-probs are log p(drawn token), zero after the reference's early `break`.
    cons: forward_rl's token constraints (an isc_decode_constraints struct) - they decide which token is drawn; the
    log-probability, and so the gradient, stays the model's own of that token.
    group = n > 1 (forward_rl captions_per_image): the inputs hold one entry per image, the draws (`replay`, the
    uniforms) and the returned tensors n rows per image, row i*n + j = draw j of image i.
    filt: forward_rl's sampling controls (Captioner._sample_filter).  When they change the sampled distribution
    (temperature / top_k / top_p on, or constraints with the sampling log-probs wanted) the draws come from the filtered
    finalize, which keeps what the backward needs, and the sampling log-probabilities log q(drawn token) are a second
    differentiable output - the on-policy REINFORCE gradient of a filtered roll-out is that of log q, not of the
    model's log p.  With `want_slp` they are returned as the fourth tensor (default controls: the model's own)."""
    fc, att = cap._f32(fc), cap._f32(att)          # (as xe_with_grad: fp32 once, in front of the prologue)
    names = [n for n, q in cap.named_parameters() if q.requires_grad]
    params = [q for _, q in cap.named_parameters() if q.requires_grad]
    B = fc.shape[0] * group
    draws = {'T': T, 'cons': cons}
    if replay is not None:
        draws['forced'] = cap._ids(replay)
        if group > 1 and tuple(draws['forced'].shape) != (B, T):
            raise ValueError('_replay must hold the draws of every row, [%d, %d], got %r'
                             % (B, T, tuple(draws['forced'].shape)))
    elif filt is not None and filt['uniforms'] is not None:
        u = filt['uniforms']
        if not torch.is_tensor(u) or u.dtype != torch.float32 or tuple(u.shape) != (B, T):
            raise ValueError('_uniforms must be a float32 tensor of shape [B, T] = [%d, %d]' % (B, T))
        draws['u'] = u.to(cap._dev).contiguous()
    elif filt is not None and filt['generator'] is not None:
        draws['u'] = torch.rand(B, T, device=cap._dev, generator=filt['generator'])
    else:
        draws['u'] = torch.rand(B, T, device=cap._dev)
    want_slp = filt is not None and filt['want_slp']
    if filt is not None and (filt['filtered'] or (cons is not None and want_slp)):
        draws['flt'] = filt
    was = cap.training
    # the roll-out's [B,T,V] log-probs are never an API output (captioner.py:336 keeps log p(drawn token) only): the
    # decode node returns that column - already times `live` - from the raw logits (lazy = True; DecodeFn.backward)
    outs = DecodeFn.apply(cap, 'rl' if group == 1 else ('rl', group), fc, att, cpt_words, senti_words, draws,
                          senti_labels, 0.0, masks, names, True, *params)
    cap.train(was)
    lp = outs[0]
    cap.cpt_feats, cap.fc_feats = outs[1], outs[2]
    seq, seq_masks, raw, alive = cap._last_sample
    cap._last_sample = None
    if want_slp:       # (default controls: the sampled distribution IS the model's)
        return seq, lp, seq_masks, outs[3] if 'flt' in draws else lp.clone()
    return seq, lp, seq_masks


def _decode_node(logp):
    """The sparse side channel behind `logp` - (decode node, slot) - if the criterion may use it: `logp` must be that
    node's own output (a slice or a copy of it has another grad_fn), else None (dense hand-over).  A DecodeFn node has one
    log-prob output (slot None: `_isc_sparse` is a list); the merged node of two sibling unrolls (autograd_pair) has two,
    keyed by output number."""
    node = logp.grad_fn
    ch = getattr(node, '_isc_sparse', None) if node is not None else None
    if ch is None:
        return None
    if isinstance(ch, dict):
        return (node, logp.output_nr) if logp.output_nr in ch else None
    return (node, None)


def _sparse_append(chan, pair):
    node, slot = chan
    (node._isc_sparse if slot is None else node._isc_sparse[slot]).append(pair)


class GatherLogpFn(torch.autograd.Function):
    """log p(drawn token) * live (captioner.py:336, zero after the early break).  Backward: the gradient w.r.t. the
    [B,T,V] log-probs is g[b,t] * live[t] at column raw[b,t] - handed to the decode node as an (ids, coef) pair."""

    @staticmethod
    def forward(ctx, logp, raw, live, node):
        ctx.node, ctx.shape = node, logp.shape
        ctx.save_for_backward(raw, live)
        return logp.gather(2, raw.unsqueeze(2)).squeeze(2) * live

    @staticmethod
    def backward(ctx, g):
        raw, live = ctx.saved_tensors
        coef = (g * live).contiguous()
        if ctx.node is not None:
            _sparse_append(ctx.node, (raw.contiguous(), coef))
            return None, None, None, None
        d = torch.zeros(ctx.shape, dtype=coef.dtype, device=coef.device)
        d.scatter_(2, raw.unsqueeze(2), coef.unsqueeze(2))
        return d, None, None, None


class XELossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, lengths_i32, node):
        out2 = torch.empty(2, dtype=torch.float32, device=pred.device)
        ops.xe_loss_fwd(pred, target, lengths_i32, out2)
        ctx.save_for_backward(target, lengths_i32, out2)
        ctx.shape, ctx.node = pred.shape, node
        return out2[0] / out2[1]

    @staticmethod
    def backward(ctx, g):
        target, lengths_i32, out2 = ctx.saved_tensors
        gout = g.reshape(1).contiguous().float()
        if ctx.node is not None:        # pred is a decode node's own output: hand (target, coef) over, no [B,T,V] tensor
            coef = torch.empty(ctx.shape[:2], dtype=torch.float32, device=target.device)
            ops.xe_loss_bwd_sparse(lengths_i32, ctx.shape[1], gout, out2, coef)
            _sparse_append(ctx.node, (target, coef))
            return None, None, None, None
        dlogp = torch.zeros(ctx.shape, dtype=torch.float32, device=target.device)
        ops.xe_loss_bwd(target, lengths_i32, gout, out2, dlogp)
        return dlogp, None, None, None


class XETokenLossFn(torch.autograd.Function):
    """XECriterion (captioner.py:427-440) on per-token log-probs tlp [B,T] = log p(target) (Captioner.token_logprobs):
    the same masked mean, the same summation order as on the [B,T,V] tensor."""

    @staticmethod
    def forward(ctx, tlp, lengths_i32):
        out2 = torch.empty(2, dtype=torch.float32, device=tlp.device)
        ops.xe_loss_tokens_fwd(tlp, lengths_i32, out2)
        ctx.save_for_backward(lengths_i32, out2)
        ctx.shape = tlp.shape
        return out2[0] / out2[1]

    @staticmethod
    def backward(ctx, g):
        lengths_i32, out2 = ctx.saved_tensors
        coef = torch.empty(ctx.shape, dtype=torch.float32, device=out2.device)
        ops.xe_loss_bwd_sparse(lengths_i32, ctx.shape[1], g.reshape(1).contiguous().float(), out2, coef)
        return coef, None


def xe_criterion_with_grad(pred, target, lengths):
    ops.require_device(pred, target)
    ln = ops.upload(lengths, torch.int32, pred.device)
    if pred.dim() == 2:                 # log p(target) [B,T] of a call inside Captioner.token_logprobs()
        return XETokenLossFn.apply(pred.contiguous(), ln)
    node = _decode_node(pred) if pred.is_contiguous() else None
    return XELossFn.apply(pred.contiguous(), target.long().contiguous(), ln, node)


class RewardLossFn(torch.autograd.Function):
    """RewardCriterion (self_critical/utils.py:169-177) as one launch each way (isc_reward_loss_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, seq_logprobs, seq_masks, reward):
        out2 = torch.empty(2, dtype=torch.float32, device=seq_logprobs.device)
        ops.reward_loss_fwd(seq_logprobs, seq_masks, reward, out2)
        ctx.save_for_backward(seq_masks, reward, out2)
        return out2[0] / out2[1]

    @staticmethod
    def backward(ctx, g):
        seq_masks, reward, out2 = ctx.saved_tensors
        d = torch.empty_like(seq_masks)
        ops.reward_loss_bwd(seq_masks, reward, g.reshape(1).contiguous().float(), out2, d)
        return d, None, None


def reward_criterion(seq_logprobs, seq_masks, reward):
    """-sum(logp * mask * reward) / sum(mask) on the device; `reward` may be a [B,T] tensor of any float dtype or
    broadcastable to it."""
    ops.require_device(seq_logprobs, seq_masks)
    lp = seq_logprobs.float().contiguous()
    mk = seq_masks.float().contiguous()
    rw = torch.as_tensor(reward, dtype=torch.float32, device=lp.device).expand_as(lp).contiguous()
    return RewardLossFn.apply(lp, mk, rw)
