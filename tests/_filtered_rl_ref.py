"""References of the differentiable filtered roll-out (self-critical RL under temperature / top-k / top-p).  Test code only.

  * row_grad: the fp64 formula of d log q(tok) / d x for one row, from (x, tau, kept set, banned ids);
  * saved_scalars: what the forward keeps for a row (K* as int64 bits, the largest allowed logit, log Z), from the same;
  * rollout: a differentiable roll-out on the oracle's prologue / step / init_state that draws (or replays) every step's
    token under the sampling controls and the token constraints, the kept set of each step taken from
    _sample_filter_ref.kept_set on the detached row with the banned ids removed first, and returns the model's and the
    sampling log-probabilities with autograd."""
import numpy as np
import torch

import _sample_filter_ref as ref

CON_MAX = 10        # ISC_CON_MAX


def flt_key(x, ids):
    """The 64-bit rank key of csrc/flt_key.h for fp32 logits x at ids: ascending key = descending logit, ties to the
    smaller id."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    dk = np.where(b & 0x80000000, b, ~b & np.uint32(0x7fffffff)).astype(np.uint64)
    return (dk << np.uint64(32)) | np.asarray(ids, dtype=np.uint64)


def kept_ids(x, tau, top_k, top_p, banned=()):
    """The kept set of one row (ids, in rank order): the banned ids leave first, then temperature, top-k, top-p."""
    x = np.asarray(x, dtype=np.float64)
    allowed = np.setdiff1d(np.arange(x.shape[0]), np.asarray([i for i in banned if i >= 0], dtype=np.int64))
    return allowed[ref.kept_set(x[allowed], tau, top_k, top_p)]


def row_grad(x, tau, kept, tok, banned=()):
    """fp64: d log q(tok) / d x_v = (1 / tau) ([v == tok] - [v in K] q_v), q = softmax over K of x / tau."""
    x = np.asarray(x, dtype=np.float64)
    kept = np.setdiff1d(np.asarray(kept, dtype=np.int64), np.asarray(list(banned), dtype=np.int64))
    z = (x[kept] - x[kept].max()) / tau
    q = np.exp(z) / np.exp(z).sum()
    g = np.zeros_like(x)
    g[kept] = -q
    g[tok] += 1.0
    return g / tau


def saved_scalars(x32, tau, kept, banned=()):
    """(kstar as int64 bits, gmax fp32, logz fp32) of a row of fp32 logits whose kept set is `kept` (minus `banned`)."""
    x32 = np.asarray(x32, dtype=np.float32)
    kept = np.setdiff1d(np.asarray(kept, dtype=np.int64), np.asarray(list(banned), dtype=np.int64))
    kstar = flt_key(x32[kept], kept).max()
    g = x32[kept].max()
    logz = np.log(np.exp((x32[kept].astype(np.float64) - float(g)) / tau).sum())
    return np.array([kstar], dtype=np.uint64).view(np.int64)[0], np.float32(g), np.float32(logz)


def banned_ids(ids, cons, t, fed):
    """The ids a row may not choose at step t (forward_rl's token constraints): `fed` = the token fed into the step."""
    ban = []
    if cons.get('suppress_special') and ids.pad != ids.eos:
        ban += [ids.pad, ids.sos, ids.unk]
    if cons.get('decoding_constraint'):
        ban.append(int(fed))
    if t < cons.get('min_len', 0):
        ban.append(ids.eos)
    return sorted(set(ban))


def rollout(p, ids, fc, att, cpt_words, senti_words, senti_labels, T, u, tau=1.0, top_k=0, top_p=1.0, cons=None,
            masks=None, p_drop=0.5, replay=None):
    """The sampled roll-out of oracle.captioner_oracle.forward_rl with the draws made here: at every executed step and row
    the token is `replay`'s, or the reference sampler's for uniform u[b, t] over the row's kept set.  Returns a dict: seq,
    mk, raw (the draws), lp (the model's log-probabilities), slp (the sampling ones: log_softmax(x[K] / tau)[tok]) - both
    [B,T], zero behind the early break, differentiable - P, and per executed (b, t) `kept` (sorted ids), `n_kept`,
    `bound` ('k' / 'p' / '': which control cut the row) and `near` (RowCheck.near_boundary of the draw)."""
    from oracle import captioner_oracle as O
    cons = cons or {}
    u = np.array(u, dtype=np.float32)
    P = O.prologue(p, ids, 'rl', fc, att, cpt_words, senti_words, senti_labels, masks, p_drop)
    B = fc.shape[0]
    state = O.init_state(p, B)
    seq = torch.zeros((B, T), dtype=torch.long)
    raw = torch.zeros((B, T), dtype=torch.long)
    zero = lambda: [fc.new_zeros(B) for _ in range(T)]
    lps, slps, mk = zero(), zero(), fc.new_zeros((B, T))
    it = torch.full((B,), ids.sos, dtype=torch.long)
    unfinished = it == ids.sos
    facts = {}
    for t in range(T):
        om = masks['out'][t] if (masks is not None and 'out' in masks) else None
        logp, state, _ = O.step(p, it, state, P.fc_e, P.att_e, P.p_att, P.words_e, P.p_words, P.label_e, om, p_drop)
        rows = logp.detach().double().numpy()
        toks, s_rows = [], []
        for b in range(B):
            ban = banned_ids(ids, cons, t, it[b])
            allowed = np.setdiff1d(np.arange(rows.shape[1]), np.asarray(ban, dtype=np.int64))
            xa = rows[b, allowed]
            chk = ref.RowCheck(xa, float(u[b, t]), tau, top_k, top_p)
            kept = allowed[chk.order[:chk.n]]
            tok = int(replay[b, t]) if replay is not None else int(allowed[chk.ref_token()])
            n_k = len(allowed) if (top_k == 0 or top_k >= len(allowed)) else top_k
            facts[(b, t)] = dict(kept=np.sort(kept), n_kept=chk.n, ban=ban, near=chk.near_boundary(), live=bool(unfinished[b]),
                                 bound='p' if chk.n < n_k else ('k' if n_k < len(allowed) else ''))
            toks.append(tok)
            kt = torch.from_numpy(kept)
            s_rows.append(torch.log_softmax(logp[b, kt] / tau, dim=0)[int(np.nonzero(kept == tok)[0][0])])
        it = torch.tensor(toks, dtype=torch.long)
        raw[:, t] = it
        lps[t] = logp.gather(1, it.unsqueeze(1)).squeeze(1)
        slps[t] = torch.stack(s_rows)
        mk[:, t] = unfinished.to(mk.dtype)
        it = it * unfinished.to(it.dtype)
        seq[:, t] = it
        unfinished = unfinished & (it != ids.eos)
        if int(unfinished.sum()) == 0:
            break
    return dict(seq=seq, raw=raw, mk=mk, lp=torch.stack(lps, dim=1), slp=torch.stack(slps, dim=1), P=P, facts=facts,
                steps=t + 1, u=u)


# ------------------------------------------------------------------------------------------------ the GPU cases
# (tests/test_gpu_filtered_rl.py runs them; tests/test_filtered_rl_host.py establishes their CPU facts)
V, I, R, T = 64, 3, 6, 8
CONTROLS = {
    'tau0.7': dict(temperature=0.7),
    'k5': dict(top_k=5),
    'p0.8_tau1.3': dict(top_p=0.8, temperature=1.3),
    'k8_p0.9_cons': dict(top_k=8, top_p=0.9, suppress_special=True, decoding_constraint=1),
}
W_SEED, EOS_BIAS = 3, 9.0


def case_weights():
    """The synthetic 'tiny' weights with the classifier's <EOS> bias raised: as drawn, log p(<EOS>) is -11 .. -15 and no
    sampled row would ever end - raised, <EOS> competes with the top ranks: rows end at every step, some at step 1, and
    some cases end before the last step (the early break)."""
    from insenticap_model_amd import synth
    w = synth.make_weights(V, synth.TINY_SETTINGS, seed=W_SEED)
    w['classifier.bias'] = w['classifier.bias'].copy()
    w['classifier.bias'][synth.make_idx2word(V).index('<EOS>')] += EOS_BIAS
    return w


def split_controls(kw):
    flt = {k: kw[k] for k in ('temperature', 'top_k', 'top_p') if k in kw}
    cons = {k: kw[k] for k in ('suppress_special', 'decoding_constraint', 'min_len') if k in kw}
    return flt, cons


def case_inputs(name, n, with_masks):
    """(batch dict of numpy inputs for I images, uniforms [I*n, T] float32, masks or None) of one GPU case.  The seed of
    the uniforms is CASE_SEEDS[...]: chosen (tests/test_filtered_rl_host.py checks it) so that the fp32 and the fp64
    roll-out agree on every kept set, no draw sits within 2e-6 of a CDF boundary and at least five steps run."""
    from insenticap_model_amd import synth
    st = synth.TINY_SETTINGS
    b = synth.make_inputs(I, V, st, regions=R, seq_len=T, seed=60 + n)
    lo = V - 14
    b['senti_words'] = lo + b['senti_words'] % 14
    b['cpt_words'] = 4 + b['cpt_words'] % (lo - 4)
    seed = CASE_SEEDS[(name, n, with_masks)]
    u = np.random.default_rng(seed).random((I * n, T)).astype(np.float32)
    masks = None
    if with_masks:
        E, H, Wd, p_drop = st['feat_emb_dim'], st['rnn_hid_dim'], st['word_emb_dim'], st['dropout_p']
        Mw = b['senti_words'].shape[1] + 1
        g = torch.Generator().manual_seed(n)
        keep = lambda *shape: (torch.rand(*shape, generator=g) >= p_drop).to(torch.uint8)
        masks = dict(fc=keep(I, E), att=keep(I * R, E), words=keep(I * Mw, Wd), label=keep(I, Wd),
                     **{'out%d' % t: keep(I * n, H) for t in range(T)})
    return b, u, masks


def oracle_masks(masks, n):
    """Per-image masks repeated for the oracle's expanded inputs (tests/test_gpu_group_rl.py: _oracle_run)."""
    if masks is None:
        return None
    return dict(fc=masks['fc'].repeat_interleave(n, 0), att=masks['att'].view(I, R, -1).repeat_interleave(n, 0),
                words=masks['words'].view(I, -1, masks['words'].shape[1]).repeat_interleave(n, 0),
                label=masks['label'].repeat_interleave(n, 0), out=torch.stack([masks['out%d' % t] for t in range(T)]))


def oracle_case(name, n, with_masks, dtype=torch.float64, grad=True, replay=None):
    """The reference roll-out of one GPU case on the expanded inputs; returns (parameters, rollout's dict)."""
    from insenticap_model_amd import synth
    from oracle import captioner_oracle as O
    st = synth.TINY_SETTINGS
    w = case_weights()
    b, u, masks = case_inputs(name, n, with_masks)
    p = O.to_params(w, dtype=dtype, requires_grad=grad)
    ids = O.Ids(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES)
    rep = lambda a: torch.from_numpy(np.ascontiguousarray(a)).repeat_interleave(n, 0)
    flt, cons = split_controls(CONTROLS[name])
    with torch.set_grad_enabled(grad):
        out = rollout(p, ids, rep(b['fc_feats']).to(dtype), rep(b['att_feats']).to(dtype), rep(b['cpt_words']),
                      rep(b['senti_words']), rep(b['senti_labels']), T, u, flt.get('temperature', 1.0), flt.get('top_k', 0),
                      flt.get('top_p', 1.0), cons, oracle_masks(masks, n), st['dropout_p'], replay)
    return p, out


# seeds of the uniforms per (controls, n, explicit masks): the first of 0, 1, ... that meets the CPU facts of
# tests/test_filtered_rl_host.py (0 unless listed)
CASE_SEEDS = {(name, n, m): 0 for name in CONTROLS for n in (1, 3) for m in (False, True)}
CASE_SEEDS.update({('tau0.7', 1, True): 7, ('k8_p0.9_cons', 1, True): 7})


def case_facts(name, n, with_masks):
    """The CPU facts of one GPU case: the fp64 roll-out and the fp32 one on the same uniforms.
    Returns (ok, out64): ok = same executed steps, same draws, the same kept set at every executed (row, step), and no
    draw within 2e-6 of a CDF boundary in either."""
    _, o64 = oracle_case(name, n, with_masks, grad=False)
    _, o32 = oracle_case(name, n, with_masks, dtype=torch.float32, grad=False)
    ok = o64['steps'] == o32['steps'] and torch.equal(o64['raw'], o32['raw']) and set(o64['facts']) == set(o32['facts'])
    ok = ok and all(np.array_equal(f['kept'], o32['facts'][k]['kept']) and not f['near'] and not o32['facts'][k]['near']
                    for k, f in o64['facts'].items())
    return ok, o64
