"""fp64 references of the forward pointwise / scan kernels (csrc/pointwise.hip, csrc/attention.hip), one formula per
operation of include/insenticap_hip.h, for tests/test_gpu_forward_kernels.py (checked on the host by
tests/test_fwd_ref_host.py).  The comparison, the bound atol = 8 * max(err32, 2^-23 * max|ref|) and the float32 tanh are
those of tests/_bwd_ref.py: every formula is written once over a dtype, float64 = the reference, float32 = err32.

Outputs that are exact by construction (token ids, masks, counters) are held by `check_exact`; a sampled token by
`check_sample_interval` (the interval test of tests/test_gpu_sampling.py), after which everything downstream of the token
is exact given the token."""
import numpy as np
import torch

from _bwd_ref import (F32, F64, FACTOR, SENTINEL, WORST, _c, both, bound,   # noqa: F401  (re-exported to the tests)
                      check_output, tanh_)

TILE = 128               # columns per tile of the vocabulary statistics (isc_vocab_fwd)
SAMPLE_TOL = 2e-6        # the interval test's slack, as in tests/test_gpu_sampling.py


def _ids(x):
    return x.detach().cpu().to(torch.int64)


def check_exact(got, want, name):
    """Equality of an output with an exact expected value (ids, masks, counters): shape, then every element."""
    got, want = torch.as_tensor(got).detach().cpu(), torch.as_tensor(want).detach().cpu()
    assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
    bad = got.to(F64) != want.to(F64)
    assert not bool(bad.any()), '%s: element %s holds %r, not %r' % (
        name, tuple(bad.nonzero()[0].tolist()), got[bad][0].item(), want[bad][0].item())


# ------------------------------------------------------------------------------------------------ embeddings
def embed_relu_ref(dt, emb, ids, add=None):
    """xt[b,:] = relu(Emb[ids[b]]) (+ add[b,:])"""
    out = torch.relu(_c(emb, dt)[_ids(ids)])
    return {'out': out if add is None else out + _c(add, dt)}


def embed_relu_mean_ref(dt, emb, ids):
    """out[b,:] = mean_c relu(Emb[ids[b,c]]): ReLU per word, the words summed in ascending order, divided by C."""
    e, ids = _c(emb, dt), _ids(ids)
    C = ids.shape[1]
    s = torch.zeros(ids.shape[0], e.shape[1], dtype=dt)
    for c in range(C):
        s = s + torch.relu(e[ids[:, c]])
    return {'out': s / C}


def embed_senti_words_ref(dt, emb, ids, pad_id, keep_mask=None, mask_scale=1.0):
    """out[b,m,:] = relu(Emb[m == 0 ? pad_id : ids[b,m-1]]) [* mask * scale]; out [B, n_words + 1, W]"""
    ids = _ids(ids)
    full = torch.cat([torch.full((ids.shape[0], 1), int(pad_id), dtype=torch.int64), ids], dim=1)
    out = torch.relu(_c(emb, dt)[full])
    if keep_mask is not None:
        out = out * _c(keep_mask, dt) * float(mask_scale)
    return {'out': out}


# ------------------------------------------------------------------------------------------------ gate mix, scan
def gate_mix_ref(dt, z, w, w_bias, v, s):
    """beta = sigmoid(w . tanh(z[b,:]) + *w_bias); out = beta v + (1 - beta) s"""
    u = (tanh_(_c(z, dt)) * _c(w, dt).reshape(-1)).sum(1)
    if w_bias is not None:
        u = u + _c(w_bias, dt).reshape(())
    beta = torch.sigmoid(u)
    bt = beta.unsqueeze(1)
    return {'beta': beta, 'out': bt * _c(v, dt) + (1 - bt) * _c(s, dt)}


def scan_fwd_ref(dt, P, V, q, w, w_bias=None, q2=None, row_ids=None):
    """e_r = w . tanh(P[b,r,:] + q[b,:] (+ q2[b,:])) + *w_bias; alpha = softmax_r(e); out[b,:] = sum_r alpha_r V[b,r,:].
    row_ids [B,R] (gather mode): P / V are tables and region r of row b is their row row_ids[b,r]."""
    P, V = _c(P, dt), _c(V, dt)
    if row_ids is not None:
        P, V = P[_ids(row_ids)], V[_ids(row_ids)]
    qq = _c(q, dt) if q2 is None else _c(q, dt) + _c(q2, dt)
    e = (tanh_(P + qq.unsqueeze(1)) * _c(w, dt).reshape(-1)).sum(-1)
    if w_bias is not None:
        e = e + _c(w_bias, dt).reshape(())
    alpha = torch.softmax(e, dim=-1)
    return {'alpha': alpha, 'out': torch.einsum('br,brd->bd', alpha, V)}


# ------------------------------------------------------------------------------------------------ tile statistics
def tile_stats(x, tile=TILE):
    """(pmax, psum, pidx) per `tile`-column tile of the float32 rows x [M, V] (128: isc_vocab_fwd's; the few-row
    classifier's is isc_rows_stats_tile(V)), made on the host: pmax the tile maximum
    (exact), psum = float32(sum in float64 of exp(x - pmax)), pidx the GLOBAL index of the tile maximum, the smallest on
    ties.  [M, n_tile] float32, float32, int32 - what isc_vocab_fwd leaves for its consumers."""
    x = x.detach().cpu()
    assert x.dtype == F32 and x.dim() == 2
    M, V = x.shape
    nt = (V + tile - 1) // tile
    pad = np.full((M, nt * tile), -np.inf, dtype=np.float64)
    pad[:, :V] = x.numpy()
    t = pad.reshape(M, nt, tile)
    pmax = t.max(axis=2)
    psum = np.exp(t - pmax[:, :, None]).sum(axis=2)
    pidx = t.argmax(axis=2) + np.arange(nt)[None, :] * tile          # numpy: the first maximum
    return (torch.from_numpy(pmax.astype(np.float32)), torch.from_numpy(psum.astype(np.float32)),
            torch.from_numpy(pidx.astype(np.int32)))


def _fold(dt, pmax, psum):
    """gmax and S = sum_j psum_j exp(pmax_j - gmax) of every row"""
    pm, ps = _c(pmax, dt), _c(psum, dt)
    gmax = pm.max(dim=1).values
    return gmax, (ps * torch.exp(pm - gmax.unsqueeze(1))).sum(1)


def logp_from_stats_ref(dt, x, pmax, psum):
    """logp = (x - gmax) - log(sum_j psum_j exp(pmax_j - gmax)), lse = gmax + the same log"""
    gmax, S = _fold(dt, pmax, psum)
    logS = torch.log(S)
    return {'logp': (_c(x, dt) - gmax.unsqueeze(1)) - logS.unsqueeze(1), 'lse': gmax + logS}


def softmax_cdf(x):
    """float64 cumulative softmax of raw logits [M, V] (numpy)"""
    return torch.cumsum(torch.softmax(x.detach().cpu().to(F64), dim=1), dim=1).numpy()


def check_sample_interval(x, u, tok, name, rows=None):
    """An inverse-CDF draw: u within [cdf[tok-1] - 2e-6, cdf[tok] + 2e-6] of the float64 softmax of the raw logits
    (float32 partial sums may move a draw across a boundary only when u sits within rounding of it)."""
    cdf = softmax_cdf(x)
    tok = np.asarray(torch.as_tensor(tok).cpu(), dtype=np.int64)
    un = np.asarray(torch.as_tensor(u).cpu(), dtype=np.float64)
    M, V = cdf.shape
    assert ((tok >= 0) & (tok < V)).all(), (name, 'token out of range')
    r = np.arange(M)
    lo = np.where(tok > 0, cdf[r, np.maximum(tok - 1, 0)], 0.0)
    ok = (un >= lo - SAMPLE_TOL) & (un <= cdf[r, tok] + SAMPLE_TOL)
    if rows is not None:
        ok = ok[np.asarray(rows)]
    assert ok.all(), '%s: a drawn token whose interval does not hold its uniform (first at %d)' % (name, int((~ok).argmax()))


# ------------------------------------------------------------------------------------------------ roll-out step
def rollout_finalize_ref(dt, x, pmax, psum, pidx, unfinished, eos_id, emb, xt_add=None, mode='greedy', forced=None,
                         tokens=None):
    """One step t of the roll-out's state machine, row by row (plain Python over numpy; the two floating outputs in dt).
    mode 'greedy': token = the arg-max (largest tile maximum, the smallest id on ties), lp = -log S;
         'forced': token = forced[b], lp = (x[b, token] - gmax) - log S;
         'sampled': token = tokens[b] (the kernel's draw, held by check_sample_interval), lp as forced.
    Per row: raw = token; a finished row feeds id 0; mask = the old unfinished; unfinished' = u and token != eos;
    xt_next = relu(emb[masked token]) + xt_add.  Returns the columns t of seq / seq_masks / seq_logprobs / raw_tokens,
    the new unfinished, alive[t+1] = the count of unfinished' and xt_next."""
    gmax, S = _fold(dt, pmax, psum)
    logS = torch.log(S)
    pm, pi = pmax.detach().cpu().numpy(), pidx.detach().cpu().numpy()
    u_old = np.asarray(unfinished.detach().cpu(), dtype=np.int64)
    B = pm.shape[0]
    xd = None if x is None else _c(x, dt)
    raw = np.zeros(B, dtype=np.int64)
    lp = torch.zeros(B, dtype=dt)
    for b in range(B):
        if mode == 'greedy':
            raw[b] = min(int(pi[b, j]) for j in range(pm.shape[1]) if pm[b, j] == pm[b].max())
            lp[b] = -logS[b]
        else:
            raw[b] = int((forced if mode == 'forced' else tokens)[b])
            lp[b] = (xd[b, raw[b]] - gmax[b]) - logS[b]
    seq = np.where(u_old != 0, raw, 0)
    u_new = ((u_old != 0) & (seq != int(eos_id))).astype(np.int64)
    xt = torch.relu(_c(emb, dt)[torch.from_numpy(seq)])
    if xt_add is not None:
        xt = xt + _c(xt_add, dt)
    return {'seq': torch.from_numpy(seq), 'seq_masks': torch.from_numpy((u_old != 0).astype(np.float32)),
            'seq_logprobs': lp, 'raw_tokens': torch.from_numpy(raw), 'unfinished': torch.from_numpy(u_new),
            'alive_next': torch.tensor(int(u_new.sum())), 'xt_next': xt}
