"""The references the forward-kernel tests stand on (tests/_fwd_ref.py), on the host: the float32 evaluation of every
reference passes the comparison of tests/_bwd_ref.py, and every single defect of the kinds a forward kernel can have -
injected into a copy of the float32 evaluation, one at a time - raises.  Outputs that are exact (ids, masks, counters)
are compared by equality.

Not here: the scan without its w_bias.  alpha = softmax(e) is unchanged under a constant added to every score and the
kernel hands out no score, so no output of isc_attn_scan_fwd can show that defect (test_scan_bias_is_not_observable
holds exactly that)."""
import numpy as np
import pytest
import torch

import _fwd_ref as R

F32, F64 = R.F32, R.F64


def _rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _passes(ref, ev32, name):
    assert ref.keys() == ev32.keys()
    for k in ref:
        assert ref[k].dtype == F64 and ev32[k].dtype == F32 and ref[k].shape == ev32[k].shape, (name, k)
        assert R.check_output(ev32[k], ref[k], ev32[k], 'host/%s/%s' % (name, k)) <= 1.0


def _raises(bad, ref, ev32, name):
    with pytest.raises(AssertionError):
        R.check_output(bad, ref, ev32, 'host/' + name)


# ------------------------------------------------------------------------------------------------ embeddings
def _emb_case(seed=1, V=11, W=12, B=5, C=9):
    g = _g(seed)
    emb = _rn(g, V, W)
    ids = torch.randint(0, V, (B, C), generator=g)
    if C > 1:
        ids[:, 1] = ids[:, 0]                   # every row repeats an id
    ids[0, 0], ids[1, C - 1] = 0, V - 1
    return emb, ids, _rn(g, B, W)


def test_embed_relu_reference_and_its_defects():
    emb, ids, add = _emb_case()
    col = ids[:, 2]
    ref, ev = R.both(R.embed_relu_ref, emb, col, add=add)
    _passes(ref, ev, 'embed')
    _passes(*R.both(R.embed_relu_ref, emb, col), 'embed_noadd')
    assert bool((emb[col] < 0).any()) and bool((add < 0).any())
    _raises(torch.relu(emb[col]), ref['out'], ev['out'], 'embed/add omitted')
    _raises(torch.relu(emb[col] + add), ref['out'], ev['out'], 'embed/relu after the add')


@pytest.mark.parametrize('C', [1, 9, 17])
def test_embed_relu_mean_reference_and_its_defects(C):
    emb, ids, _ = _emb_case(C=C)
    ref, ev = R.both(R.embed_relu_mean_ref, emb, ids)
    _passes(ref, ev, 'mean')
    rows = torch.relu(emb[ids])                                                       # [B, C, W]
    _raises(rows.sum(1) / 8, ref['out'], ev['out'], 'mean/divides by 8')
    _raises((rows.sum(1) + rows[:, C - 1]) / C, ref['out'], ev['out'], 'mean/word C-1 twice')
    if C > 1:                                   # (one word: the same expression)
        _raises(torch.relu(emb[ids].sum(1)) / C, ref['out'], ev['out'], 'mean/relu after the sum')


def test_embed_senti_words_reference_and_its_defects():
    g = _g(3)
    V, W, B, n, pad_id = 11, 6, 3, 5, 2
    emb = _rn(g, V, W)
    emb[pad_id] = emb[pad_id].abs() + 0.5
    ids = torch.randint(3, V, (B, n), generator=g)
    mask = (torch.rand(B, n + 1, W, generator=g) > 0.4).to(torch.uint8)
    mask[:, 0] = 1
    ref, ev = R.both(R.embed_senti_words_ref, emb, ids, pad_id, keep_mask=mask, mask_scale=2.0)
    _passes(ref, ev, 'senti')
    _passes(*R.both(R.embed_senti_words_ref, emb, ids, pad_id), 'senti_nomask')
    assert ev['out'].shape == (B, n + 1, W)

    def f(full, scale=2.0):
        return (torch.relu(emb[full]) * mask.float() * scale).reshape(B * (n + 1), W)
    r2, e2 = ref['out'].reshape(-1, W), ev['out'].reshape(-1, W)
    pad = torch.full((B, 1), pad_id)
    assert torch.equal(f(torch.cat([pad, ids], 1)), e2)
    _raises(f(torch.cat([torch.zeros(B, 1, dtype=torch.int64), ids], 1)), r2, e2, 'senti/slot 0 reads id 0')
    _raises(f(torch.cat([pad, ids], 1), scale=1.0), r2, e2, 'senti/mask without scale')
    _raises(f(torch.cat([pad, ids[:, 1:], ids[:, -1:]], 1)), r2, e2, 'senti/off by one on m-1')


# ------------------------------------------------------------------------------------------------ gate mix
def test_gate_mix_reference_and_its_defects():
    g = _g(4)
    B, A, D = 5, 36, 20
    z, w, bias, v, s = _rn(g, B, A), _rn(g, A, scale=0.3), torch.tensor([0.7]), _rn(g, B, D), _rn(g, B, D)
    z[2] = (torch.rand(A, generator=g) * 70 + 30) * torch.where(torch.rand(A, generator=g) > 0.5, 1.0, -1.0)
    ref, ev = R.both(R.gate_mix_ref, z, w, bias, v, s)
    _passes(ref, ev, 'gate')
    _passes(*R.both(R.gate_mix_ref, z, w, None, v, s), 'gate_nobias')
    assert bool(torch.isfinite(ev['beta']).all()) and 0.0 < float(ev['beta'].min()) and float(ev['beta'].max()) < 1.0
    bt = ev['beta'].unsqueeze(1)
    _raises((1 - bt) * v + bt * s, ref['out'], ev['out'], 'gate/beta and 1 - beta swapped')
    nb = R.gate_mix_ref(F32, z, w, None, v, s)
    _raises(nb['beta'], ref['beta'], ev['beta'], 'gate/w_bias dropped (beta)')
    _raises(nb['out'], ref['out'], ev['out'], 'gate/w_bias dropped (out)')
    cut = R.gate_mix_ref(F32, z[:, :A - 4], w[:A - 4], bias, v, s)
    _raises(cut['beta'], ref['beta'], ev['beta'], 'gate/last float4 of A dropped')


# ------------------------------------------------------------------------------------------------ scan
def _scan_case(seed=5, B=3, R_=6, A=8, D=12, n_table=9):
    g = _g(seed)
    return dict(P=_rn(g, n_table, A), V=_rn(g, n_table, D), q=_rn(g, B, A), w=_rn(g, A), q2=_rn(g, B, A),
                bias=torch.tensor([0.4]), ids=torch.randint(0, n_table, (B, R_), generator=g))


def test_scan_reference_and_its_defects():
    c = _scan_case()
    B, R_ = c['ids'].shape
    D = c['V'].shape[1]
    ref, ev = R.both(R.scan_fwd_ref, c['P'], c['V'], c['q'], c['w'], w_bias=c['bias'], q2=c['q2'], row_ids=c['ids'])
    _passes(ref, ev, 'scan_gather')
    Pb, Vb = c['P'][c['ids']], c['V'][c['ids']]                     # the per-row form of the same problem
    ref2, ev2 = R.both(R.scan_fwd_ref, Pb, Vb, c['q'], c['w'], w_bias=c['bias'], q2=c['q2'])
    _passes(ref2, ev2, 'scan')
    assert all(torch.equal(ref[k], ref2[k]) for k in ref)
    assert float(ref['alpha'].sum(1).sub(1).abs().max()) < 1e-12

    no_q2 = R.scan_fwd_ref(F32, Pb, Vb, c['q'], c['w'], w_bias=c['bias'])
    for k in ('alpha', 'out'):
        _raises(no_q2[k], ref[k], ev[k], 'scan/q2 dropped (%s)' % k)
    # D taken as A: rows of V and of `out` addressed with the stride of P (A floats); `out` lies in a sentinel buffer
    A = c['P'].shape[1]
    assert A < D
    Va = Vb.reshape(B, -1)[:, :R_ * A].reshape(B, R_, A)
    wrong = torch.einsum('br,bra->ba', ev['alpha'], Va)
    buf = torch.full((B + 1, D), R.SENTINEL)
    buf.view(-1)[:B * A] = wrong.reshape(-1)
    _raises(buf, ref['out'], ev['out'], 'scan/D taken as A')
    right = torch.full((B + 1, D), R.SENTINEL)
    right[:B] = ev['out']
    R.check_output(right, ref['out'], ev['out'], 'host/scan/out in its buffer')
    # gather ignoring row_ids: region r = row r of the tables
    plain = R.scan_fwd_ref(F32, c['P'][:R_].expand(B, -1, -1), c['V'][:R_].expand(B, -1, -1), c['q'], c['w'],
                           w_bias=c['bias'], q2=c['q2'])
    for k in ('alpha', 'out'):
        _raises(plain[k], ref[k], ev[k], 'scan/gather ignoring row_ids (%s)' % k)


def test_scan_bias_is_not_observable():
    """softmax is shift-invariant: without w_bias both outputs stay within the bound - why no kernel test can hold the
    bias of the scan, and why the defect list of this file leaves it out."""
    c = _scan_case()
    ref, ev = R.both(R.scan_fwd_ref, c['P'], c['V'], c['q'], c['w'], w_bias=c['bias'], q2=c['q2'], row_ids=c['ids'])
    nb = R.scan_fwd_ref(F32, c['P'], c['V'], c['q'], c['w'], q2=c['q2'], row_ids=c['ids'])
    for k in ('alpha', 'out'):
        assert R.check_output(nb[k], ref[k], ev[k], 'host/scan/no bias/' + k) <= R.FACTOR


# ------------------------------------------------------------------------------------------------ statistics, log-softmax
def _rows(seed=6, M=2, V=8321):
    """row 0 has its maximum in the last tile (65), row 1 in tile 0; shifted by +80 / -80"""
    g = _g(seed)
    x = _rn(g, M, V, scale=2.0)
    x[0, V - 1] = 9.0
    x[1, 3] = 9.0
    x[0] += 80.0
    x[1] -= 80.0
    return x


def test_tile_stats_are_the_rows_statistics():
    x = _rows()
    M, V = x.shape
    pm, ps, pi = R.tile_stats(x)
    nt = (V + 127) // 128
    assert nt == 66 and pm.shape == ps.shape == pi.shape == (M, nt)
    assert pm.dtype == F32 and ps.dtype == F32 and pi.dtype == torch.int32
    for j in (0, 1, 64, 65):
        t = x[:, j * 128:(j + 1) * 128]
        assert torch.equal(pm[:, j], t.max(1).values)
        assert torch.equal(x[torch.arange(M), pi[:, j].long()], pm[:, j]) and bool((pi[:, j] // 128 == j).all())
        want = torch.exp(t.double() - pm[:, j].double().unsqueeze(1)).sum(1)
        assert float((ps[:, j].double() - want).abs().max()) <= 2.0 ** -24 * float(want.max())
    assert int(pm[0].argmax()) == 65 and int(pm[1].argmax()) == 0
    tie = torch.zeros(1, 300)
    tie[0, [5, 9, 200, 210]] = 1.0
    assert R.tile_stats(tie)[2].tolist() == [[5, 200, 256]]            # the smallest index on ties, global
    # the statistics fold to the row's log-sum-exp
    ref = R.logp_from_stats_ref(F64, x, pm, ps)
    assert float((ref['lse'] - torch.logsumexp(x.double(), 1)).abs().max()) < 1e-6
    assert float((ref['logp'] - torch.log_softmax(x.double(), 1)).abs().max()) < 1e-6


def test_logsoftmax_reference_and_its_defects():
    x = _rows()
    pm, ps, _ = R.tile_stats(x)
    ref, ev = R.both(R.logp_from_stats_ref, x, pm, ps)
    _passes(ref, ev, 'logp')
    cut = R.logp_from_stats_ref(F32, x, pm[:, :64], ps[:, :64])
    _raises(cut['logp'], ref['logp'], ev['logp'], 'logp/tiles >= 64 ignored')
    _raises(cut['lse'], ref['lse'], ev['lse'], 'logp/tiles >= 64 ignored (lse)')
    gmax = pm.max(1).values
    _raises(ev['lse'] - gmax, ref['lse'], ev['lse'], 'logp/lse = log S without gmax')


def test_sample_interval_holds_the_draw_and_nothing_else():
    g = _g(7)
    x = _rn(g, 4, 300, scale=1.5)
    u = torch.tensor([0.0, 0.3, 0.77, 0.999999])
    cdf = R.softmax_cdf(x)
    tok = np.minimum((cdf > u.double().numpy()[:, None]).argmax(1), 299)
    R.check_sample_interval(x, u, tok, 'host/interval')
    for shift in (-1, 1):
        bad = tok.copy()
        bad[1] += shift
        with pytest.raises(AssertionError):
            R.check_sample_interval(x, u, bad, 'host/interval')
    R.check_sample_interval(x, u, bad, 'host/interval', rows=[0, 2, 3])
    with pytest.raises(AssertionError):
        R.check_sample_interval(x, u, np.array([0, 0, 0, 300]), 'host/interval')


# ------------------------------------------------------------------------------------------------ roll-out step
def _rollout_case(seed=8, B=6, V=300, W=4, eos=5):
    g = _g(seed)
    x = _rn(g, B, V, scale=2.0)
    x[0, 5], x[3, 5] = 20.0, 20.0                  # rows 0 (live) and 3 (finished) draw <EOS>
    x[1, [7, 140]] = 21.0                          # one maximum in two tiles: the smaller id
    unf = torch.tensor([1, 1, 0, 0, 1, 1], dtype=torch.int32)[:B]
    return dict(x=x, stats=R.tile_stats(x), unf=unf, eos=eos, emb=_rn(g, V, W), add=_rn(g, B, W),
                forced=torch.tensor([5, 0, 9, 5, 299, 17])[:B])


def _rollout(c, dt, mode, **kw):
    pm, ps, pi = c['stats']
    return R.rollout_finalize_ref(dt, c['x'], pm, ps, pi, c['unf'], c['eos'], c['emb'], xt_add=c['add'], mode=mode, **kw)


EXACT = ('seq', 'seq_masks', 'raw_tokens', 'unfinished', 'alive_next')


@pytest.mark.parametrize('mode', ['greedy', 'forced', 'sampled'])
def test_rollout_reference_every_rule(mode):
    c = _rollout_case()
    kw = {'forced': dict(forced=c['forced']), 'sampled': dict(tokens=c['forced']), 'greedy': {}}[mode]
    ref, ev = _rollout(c, F64, mode, **kw), _rollout(c, F32, mode, **kw)
    for k in EXACT:
        R.check_exact(ev[k], ref[k], 'host/rollout/' + k)
    for k in ('seq_logprobs', 'xt_next'):
        assert R.check_output(ev[k], ref[k], ev[k], 'host/rollout/' + k) <= 1.0
    want_raw = c['x'].argmax(1) if mode == 'greedy' else c['forced']
    if mode == 'greedy':
        assert int(ref['raw_tokens'][1]) == 7
        lsm = torch.log_softmax(c['x'].double(), 1)
        assert float((ref['seq_logprobs'] - lsm.max(1).values).abs().max()) < 1e-6
    R.check_exact(ref['raw_tokens'][[0, 2, 3, 4, 5]], want_raw[[0, 2, 3, 4, 5]], 'host/rollout/raw')
    assert ref['seq'].tolist()[2:4] == [0, 0] and ref['seq_masks'].tolist() == [1, 1, 0, 0, 1, 1]
    assert ref['unfinished'].tolist() == [0, 1, 0, 0, 1, 1] and int(ref['alive_next']) == 3
    assert torch.equal(ref['xt_next'][2], torch.relu(c['emb'][0].double()) + c['add'][2].double())


def test_rollout_defects_are_caught_by_equality():
    c = _rollout_case()
    ref, ev = _rollout(c, F64, 'greedy'), _rollout(c, F32, 'greedy')
    u = c['unf'].long()
    with pytest.raises(AssertionError):                        # a finished row keeps its token
        R.check_exact(ev['raw_tokens'], ref['seq'], 'host/rollout/finished row keeps its token')
    with pytest.raises(AssertionError):                        # ... and feeds that token's embedding
        keep = torch.relu(c['emb'][ev['raw_tokens']]) + c['add']
        R.check_output(keep, ref['xt_next'], ev['xt_next'], 'host/rollout/finished row keeps its token (xt_next)')
    with pytest.raises(AssertionError):                        # <EOS> does not clear unfinished
        R.check_exact(u, ref['unfinished'], 'host/rollout/eos does not clear')
    with pytest.raises(AssertionError):                        # alive[t+1] counts u instead of u'
        R.check_exact(u.sum(), ref['alive_next'], 'host/rollout/alive counts u')
    pm, _, pi = c['stats']
    larger = torch.stack([pi[b][pm[b] == pm[b].max()].max() for b in range(pm.shape[0])]).long()
    assert larger.tolist()[1] == 140
    with pytest.raises(AssertionError):                        # a tie resolves to the larger id
        R.check_exact(larger, ref['raw_tokens'], 'host/rollout/tie to the larger id')
    with pytest.raises(AssertionError):                        # a shape is part of equality
        R.check_exact(ref['seq'][:5], ref['seq'], 'host/rollout/shape')
