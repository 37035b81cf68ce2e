"""Few-row launches as fused matrix-vector kernels (gemv_rows_kernel; isc_set_gemv_rows): isc_linear_fwd / isc_lstm_fwd /
isc_vocab_fwd with M <= 8 rows - beam rows of one image, roll-outs of a handful of captions.  Checked against fp64
through every epilogue (linear: biases / ReLU / accumulate / keep-mask / pre-mask copy, grouped launches; LSTM cell
with the hoisted term, the token table, saved gates, planes of h; vocabulary statistics with and without logits) on
every row count 1..8, ragged column counts and K that is not a multiple of the 256-wide chunk; bit-repeatable; exact
fp32 (error no larger than the fp32 MFMA tiles'); off where it must be off; and end to end: a beam-5 search and a
4-caption roll-out on this path against the same on the kernels they replaced.  pytest -m gpu."""
import numpy as np
import pytest
import torch

from _split_f16 import planes as _planes
from insenticap_model_amd import Captioner, ops, synth

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _restore():
    yield
    ops.set_h3_mode(1)
    ops.set_tile_override(-1)
    ops.set_gemv_rows(8)


def _rand(g, *shape, scale=1.0):
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _n():
    return ops._lib.load().isc_gemv_launches()


@pytest.mark.parametrize('M', [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize('N,K1,K2', [(512, 512, 0), (130, 96, 32), (1024, 2048, 1024), (20, 32, 0)])
def test_linear_every_feature_vs_fp64(M, N, K1, K2):
    g = torch.Generator().manual_seed(M * 131 + N)
    x1, w1, b0, b1 = _rand(g, M, K1), _rand(g, N, K1, scale=K1 ** -0.5), _rand(g, N), _rand(g, N)
    keep = (torch.rand(M, N, generator=g) > 0.5).to(torch.uint8)
    prior = _rand(g, M, N)
    ref = x1.double() @ w1.double().t() + b0.double() + b1.double() + prior.double()
    segs = [(x1.to(DEV), w1.to(DEV))]
    if K2:
        x2, w2 = _rand(g, M, K2), _rand(g, N, K2, scale=K2 ** -0.5)
        ref = ref + x2.double() @ w2.double().t()
        segs.append((x2.to(DEV), w2.to(DEV)))
    ref_pre = torch.relu(ref)
    ref_out = ref_pre * keep.double() * 2.0
    outs = []
    for rep in range(2):
        n0 = _n()
        out, pre = prior.clone().to(DEV), torch.full((M, N), float('nan'), device=DEV)
        ops.linear_fwd([ops.linear_problem(segs, out, b0.to(DEV), b1.to(DEV), relu=True, keep_mask=keep.to(DEV),
                                           mask_scale=2.0, out_pre=pre, accumulate=True)])
        torch.cuda.synchronize()
        assert _n() == n0 + 1
        np.testing.assert_allclose(out.cpu().numpy(), ref_out.float().numpy(), atol=2e-6, rtol=2e-6)
        np.testing.assert_allclose(pre.cpu().numpy(), ref_pre.float().numpy(), atol=2e-6, rtol=2e-6)
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    ops.set_gemv_rows(0)                                   # the kernels it replaces: same numbers to fp32 rounding
    ops.set_h3_mode(0)
    out0, pre0 = prior.clone().to(DEV), torch.empty(M, N, device=DEV)
    n0 = _n()
    ops.linear_fwd([ops.linear_problem(segs, out0, b0.to(DEV), b1.to(DEV), relu=True, keep_mask=keep.to(DEV),
                                       mask_scale=2.0, out_pre=pre0, accumulate=True)])
    torch.cuda.synchronize()
    assert _n() == n0
    e1 = (pre.double().cpu() - ref_pre).abs().max().item()
    e0 = (pre0.double().cpu() - ref_pre).abs().max().item()
    assert e1 <= e0 * 1.5 + 1e-7, (e1, e0)


def test_linear_three_problems_one_launch_and_strided_output():
    g = torch.Generator().manual_seed(4)
    M, K = 5, 512
    x = _rand(g, M, K).to(DEV)
    ws = [_rand(g, n, K, scale=K ** -0.5).to(DEV) for n in (512, 512, 36)]
    bs = [_rand(g, n).to(DEV) for n in (512, 512, 36)]
    big = torch.zeros(M, 2000, device=DEV)                 # problem 0 writes a column window of a wider tensor
    outs = [big[:, 100:612], torch.empty(M, 512, device=DEV), torch.empty(M, 36, device=DEV)]
    n0 = _n()
    ops.linear_fwd([ops.linear_problem([(x, w)], o, b) for w, o, b in zip(ws, outs, bs)])
    torch.cuda.synchronize()
    assert _n() == n0 + 1
    for w, b, o in zip(ws, bs, outs):
        ref = x.double().cpu() @ w.double().cpu().t() + b.double().cpu()
        np.testing.assert_allclose(o.cpu().numpy(), ref.float().numpy(), atol=2e-6, rtol=2e-6)
    assert float(big[:, :100].abs().max()) == 0.0 and float(big[:, 612:].abs().max()) == 0.0


@pytest.mark.parametrize('M', [1, 4, 5, 8])
@pytest.mark.parametrize('H,with_pre,with_tab', [(512, True, True), (64, True, False), (96, False, False)])
def test_lstm_cell_vs_fp64(M, H, with_pre, with_tab):
    g = torch.Generator().manual_seed(M + H)
    ks = (max(32, H // 32 * 32), 64, 32) if H != 512 else (512, 512, 1024)
    xs = [_rand(g, M, k) for k in ks]
    ws = [_rand(g, 4 * H, k, scale=(3 * k) ** -0.5) for k in ks]
    b_ih, b_hh, c0 = _rand(g, 4 * H), _rand(g, 4 * H), _rand(g, M, H)
    z = sum(x.double() @ w.double().t() for x, w in zip(xs, ws)) + b_ih.double() + b_hh.double()
    kw = {}
    if with_pre:
        pre = _rand(g, M, 4 * H, scale=0.3)
        z = z + pre.double()
        kw['pre'] = pre.to(DEV)
    if with_tab:
        tab = _rand(g, 50, 4 * H, scale=0.3)
        ids = torch.randint(0, 50, (M,), generator=g)
        z = z + tab.double()[ids]
        kw['tab'], kw['tab_ids'] = tab.to(DEV), ids.to(DEV)
    i, f, gg, o = z.split(H, dim=1)
    c_ref = torch.sigmoid(f) * c0.double() + torch.sigmoid(i) * torch.tanh(gg)
    h_ref = torch.sigmoid(o) * torch.tanh(c_ref)
    dx = [x.to(DEV) for x in xs]
    dsegs = [(dx[0], ws[0].to(DEV), _planes(dx[0])), (dx[1], ws[1].to(DEV)), (dx[2], ws[2].to(DEV))]   # planes: ignored
    n0 = _n()
    h, c = torch.empty(M, H, device=DEV), torch.empty(M, H, device=DEV)
    gates = torch.empty(M, 4 * H, device=DEV)
    hp = torch.empty(2, M, H, dtype=torch.float16, device=DEV) if H % 32 == 0 else None
    ops.lstm_fwd(dsegs, b_ih.to(DEV), b_hh.to(DEV), c0.to(DEV), h, c, gates_out=gates, h_planes=hp, **kw)
    torch.cuda.synchronize()
    assert _n() == n0 + 1
    np.testing.assert_allclose(h.cpu().numpy(), h_ref.float().numpy(), atol=3e-6)
    np.testing.assert_allclose(c.cpu().numpy(), c_ref.float().numpy(), atol=3e-6)
    act = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)], dim=1)
    np.testing.assert_allclose(gates.cpu().numpy(), act.float().numpy(), atol=3e-6)
    if hp is not None:
        assert torch.equal(hp.cpu(), _planes(h).cpu())


@pytest.mark.parametrize('M,V,K,logits', [(5, 10000, 512, True), (8, 10000, 512, False), (1, 9487, 512, True),
                                          (3, 130, 64, True), (7, 128, 32, True)])
def test_vocab_statistics_vs_fp64(M, V, K, logits):
    g = torch.Generator().manual_seed(V + M)
    h, W, bias = _rand(g, M, K), _rand(g, V, K, scale=4 * K ** -0.5), _rand(g, V)
    logits_ref = h.double() @ W.double().t() + bias.double()
    lse_ref = torch.logsumexp(logits_ref, 1)
    nt = (V + 127) // 128
    n0 = _n()
    pm, ps = torch.empty(M, nt, device=DEV), torch.empty(M, nt, device=DEV)
    pi = torch.empty(M, nt, device=DEV, dtype=torch.int32)
    lg = torch.full((M, V), float('nan'), device=DEV) if logits else None
    ops.vocab_fwd(h.to(DEV), W.to(DEV), bias.to(DEV), pm, ps, pi, lg)
    torch.cuda.synchronize()
    assert _n() == n0 + 1
    mx = pm.max(1).values
    lse = mx + torch.log((ps * torch.exp(pm - mx[:, None])).sum(1))
    np.testing.assert_allclose(lse.cpu().numpy(), lse_ref.float().numpy(), atol=5e-6, rtol=2e-6)
    arg = pi.gather(1, pm.argmax(1)[:, None]).squeeze(1).long().cpu()
    ref_arg = logits_ref.argmax(1)
    for r in (arg != ref_arg).nonzero().flatten().tolist():
        top2 = logits_ref[r].topk(2).values
        assert (top2[0] - top2[1]).item() < 1e-6, (r, top2)
    if logits:
        np.testing.assert_allclose(lg.cpu().numpy(), logits_ref.float().numpy(), atol=3e-6, rtol=2e-6)
        assert torch.equal(arg, lg.argmax(1).cpu())
        # per-tile statistics are exactly those of the stored logits
        pad = torch.full((M, nt * 128), float('-inf'))
        pad[:, :V] = lg.cpu()
        t = pad.view(M, nt, 128)
        assert torch.equal(pm.cpu(), t.max(2).values)
        assert torch.equal(pi.cpu().long(), t.argmax(2) + torch.arange(nt)[None, :] * 128)


def test_path_is_off_where_it_must_be():
    g = torch.Generator().manual_seed(9)
    x, w = _rand(g, 5, 512).to(DEV), _rand(g, 512, 512, scale=0.05).to(DEV)
    x9 = _rand(g, 9, 512).to(DEV)

    def launches(xx, **kw):
        n0 = _n()
        ops.linear_fwd([ops.linear_problem([(xx, w)], torch.empty(xx.shape[0], 512, device=DEV))])
        torch.cuda.synchronize()
        return _n() - n0
    assert launches(x) == 1 and launches(x9) == 0           # more than 8 rows: the tile kernels
    for mode in (2, 3, 4):                                  # forced split-f16 kernels (their own tests rely on it)
        ops.set_h3_mode(mode)
        assert launches(x) == 0
    ops.set_h3_mode(0)
    assert launches(x) == 1                                 # exact-fp32 engine: this kernel IS exact fp32
    ops.set_h3_mode(1)
    ops.set_tile_override(1)
    assert launches(x) == 0
    ops.set_tile_override(-1)
    assert ops.set_gemv_rows(4) == 8
    assert launches(x) == 0 and launches(x[:4].contiguous()) == 1
    wk = _rand(g, 512, 4128, scale=0.02).to(DEV)            # K beyond the LDS image
    n0 = _n()
    ops.linear_fwd([ops.linear_problem([(_rand(g, 4, 4128).to(DEV), wk)], torch.empty(4, 512, device=DEV))])
    torch.cuda.synchronize()
    assert _n() == n0


def _captioner():
    V, st = 10000, synth.DEFAULT_SETTINGS
    cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)
    cap.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
    return cap.to(DEV).eval(), V, st


def test_beam5_search_and_small_rollout_on_this_path_match_the_replaced_kernels():
    """One image through beam search (5 rows per step) and a 4-caption greedy roll-out: every step's LSTM cells,
    h-projections and classifier go out as matrix-vector launches; captions equal those of the skinny split-f16 kernels
    (tokens on trusted margins, log-probs within 1e-4 - both sit within 1e-4 of the CPU oracle, test_gpu_parity)."""
    cap, V, st = _captioner()
    cap.enable_beam_graphs(False)
    cap.rows_step = False                 # (the few-row decode step of csrc/rows.hip has its own tests: test_gpu_rows.py)
    d = synth.make_inputs(4, V, st, regions=36, seq_len=20, seed=11)
    t = lambda k: torch.from_numpy(np.asarray(d[k])).to(DEV)
    res = {}
    for rows in (8, 0):
        ops.set_gemv_rows(rows)
        n0 = _n()
        with torch.no_grad():
            seq, lp, mk = cap(t('fc_feats'), t('att_feats'), t('cpt_words'), t('senti_words'), t('senti_labels'), 20, 1,
                              mode='rl')
            beam = cap.sample(t('fc_feats')[0], t('att_feats')[0], t('senti_words')[0], t('senti_labels')[0:1], 5, 1, 20)
        torch.cuda.synchronize()
        res[rows] = (seq.cpu(), lp.cpu(), mk.cpu(), beam, _n() - n0)
    assert res[8][4] >= 20 * 4 * 2 - 8 and res[0][4] == 0      # >= 4 launches per step, both searches
    a, b = res[8], res[0]
    same = (a[0] == b[0]).all(1)
    assert same.float().mean() >= 0.75                          # (a near-tie may flip a token between engines)
    assert float((a[1][same] - b[1][same]).abs().max()) < 1e-4
    assert a[3][0][0] == b[3][0][0] or abs(a[3][1][0] - b[3][1][0]) < 1e-3, (a[3], b[3])
