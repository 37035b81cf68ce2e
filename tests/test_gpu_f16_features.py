"""float16 region features from the stores to the att_embed GEMM.  The split-f16 engine writes an fp32 operand as
hi + lo * 2^-11 with hi = f16(x); a value that already IS an f16 has hi == x and lo == 0 exactly, so reading f16 rows
natively (isc_seg.a_f16, the large split-f16 tile kernels) computes what the fp32 path computes on the up-cast values,
bit for bit.  Every check here is therefore `torch.equal` against the same call with `x.float()` - no tolerance - at the
GEMM level (every tile geometry, the half-line tail, strides, mixed segments, every fall-back with its counter), end to
end (greedy / filtered roll-outs, beam search, Detector.sample), through one training step, for out-of-domain batches and
for the device-resident store.  pytest -m gpu.

Two cases differ from the plain reading of their description, for reasons that lie in the dispatch as it stands:
  * 128-row tile at M = 1000 under isc_set_h3_mode(2) with K = 2048: a launch of 128 row-blocks of 32 and 64 chunks is
    taken by split-K in front of the split-f16 kernels (plan_splitk), for fp32 rows as well - so that case converts, and
    the 128-row tile is reached with K = 2048 at M = 5000 (160 tiles of 128 x 128; clamped last tile, M % 8 != 0 too).
  * K = 48: isc_linear_fwd answers ISC_E_SHAPE for K % 32 != 0 whatever the dtype, so "equal" means: the f16 call converts
    (counter) and then raises exactly as the fp32 call does."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from insenticap_model_amd import Captioner, _lib, data, ops, synth

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
N = 512


@pytest.fixture(autouse=True)
def _restore():
    yield
    ops.set_h3_mode(1)
    ops.set_tile_override(-1)


def counters():
    lib = _lib.load()
    return {'h3': lib.isc_h3_launches(), 'h3x': lib.isc_h3x_launches(), 'f16a': lib.isc_h3_f16a_launches(),
            'conv': lib.isc_f16_convert_launches(), 'gemv': lib.isc_gemv_launches(), 'h3s': lib.isc_h3s_launches(),
            **{'kind%d' % k: ops.h3_kernel_launches(k) for k in range(ops.H3_KINDS)}}


def moved(before):
    now = counters()
    return {k: now[k] - before[k] for k in now}


def same(a, b, nan=False):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(
        torch.nan_to_num(a, nan=12345.0) if nan else a, torch.nan_to_num(b, nan=12345.0) if nan else b)


_W = {}


def weights(K):
    if K not in _W:
        g = torch.Generator().manual_seed(K)
        _W[K] = ((torch.randn(N, K, generator=g) * K ** -0.5).to(DEV), torch.randn(N, generator=g).to(DEV))
    return _W[K]


def linear(x, K, full):
    """ops.linear_fwd of x [M, K] (any dtype / stride) against the shared weights; `full`: relu + bias + keep_mask +
    out_pre.  Returns (out, pre or None)."""
    w, b = weights(K)
    M = x.shape[0]
    out = torch.full((M, N), float('nan'), device=DEV)
    if not full:
        ops.linear_fwd([ops.linear_problem([(x, w)], out)])
        return out, None
    keep = (torch.rand(M, N, generator=torch.Generator().manual_seed(M)) > 0.5).to(torch.uint8).to(DEV)
    pre = torch.full((M, N), float('nan'), device=DEV)
    ops.linear_fwd([ops.linear_problem([(x, w)], out, b, relu=True, keep_mask=keep, mask_scale=2.0, out_pre=pre)])
    return out, pre


def feats16(M, K, seed=0, ld=None):
    g = torch.Generator().manual_seed(seed * 7919 + M + K)
    x = torch.randn(M, ld or K, generator=g).half().to(DEV)
    return x[:, :K] if ld else x


def check_equal(x16, K, full, mode=1):
    ops.set_h3_mode(mode)
    ref = linear(x16.float(), K, full)
    c = counters()
    got = linear(x16, K, full)
    d = moved(c)
    torch.cuda.synchronize()
    assert same(got[0], ref[0]) and (not full or same(got[1], ref[1]))
    assert not torch.isnan(got[0]).any()
    return d


# ------------------------------------------------------------------ 1. GEMM level
GEOMS = {'256': (14336, 1), '64': (4096, 1), '128': (5000, 1), '128_forced_m1000': (1000, 2)}
# the f16-row kind of ops.h3_kernel_launches each geometry must run (3 g + 2, g = 0 / 1 / 2 for 128 / 256 / 64 rows).  M =
# 1000 under mode 2 is 32 tiles of 128 x 128 = 64 tiles of 64 x 128: h3_plan's half_tile rule gives it the 64-row tile,
# not the 128-row one its name promises (the 128-row tile is M = 5000's: 160 tiles, 316 of 64 rows = two rounds)
GEOM_KIND = {'256': 5, '64': 8, '128': 2, '128_forced_m1000': 8}


@pytest.mark.parametrize('full', [False, True], ids=['plain', 'relu_bias_mask_pre'])
@pytest.mark.parametrize('K', [64, 96, 2048])
@pytest.mark.parametrize('geom', list(GEOMS))
def test_native_geometries(geom, K, full):
    M, mode = GEOMS[geom]
    d = check_equal(feats16(M, K), K, full, mode)
    if geom == '128_forced_m1000' and K == 2048:     # split-K takes this launch in front of the split-f16 kernels
        assert d['conv'] == 1 and d['f16a'] == 0 and d['h3'] == 0
        return
    assert d['f16a'] == 1 and d['h3'] == 1 and d['conv'] == 0 and d['gemv'] == 0 and d['h3s'] == 0, d
    assert d['h3x'] == (1 if geom == '256' else 0), d
    kinds = {k: v for k, v in d.items() if k.startswith('kind') and v}
    assert kinds == {'kind%d' % GEOM_KIND[geom]: 1, 'kind16': 1}, kinds      # the tile's f16-row form + one weight split


@pytest.mark.parametrize('geom', ['256', '64', '128'])
def test_row_stride_of_a_wider_tensor(geom):
    M, mode = GEOMS[geom]
    K = 96
    x = feats16(M, K, seed=1, ld=K + 64)
    assert x.stride(0) == K + 64
    d = check_equal(x, K, True, mode)
    assert d['f16a'] == 1 and d['conv'] == 0, d


def _planes(x):
    """The interleaved hi / lo plane buffer of x [M, K] (include/insenticap_hip.h: isc_seg.A_hi) as a [2, M, K] tensor."""
    M, K = x.shape
    hi = x.half()
    lo = ((x - hi.float()) * 2048.0).half()
    buf = torch.stack([hi.view(M, K // 32, 32), lo.view(M, K // 32, 32)], dim=2).contiguous()
    return buf.view(2, M, K)


@pytest.mark.parametrize('geom', ['256', '64', '128', '128_forced_m1000'])
def test_three_segment_problem(geom):
    """f16 rows K = 96 (odd chunk count: the parity restarts behind it), fp32 rows K = 64, a plane segment K = 32."""
    M, mode = GEOMS[geom]
    g = torch.Generator().manual_seed(M)
    x16 = feats16(M, 96, seed=2)
    x32 = torch.randn(M, 64, generator=g).to(DEV)
    xp = torch.randn(M, 32, generator=g).to(DEV)
    pl = _planes(xp)
    (w1, b), (w2, _), w3 = weights(96), weights(64), (torch.randn(N, 32, generator=g) * 0.2).to(DEV)
    ops.set_h3_mode(mode)
    outs = []
    for a in (x16.float(), x16):
        out = torch.full((M, N), float('nan'), device=DEV)
        c = counters()
        ops.linear_fwd([ops.linear_problem([(a, w1), (x32, w2), (xp, w3, pl)], out, b, relu=True)])
        d = moved(c)
        outs.append(out)
    torch.cuda.synchronize()
    assert same(outs[0], outs[1]) and not torch.isnan(outs[1]).any()
    assert d['f16a'] == 1 and d['conv'] == 0, d
    # ... and the f16 segment last (the launch ends on a half line), in a grouped launch next to an fp32 problem
    outs = []
    for a in (x16.float(), x16):
        o1, o2 = torch.full((M, N), float('nan'), device=DEV), torch.full((M, N), float('nan'), device=DEV)
        ops.linear_fwd([ops.linear_problem([(x32, w2), (a, w1)], o1, b), ops.linear_problem([(x32, w2)], o2)])
        outs.append((o1, o2))
    torch.cuda.synchronize()
    assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1])


def test_fallback_gemv():
    d = check_equal(feats16(4, 2048, seed=3), 2048, True)
    assert d['conv'] == 1 and d['f16a'] == 0 and d['gemv'] == 1, d


def test_fallback_skinny_kernels_inside_a_weights_scope():
    x = feats16(300, 2048, seed=4)
    with ops.h3_weights_scope(DEV):
        d = check_equal(x, 2048, True)
    assert d['conv'] == 1 and d['f16a'] == 0 and d['h3s'] == 1, d


def test_fallback_exact_engine():
    d = check_equal(feats16(4096, 2048, seed=5), 2048, True, mode=0)
    assert d['conv'] == 1 and d['f16a'] == 0 and d['h3'] == 0, d


def test_fallback_misaligned_row_stride():
    x = feats16(4096, 64, seed=6, ld=68)            # 68 halfs: rows are not 16-byte aligned
    d = check_equal(x, 64, True)
    assert d['conv'] == 1 and d['f16a'] == 0 and d['h3'] == 1, d      # the fp32 copy still takes the split-f16 kernel


def test_fallback_k_48():
    """K % 32 != 0 is ISC_E_SHAPE for every dtype (check_segs): the f16 call converts, then fails as the fp32 call does."""
    x = feats16(4096, 48, seed=7)
    with pytest.raises(_lib.HipLibraryError, match='ISC_E_SHAPE') as e32:
        linear(x.float(), 48, False)
    c = counters()
    with pytest.raises(_lib.HipLibraryError, match='ISC_E_SHAPE') as e16:
        linear(x, 48, False)
    d = moved(c)
    assert str(e16.value) == str(e32.value)
    assert d['conv'] == 1 and d['f16a'] == 0 and d['h3'] == 0, d


def test_convert_kernel_is_exact_on_odd_shapes():
    for rows, cols, ld in ((5, 7, 9), (33, 64, 64), (1000, 2048, 2048), (3, 8, 24)):
        x = feats16(rows, cols, seed=8, ld=ld if ld != cols else None)
        assert same(ops.f16_to_f32(x), x.float())


def test_entry_points_that_cannot_read_halfs_refuse():
    lib = _lib.load()
    x, (w, b) = feats16(256, 64, seed=9), weights(64)
    out = torch.zeros(256, N, device=DEV)
    c = counters()
    p = ops.linear_problem([(x, w)], out)
    assert p.seg[0].a_f16 == 1
    arr = (_lib.LinearProblem * 1)(p)
    for layout in (1, 2):
        assert lib.isc_gemm_bwd(arr, 1, layout, ops.stream()) == -2
    lp = _lib.LstmProblem()
    lp.seg[0] = p.seg[0]
    lp.nseg, lp.M, lp.H = 1, 256, 128
    z = torch.zeros(256, 128, device=DEV)
    lp.c_prev, lp.h_out, lp.c_out, lp.b_ih, lp.b_hh = (z.data_ptr(),) * 3 + (b.data_ptr(),) * 2
    assert lib.isc_lstm_fwd(ctypes.byref(lp), ops.stream()) == -2
    # the forward entry itself, where its dispatch would not take the native path (few rows: GEMV)
    arr[0].M = 4
    assert lib.isc_linear_f16_native(arr, 1, ops.stream()) == 0
    assert lib.isc_linear_fwd(arr, 1, ops.stream()) == -2
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and all(v == 0 for v in moved(c).values())     # nothing was launched


# ------------------------------------------------------------------ 2. end to end
V, R, T = 10000, 36, 3


@pytest.fixture(scope='module')
def cap():
    c = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, synth.DEFAULT_SETTINGS)
    c.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, synth.DEFAULT_SETTINGS, seed=0).items()})
    return c.to(DEV).eval()


def inputs(B, seed=11, regions=R, seq_len=T):
    d = synth.make_inputs(B, V, synth.DEFAULT_SETTINGS, regions=regions, seq_len=seq_len, seed=seed)
    d = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in d.items() if isinstance(v, np.ndarray)}
    d['fc16'], d['att16'] = d['fc_feats'].half(), d['att_feats'].half()
    d['fc32'], d['att32'] = d['fc16'].float(), d['att16'].float()
    return d


def rollout(c, d, which, **kw):
    with torch.no_grad():
        out = c.forward_rl(d['fc' + which], d['att' + which], d['cpt_words'], d['senti_words'], d['senti_labels'], T,
                           kw.pop('sample_max', 1), **kw)
    w = [x.clone() if torch.is_tensor(x) else x for x in (c.cont_weights, c.senti_weights, c.cont_senti_weights)]
    return [x.clone() for x in out] + w


def assert_rollouts_equal(a, b, nan=False):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.is_tensor(x) == torch.is_tensor(y)
        if torch.is_tensor(x):
            assert same(x, y, nan=nan and x.is_floating_point())


def plain(x):
    """Nested results (lists / tuples of strings, floats, arrays, tensors) as plain Python values."""
    if torch.is_tensor(x):
        return x.cpu().tolist()
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (list, tuple)):
        return [plain(y) for y in x]
    return x


def test_greedy_rollout_few_rows(cap):
    d = inputs(4)
    assert_rollouts_equal(rollout(cap, d, '16'), rollout(cap, d, '32'))


def test_greedy_rollout_graph_served(cap):
    d = inputs(128, seed=12)
    cap.enable_rollout_graphs(True)
    try:
        ref = [rollout(cap, d, '32') for _ in range(3)][-1]           # eager, capture, replay
        got = [rollout(cap, d, '16') for _ in range(3)]              # float16 inputs: captures of their own
        keys = list(cap._rollout_graphs)
        assert any(k[0][1][1] == torch.float16 for k in keys) and any(k[0][1][1] == torch.float32 for k in keys)
        assert all(isinstance(cap._rollout_graphs[k], tuple) for k in keys)      # both are captured graphs by now
    finally:
        cap.enable_rollout_graphs(False)
    for g in got:
        assert_rollouts_equal(g, ref)


def test_greedy_rollout_native_att_embed_makes_no_fp32_image(cap):
    """B = 96, eager: att_embed is [3456 x 2048 x 512] - inside the roll-out's weights scope the large split-f16 kernels
    take it (more rows than the skinny kernels serve, enough row blocks that split-K stays out; B = 64 under
    isc_set_h3_mode(2), 288 row blocks, is split over K instead) and read the float16 rows natively: the convert counter
    moves for the fc features' few-row launch at most, never for a [B R, 2048] image."""
    d = inputs(96, seed=13)
    ref = rollout(cap, d, '32')
    seen = []
    orig = ops.f16_to_f32
    ops.f16_to_f32 = lambda x, out=None: (seen.append(tuple(x.shape)), orig(x, out))[1]
    try:
        c = counters()
        got = rollout(cap, d, '16')
        m = moved(c)
    finally:
        ops.f16_to_f32 = orig
    assert_rollouts_equal(got, ref)
    assert m['f16a'] >= 1
    assert m['conv'] == len(seen) and all(s[0] != 96 * R for s in seen), (m, seen)


def test_beam_search(cap):
    d = inputs(8, seed=14, seq_len=20)
    with torch.no_grad():
        for n in (1, 8):
            a = [d[k][:n] for k in ('fc16', 'att16', 'senti_words', 'senti_labels')]
            b = [d[k][:n] for k in ('fc32', 'att32', 'senti_words', 'senti_labels')]
            for _ in range(2):                  # (the second call is served from the search's graph where it has one)
                got, ref = cap.sample_batch(*a, 5, 1, 20), cap.sample_batch(*b, 5, 1, 20)
                assert len(got) == 3 and plain(got) == plain(ref)        # captions, scores, ids
                assert len(got[0]) == n and len(got[0][0]) == 5
        got = cap.sample(d['fc16'][0], d['att16'][0], d['senti_words'][0], d['senti_labels'][0:1], 5, 1, 20)
        ref = cap.sample(d['fc32'][0], d['att32'][0], d['senti_words'][0], d['senti_labels'][0:1], 5, 1, 20)
        assert plain(got) == plain(ref)
        u = torch.rand(8, 6, generator=torch.Generator().manual_seed(9)).to(DEV)
        got = cap.sample_captions(d['fc16'][:4], d['att16'][:4], d['cpt_words'][:4], d['senti_words'][:4],
                                  d['senti_labels'][:4], n=2, max_seq_len=6, temperature=0.9, top_k=50, _uniforms=u)
        ref = cap.sample_captions(d['fc32'][:4], d['att32'][:4], d['cpt_words'][:4], d['senti_words'][:4],
                                  d['senti_labels'][:4], n=2, max_seq_len=6, temperature=0.9, top_k=50, _uniforms=u)
        assert plain(got) == plain(ref)


def test_filtered_sampling(cap):
    d = inputs(16, seed=15)
    u = torch.rand(16, T, generator=torch.Generator().manual_seed(3)).to(DEV)
    kw = dict(sample_max=0, temperature=0.8, top_p=0.9, _uniforms=u)
    assert_rollouts_equal(rollout(cap, d, '16', **dict(kw)), rollout(cap, d, '32', **dict(kw)))


def test_detector_sample():
    from insenticap_model_amd.detector import Detector
    from test_detector import load_helper
    st = dict(synth.DEFAULT_SETTINGS, **synth.HELPER_SETTINGS)
    det = Detector(synth.make_idx2word(V), 20, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-5}, st)
    det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
    load_helper(det.senti_detector, 51)
    det.to(DEV).eval()
    batches, _ = synth.make_rl_batches(1, 2, V, st, grid=(6, 6), seq_len=20, seed=60)
    b = batches[0]
    for i in range(2):
        fc, att, sw = (torch.from_numpy(b[k][i]).to(DEV) for k in (1, 2, 5))
        got = det.sample(fc.half(), att.half(), sw, beam_size=3, decoding_constraint=1)
        ref = det.sample(fc.half().float(), att.half().float(), sw, beam_size=3, decoding_constraint=1)
        assert list(got[0]) == list(ref[0]) and list(got[1]) == list(ref[1])


# ------------------------------------------------------------------ 3. training
def test_training_step_is_that_of_the_upcast_features():
    """One eager XE + seq2seq step (8 + 4 rows, T = 4), dropout masks replayed: a backward will run, so the batch is
    converted once in front of the prologue - losses, every gradient and the post-step parameters are those of
    feats.float() by construction."""
    st = synth.DEFAULT_SETTINGS
    B, S, Tt = 8, 4, 4
    E, H, Wd = st['feat_emb_dim'], st['rnn_hid_dim'], st['word_emb_dim']
    d = synth.make_inputs(B, V, st, regions=R, seq_len=Tt, seed=21)
    s = synth.make_inputs(S, V, st, regions=R, seq_len=Tt, seed=22)
    t = lambda x: torch.from_numpy(x).to(DEV)      # noqa: E731
    g = torch.Generator().manual_seed(5)
    Mw = s['senti_words'].shape[1] + 1

    def m(*shape):
        return (torch.rand(*shape, generator=g) < 0.5).to(torch.uint8)
    m1 = {'fc': m(B, E), 'att': m(B * R, E), 'label': m(B, Wd)}
    m2 = {'cpt': m(S, E), 'words': m(S * Mw, Wd), 'label': m(S, Wd)}
    for i in range(Tt):
        m1['out%d' % i], m2['out%d' % i] = m(B, H), m(S, H)
    res = []
    for half in (True, False):
        cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)
        cap.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
        cap.to(DEV).train()
        optim, xc, dc = cap.get_optim_criterion(4e-4)
        fc, att = t(d['fc_feats']).half(), t(d['att_feats']).half()
        if not half:
            fc, att = fc.float(), att.float()
        caps, s_caps = t(d['captions']), t(s['captions'])
        c = counters()
        pred, pred2 = cap.forward_xe_seq2seq(fc, att, t(d['cpt_words']), caps, t(d['senti_labels']), 0.0, s_caps,
                                             t(s['cpt_words']), t(s['senti_words']), t(s['senti_labels']), 0.0,
                                             _masks=m1, _s_masks=m2)
        xe, s2s = xc(pred, caps[:, 1:], d['lengths']), xc(pred2, s_caps[:, 1:], s['lengths'])
        da = dc(cap.cpt_feats, cap.fc_feats.detach())
        (xe + da + s2s).backward()
        assert moved(c)['f16a'] == 0                 # training reads the fp32 copy, forward and backward
        grads = {k: q.grad.detach().clone() for k, q in cap.named_parameters() if q.grad is not None}
        optim.step()
        torch.cuda.synchronize()
        res.append((xe.detach().clone(), s2s.detach().clone(), grads,
                    {k: q.detach().clone() for k, q in cap.named_parameters()}))
    a, b = res
    assert same(a[0], b[0]) and same(a[1], b[1])
    assert a[2].keys() == b[2].keys() and len(a[2]) >= 30
    for k in a[2]:
        assert same(a[2][k], b[2][k]), k
    for k in a[3]:
        assert same(a[3][k], b[3][k]), k


# ------------------------------------------------------------------ 4. domain
@pytest.mark.parametrize('mode', [1, 0])
def test_out_of_domain_batch(mode):
    """A float16 can only leave the split-f16 domain as inf / NaN: such a batch goes to the exact engine, with the one
    warning, and equals (NaN == NaN) the fp32 batch with the same inf."""
    d = inputs(16, seed=31)
    d['att16'] = d['att16'].clone()
    d['att16'][3, 5, 100] = float('inf')
    d['att32'] = d['att16'].float()
    outs = []
    for which in ('16', '32'):
        c = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, synth.DEFAULT_SETTINGS)
        c.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, synth.DEFAULT_SETTINGS, seed=0).items()})
        c.to(DEV).eval()
        ops.set_h3_mode(mode)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            cnt = counters()
            outs.append(rollout(c, d, which))
            outs.append(rollout(c, d, which))                          # (warned once per captioner)
            m = moved(cnt)
        n_warn = sum('split-f16 operand domain' in str(w.message) for w in rec)
        assert n_warn == (1 if mode == 1 else 0), n_warn               # (engine off: nothing to leave)
        assert m['f16a'] == 0 and m['h3'] == 0, m                      # the exact engine served it
    assert_rollouts_equal(outs[0], outs[2], nan=True)
    assert_rollouts_equal(outs[1], outs[3], nan=True)
    assert ops.h3_mode() == mode


# ------------------------------------------------------------------ 5. stores
def test_device_store_delivers_float16_batches(cap):
    n, Bt = 24, 8
    st = synth.DEFAULT_SETTINGS
    r = np.random.RandomState(4)
    fns = ['img%d' % i for i in range(n)]
    fc = np.abs(r.randn(n, 2048)).astype(np.float32)
    att = np.abs(r.randn(n, 6, 6, 2048)).astype(np.float32)
    fc16, att16 = fc.astype(np.float16), att.astype(np.float16)
    with pytest.raises(ValueError, match='70000'):
        bad = fc.copy()
        bad[2, 7] = 70000.0
        data.DeviceFeatureStore.from_arrays(fns, bad, DEV, dtype=torch.float16)
    s16 = [data.DeviceFeatureStore.from_arrays(fns, a, DEV, chunk_rows=10, dtype=torch.float16) for a in (fc, att)]
    s32 = [data.DeviceFeatureStore.from_arrays(fns, a, DEV, chunk_rows=10) for a in (fc16, att16)]   # the same values, fp32
    assert s16[0].tensor.dtype == torch.float16 and s16[1].tensor.dtype == torch.float16
    assert s32[1].tensor.dtype == torch.float32
    assert same(s16[1].tensor, torch.from_numpy(att16).to(DEV)) and same(s32[1].tensor, s16[1].tensor.float())
    caps = {fn: [[1, 5 + i, 6, 2], [1, 7, 2]] for i, fn in enumerate(fns)}
    cpts = {fn: [10 + i, 11, 12] for i, fn in enumerate(fns)}
    sentis = {fn: [20 + i, 21] for i, fn in enumerate(fns)}
    batches = []
    for stores in (s16, s32):
        import random
        random.seed(7)
        loader = data.get_rl_fact_dataloader(stores[0], stores[1], caps, cpts, sentis, 0, 16, 5, 10, Bt, shuffle=False)
        batches.append(list(data.DevicePrefetcher(loader, DEV)))
    assert len(batches[0]) == 3
    labels = torch.arange(Bt, device=DEV) % 3
    for b16, b32 in zip(*batches):
        assert b16[0] == b32[0]
        assert b16[1].dtype == torch.float16 and b16[2].dtype == torch.float16 and b16[2].shape == (Bt, 6, 6, 2048)
        assert b32[2].dtype == torch.float32 and same(b16[2].float(), b32[2]) and same(b16[1].float(), b32[1])
    b16, b32 = batches[0][0], batches[1][0]
    with torch.no_grad():
        got = cap.forward_rl(b16[1], b16[2], b16[4], b16[5], labels, T, 1)
        ref = cap.forward_rl(b32[1], b32[2], b32[4], b32[5], labels, T, 1)
    for x, y in zip(got, ref):
        assert same(x, y)
    # a host store written as float16 + plain collate + prefetcher (kept pinned buffers, plain memcpy): float16 as well
    host = {fn: att16[i] for i, fn in enumerate(fns)}, {fn: fc16[i] for i, fn in enumerate(fns)}
    loader = data.get_rl_fact_dataloader(host[1], host[0], caps, cpts, sentis, 0, 16, 5, 10, Bt, shuffle=False)
    hb = list(data.DevicePrefetcher(loader, DEV))
    assert hb[0][2].dtype == torch.float16 and hb[0][2].is_cuda and hb[0][1].dtype == torch.float16
    assert sorted(hb[0][0]) == sorted(batches[0][0][0])
