"""Several captions per image without repeating the image's features: the grouped attention scan
(isc_scan_problem.row_div, attn_scan_group_kernel), the LSTM's per-image hoisted term (isc_lstm_problem.pre_div) and
Captioner.forward_rl(captions_per_image=n) / sample_captions(share_image=True) on top of them.

References: the existing kernels on the inputs expanded with repeat_interleave(n, 0) for the BITS (torch.equal: the
grouped kernels run the same per-row arithmetic), the fp64 formula of tests/test_gpu_parity.py::test_attention_scan_vs_fp64
with its tolerances (alpha 2e-6, out 1e-5) for the maths, and at the roll-out level - where the prologue's GEMMs run at
other row counts in the two forms - the project's bars between two correct implementations (tests/test_gpu_parity.py:
1e-4 on a log-probability, 1e-5 on an attention weight) and the CPU oracle (1e-4)."""
import numpy as np
import pytest
import torch

from conftest import case_setup
from insenticap_model_amd import Captioner, ops, synth

pytestmark = pytest.mark.gpu

LOGP_TOL = 1e-4          # tests/test_gpu_parity.py
W_TOL = 1e-5


@pytest.fixture(autouse=True)
def _restore():
    yield
    ops.set_h3_mode(1)


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def rep(x, n):
    return None if x is None else x.repeat_interleave(n, 0).contiguous()


# ----------------------------------------------------------------------------- 1. the scan, bit for bit
def _scan_case(I, n, R, A, seed, with_q2=False):
    g = torch.Generator().manual_seed(seed)
    d = dict(P=torch.randn(I, R, A, generator=g), V=torch.randn(I, R, A, generator=g),
             q=torch.randn(I * n, A, generator=g), w=torch.randn(1, A, generator=g) * 0.3,
             wb=torch.randn(1, generator=g), q2=torch.randn(I, A, generator=g) if with_q2 else None)
    return d


def _run_scan(d, n, grouped, planes=False):
    """One content-style scan launch: grouped on the per-image tensors, or plain on the expanded ones."""
    D = dev()
    B, A = d['q'].shape
    R = d['P'].shape[1]
    P, V, q2 = (d['P'], d['V'], d['q2']) if grouped else (rep(d['P'], n), rep(d['V'], n), rep(d['q2'], n))
    out, alpha = torch.full((B, A), 7.0, device=D), torch.full((B, R), 7.0, device=D)
    pl = torch.zeros(2, B, A, dtype=torch.float16, device=D) if planes else None
    t = [x.to(D) for x in (P, V, d['q'], d['w'], d['wb'])] + [None if q2 is None else q2.to(D)]     # alive past the launch
    pr = ops.scan_problem(t[0], t[1], t[2], t[3], t[4], out, alpha, q2=t[5], out_planes=pl, row_div=n if grouped else 1)
    ops.attn_scan_fwd([pr], B)
    torch.cuda.synchronize()
    return out, alpha, pl


def _fp64(d, n):
    P, V = rep(d['P'], n).double(), rep(d['V'], n).double()
    x = P + d['q'].double().unsqueeze(1)
    if d['q2'] is not None:
        x = x + rep(d['q2'], n).double().unsqueeze(1)
    e = (torch.tanh(x) @ d['w'].double().t()).squeeze(-1) + d['wb'].double()
    al = torch.softmax(e, dim=-1)
    return torch.bmm(al.unsqueeze(1), V).squeeze(1), al


SCAN_SHAPES = [(3, 2, 6, 32), (4, 5, 36, 512), (2, 8, 196, 512), (3, 11, 11, 512), (1, 3, 1, 64), (2, 4, 7, 1024)]


@pytest.mark.parametrize('I,n,R,A', SCAN_SHAPES)
def test_grouped_scan_is_the_plain_scan_on_expanded_inputs_bit_for_bit(I, n, R, A):
    d = _scan_case(I, n, R, A, seed=I * 1000 + n * 100 + R, with_q2=(R % 2 == 1))
    planes = (I, n, R, A) == (4, 5, 36, 512)                 # the out_hi / out_lo planes once
    g_out, g_alpha, g_pl = _run_scan(d, n, True, planes)
    p_out, p_alpha, p_pl = _run_scan(d, n, False, planes)
    assert torch.equal(g_alpha, p_alpha)
    assert torch.equal(g_out, p_out)
    if planes:
        assert torch.equal(g_pl, p_pl) and bool((g_pl != 0).any())
    ref_out, ref_alpha = _fp64(d, n)
    np.testing.assert_allclose(g_alpha.cpu().numpy(), ref_alpha.float().numpy(), atol=2e-6)
    np.testing.assert_allclose(g_out.cpu().numpy(), ref_out.float().numpy(), atol=1e-5)


def test_grouped_two_problem_launch_with_gathered_sentiment_words():
    """Content scan + sentiment scan in gather mode (a [50, .] table pair, Mw = 4 ids and the label term per image) as
    ONE launch, grouped against plain-on-expanded."""
    D = dev()
    I, n, R, A, Mw, NT = 3, 5, 9, 64, 4, 50
    g = torch.Generator().manual_seed(77)
    c = _scan_case(I, n, R, A, seed=78)
    tabP, tabV = torch.randn(NT, A, generator=g).to(D), torch.randn(NT, A, generator=g).to(D)
    ids = torch.randint(0, NT, (I, Mw), generator=g)
    qw, q2 = torch.randn(I * n, A, generator=g), torch.randn(I, A, generator=g)
    w2, wb2 = (torch.randn(1, A, generator=g) * 0.3).to(D), torch.randn(1, generator=g).to(D)
    B = I * n
    res = {}
    for grouped in (True, False):
        f = (lambda x: x) if grouped else (lambda x: rep(x, n))
        v, ac = torch.empty(B, A, device=D), torch.empty(B, R, device=D)
        s, as_ = torch.empty(B, A, device=D), torch.empty(B, Mw, device=D)
        k = n if grouped else 1
        t = [x.to(D) for x in (f(c['P']), f(c['V']), c['q'], c['w'], c['wb'], qw, f(q2), f(ids))]   # alive past the launch
        probs = [ops.scan_problem(t[0], t[1], t[2], t[3], t[4], v, ac, row_div=k),
                 ops.scan_problem(tabP, tabV, t[5], w2, wb2, s, as_, q2=t[6], row_ids=t[7], row_div=k)]
        ops.attn_scan_fwd(probs, B)
        torch.cuda.synchronize()
        res[grouped] = (v, ac, s, as_)
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
    # the maths of the gathered problem (fp64)
    idr = rep(ids, n)
    d2 = dict(P=tabP.cpu()[idr], V=tabV.cpu()[idr], q=qw, w=w2.cpu(), wb=wb2.cpu(), q2=rep(q2, n))
    ref_out, ref_alpha = _fp64(d2, 1)
    np.testing.assert_allclose(res[True][3].cpu().numpy(), ref_alpha.float().numpy(), atol=2e-6)
    np.testing.assert_allclose(res[True][2].cpu().numpy(), ref_out.float().numpy(), atol=1e-5)


def test_grouped_scan_above_the_non_temporal_threshold():
    """I = 1024 images x 36 x (512 + 512) x 4 B = 151 MB per image set: over the 128 MB rule counted per IMAGE."""
    D = dev()
    I, n, R, A = 1024, 2, 36, 512
    g = torch.Generator(device=D).manual_seed(3)
    P, V = torch.randn(I, R, A, device=D, generator=g), torch.randn(I, R, A, device=D, generator=g)
    q = torch.randn(I * n, A, device=D, generator=g)
    w, wb = torch.randn(1, A, device=D, generator=g) * 0.3, torch.randn(1, device=D, generator=g)
    outs = []
    for grouped in (True, False):
        out, alpha = torch.empty(I * n, A, device=D), torch.empty(I * n, R, device=D)
        Pe, Ve = (P, V) if grouped else (rep(P, n), rep(V, n))
        ops.attn_scan_fwd([ops.scan_problem(Pe, Ve, q, w, wb, out, alpha, row_div=n if grouped else 1)], I * n)
        torch.cuda.synchronize()
        outs.append((out, alpha))
        del Pe, Ve
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ----------------------------------------------------------------------------- 2. the LSTM's per-image term
@pytest.mark.parametrize('with_tab', [False, True], ids=['pre', 'pre_tab'])
@pytest.mark.parametrize('mode', [2, 0], ids=['split_f16', 'exact_fp32'])
@pytest.mark.parametrize('M,H,n', [(6, 32, 3), (65, 512, 5), (300, 512, 4)])
def test_lstm_pre_div_is_the_expanded_pre_bit_for_bit(M, H, n, mode, with_tab):
    D = dev()
    g = torch.Generator().manual_seed(M * 7 + H)
    ks = (H, H)
    xs = [torch.randn(M, k, generator=g).to(D) for k in ks]
    ws = [(torch.randn(4 * H, k, generator=g) * (3 * k) ** -0.5).to(D) for k in ks]
    c0 = torch.randn(M, H, generator=g).to(D)
    pre = (torch.randn(M // n, 4 * H, generator=g) * 0.3).to(D)
    kw = {}
    if with_tab:
        kw['tab'] = (torch.randn(50, 4 * H, generator=g) * 0.3).to(D)
        kw['tab_ids'] = torch.randint(0, 50, (M,), generator=g).to(D)
    ops.set_h3_mode(mode)
    res = []
    for grouped in (True, False):
        h, c = torch.full((M, H), 7.0, device=D), torch.full((M, H), 7.0, device=D)
        planes = torch.zeros(2, M, H, dtype=torch.float16, device=D)
        ops.lstm_fwd(list(zip(xs, ws)), None, None, c0, h, c, pre=pre if grouped else rep(pre, n), h_planes=planes,
                     pre_div=n if grouped else 1, **kw)
        torch.cuda.synchronize()
        res.append((h, c, planes))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # the maths (fp64), at the tolerance of tests/test_gpu_h3.py::test_lstm_h3
    z = sum(x.double().cpu() @ w.double().cpu().t() for x, w in zip(xs, ws)) + rep(pre, n).double().cpu()
    if with_tab:
        z = z + kw['tab'].double().cpu()[kw['tab_ids'].cpu()]
    i, f, gg, o = z.split(H, dim=1)
    c_ref = torch.sigmoid(f) * c0.double().cpu() + torch.sigmoid(i) * torch.tanh(gg)
    h_ref = torch.sigmoid(o) * torch.tanh(c_ref)
    np.testing.assert_allclose(res[0][0].cpu().numpy(), h_ref.float().numpy(), atol=2e-5)
    np.testing.assert_allclose(res[0][1].cpu().numpy(), c_ref.float().numpy(), atol=2e-5)


# ----------------------------------------------------------------------------- 3. / 4. roll-outs against the repeated call
_CAPS = {}


def make_captioner(name):
    if name not in _CAPS:
        c, st, w, d, s2s = case_setup(name)
        cap = Captioner(synth.make_idx2word(c['V']), synth.SENTIMENT_CATEGORIES, st)
        cap.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
        cap.to(dev()).eval()
        _CAPS[name] = (cap, c, st, w)
    cap = _CAPS[name][0]
    cap.rows_step = True
    return _CAPS[name]


def inputs(c, st, B, T, seed, regions=None):
    d = synth.make_inputs(B, c['V'], st, regions=regions or c['R'], seq_len=T, seed=seed)
    return [torch.from_numpy(np.asarray(d[k])).to(dev())
            for k in ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')]


def _weights(cap):
    return [x.clone() for x in (cap.cont_weights, cap.senti_weights, cap.cont_senti_weights)]


def _both_forms(cap, a, n, T, **kw):
    """(grouped, repeated): the three returned tensors + the three attention-weight attributes of each form."""
    with torch.no_grad():
        g = list(cap.forward_rl(*a, T, 0, captions_per_image=n, **kw))
        assert cap.fc_feats.shape[0] == a[0].shape[0] and cap.cpt_feats.shape[0] == a[0].shape[0]
        g += _weights(cap)
        r = list(cap.forward_rl(*[rep(x, n) for x in a], T, 0, **kw))
        assert cap.fc_feats.shape[0] == a[0].shape[0] * n
        r += _weights(cap)
    return g, r


def _assert_replay_forms_agree(g, r, B, T):
    names = ('seq', 'seq_logprobs', 'seq_masks', 'cont_weights', 'senti_weights', 'cont_senti_weights')
    for name, x, y in zip(names, g, r):
        assert x.shape == y.shape and x.shape[0] == B, name
        err = 0.0 if x.dtype == torch.int64 else float((x - y).abs().max())
        print('%-20s max |grouped - repeated| = %.3e%s' % (name, err, '' if not torch.equal(x, y) else '  (bit-identical)'))
    assert torch.equal(g[0], r[0]) and torch.equal(g[2], r[2])
    assert float((g[1] - r[1]).abs().max()) <= LOGP_TOL
    for x, y in zip(g[3:], r[3:]):
        np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), atol=W_TOL)


@pytest.mark.parametrize('I,n,rows_step', [(5, 3, True), (2, 3, True), (2, 3, False)],
                         ids=['15_rows', '6_rows_rows_step_on', '6_rows_rows_step_off'])
def test_tiny_grouped_rollout_is_the_repeated_rollout(I, n, rows_step):
    cap, c, st, w = make_captioner('tiny')
    cap.rows_step = rows_step
    T = 8
    a = inputs(c, st, I, T, 41)
    B = I * n
    # forced tokens: every row of the two forms is fed the same words
    tok = torch.randint(4, c['V'], (B, T), generator=torch.Generator().manual_seed(5)).to(dev())
    g, r = _both_forms(cap, a, n, T, _replay=tok)
    _assert_replay_forms_agree(g, r, B, T)
    # drawn tokens under the sampling controls, same uniforms
    u = torch.rand(B, T, generator=torch.Generator().manual_seed(8)).to(dev())
    kw = dict(temperature=1.3, top_k=20, top_p=0.95, return_sampling_logprobs=True)
    with torch.no_grad():
        gs = cap.forward_rl(*a, T, 0, _uniforms=u, captions_per_image=n, **kw)
        rs = cap.forward_rl(*[rep(x, n) for x in a], T, 0, _uniforms=u, **kw)
    assert len(gs) == 4 and gs[3].shape == (B, T)
    assert torch.equal(gs[0], rs[0]) and torch.equal(gs[2], rs[2])
    assert float((gs[1] - rs[1]).abs().max()) <= LOGP_TOL and float((gs[3] - rs[3]).abs().max()) <= LOGP_TOL
    seq = gs[0].cpu().view(I, n, T)
    assert any(len({tuple(x) for x in seq[i].tolist()}) > 1 for i in range(I))       # the n draws of an image differ


@pytest.mark.parametrize('form', ['fp32', 'float16_features', 'exact_fp32_engine'])
def test_full_size_grouped_rollout_is_the_repeated_rollout(form):
    cap, c, st, w = make_captioner('cfg1')
    I, n, T = 13, 5, 6
    a = inputs(c, st, I, T, 42)
    if form == 'float16_features':
        a[0], a[1] = a[0].half(), a[1].half()
    if form == 'exact_fp32_engine':
        ops.set_h3_mode(0)
    tok = torch.randint(4, c['V'], (I * n, T), generator=torch.Generator().manual_seed(6)).to(dev())
    g, r = _both_forms(cap, a, n, T, _replay=tok)
    _assert_replay_forms_agree(g, r, I * n, T)


def test_generator_and_default_controls_compose_with_captions_per_image():
    cap, c, st, w = make_captioner('tiny')
    I, n, T = 4, 3, 8
    a = inputs(c, st, I, T, 43)
    gen = torch.Generator(device=dev())
    with torch.no_grad():
        gen.manual_seed(11)
        g = cap.forward_rl(*a, T, 0, generator=gen, captions_per_image=n)
        gen.manual_seed(11)
        r = cap.forward_rl(*[rep(x, n) for x in a], T, 0, generator=gen)
    assert g[0].shape == (I * n, T) and torch.equal(g[0], r[0]) and torch.equal(g[2], r[2])
    assert float((g[1] - r[1]).abs().max()) <= LOGP_TOL


# ----------------------------------------------------------------------------- 5. against the oracle
def test_grouped_rollout_against_the_oracle():
    """The raw tokens of a grouped sampled roll-out fed to the CPU oracle on the REPEATED inputs: seq_logprobs is the
    oracle's log-probability of every drawn token (1e-4), masks and fed tokens follow from the raw tokens."""
    from oracle import captioner_oracle as O
    cap, c, st, w = make_captioner('tiny')
    I, n, T = 4, 3, 8
    B = I * n
    a = inputs(c, st, I, T, 44)
    u = torch.rand(B, T, generator=torch.Generator().manual_seed(19))
    filt = cap._sample_filter(1.3, 10, 0.95, uniforms=u.to(dev()))
    with torch.no_grad():
        seq, lp, mk, raw, alive = cap._rollout(*a, T, 0, None, None, filt, group=n)
    assert seq.shape == (B, T)
    seq, lp, mk, raw = seq.cpu(), lp.cpu().numpy(), mk.cpu().numpy(), raw.cpu()
    prm = O.to_params(w)
    oid = O.Ids(synth.make_idx2word(c['V']), synth.SENTIMENT_CATEGORIES)
    ca = [rep(x.cpu(), n) for x in a]
    with torch.no_grad():
        P = O.prologue(prm, oid, 'rl', *ca, None, 0.5)
        state = O.init_state(prm, B)
        it = torch.full((B,), oid.sos, dtype=torch.long)
        unf = torch.ones(B, dtype=torch.bool)
        for t in range(T):
            logp, state, _ = O.step(prm, it, state, P.fc_e, P.att_e, P.p_att, P.words_e, P.p_words, P.label_e, None, 0.5)
            want = logp.double().numpy()[np.arange(B), raw[:, t].numpy()]
            print('step %d: max |seq_logprobs - oracle| = %.2e' % (t, np.abs(lp[:, t] - want).max()))
            np.testing.assert_allclose(lp[:, t], want, atol=1e-4)
            assert (mk[:, t] == unf.numpy()).all()
            it = raw[:, t] * unf.long()
            assert (seq[:, t] == it).all()
            unf = unf & (it != oid.eos)
            if not unf.any():
                break


# ----------------------------------------------------------------------------- 6. sample_captions(share_image=True)
def test_sample_captions_share_image_returns_the_repeated_forms_captions():
    cap, c, st, w = make_captioner('tiny')
    I, n, T = 5, 3, 8
    a = inputs(c, st, I, T, 35)
    u = torch.rand(I * n, T, generator=torch.Generator().manual_seed(8)).to(dev())
    kw = dict(temperature=1.3, top_k=20, top_p=0.95)
    rep_caps, rep_ids = cap.sample_captions(*a, n=n, max_seq_len=T, _uniforms=u, **kw)
    assert cap.fc_feats.shape[0] == I * n
    caps, ids = cap.sample_captions(*a, n=n, max_seq_len=T, _uniforms=u, share_image=True, **kw)
    assert cap.fc_feats.shape[0] == I
    assert ids == rep_ids and caps == rep_caps
    assert len(caps) == I and all(len(x) == n for x in caps)
