"""Temperature / top-k / top-p in the device roll-out (isc_rollout_finalize_filtered, Captioner.forward_rl's sampling
controls, Captioner.sample_captions) against the fp64 reference sampler of tests/_sample_filter_ref.py.

Bars: 2e-6 on a normalised cumulative mass and 2e-5 on a log-probability - the project's own for fp32 mass sums
(tests/test_gpu_sampling.py) -, 1e-4 on a log-probability against the oracle (tests/test_gpu_parity.py)."""
import numpy as np
import pytest
import torch

import _sample_filter_ref as ref
from conftest import case_setup
from insenticap_model_amd import Captioner, _lib, ops, synth

pytestmark = pytest.mark.gpu

LP_TOL = 2e-5
XT_SENTINEL = -12345.0
PARAMS = [(1.0, 0, 0.9), (0.7, 0, 0.95), (1.5, 0, 0.5), (1.3, 50, 0.9), (2.0, 640, 0.99), (1.0, 5, 1.0), (0.8, 0, 1.0)]


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


class Rows:
    """Logits on the device WITH the tile statistics that describe them (the identity trick of
    tests/test_gpu_sampling.py::_sample: the vocabulary kernel with h = I and W^T = logits), and the buffers of one
    roll-out of T steps over them.  xt: the step also writes xt_next [B, W] = relu(emb[fed token]) (+ xt_add when
    `xt_add`) from a random embedding table; one more row of sentinels lies behind xt_next."""

    def __init__(self, logits, T=1, eos_id=2, W=32, xt=False, xt_add=False):
        D = dev()
        B, V = logits.shape
        self.B, self.V, self.T, self.W = B, V, T, W
        nt = (V + 127) // 128
        self.pm, self.ps = torch.empty(B, nt, device=D), torch.empty(B, nt, device=D)
        self.pi = torch.empty(B, nt, device=D, dtype=torch.int32)
        K = ((B + 31) // 32) * 32
        h = torch.zeros(B, K, device=D)
        h[torch.arange(B), torch.arange(B)] = 1.0
        Wm = torch.zeros(V, K, device=D)
        Wm[:, :B] = logits.to(D).t()
        self.out = torch.empty(B, V, device=D)
        ops.vocab_fwd(h, Wm, torch.zeros(V, device=D), self.pm, self.ps, self.pi, self.out)
        self.seq = torch.zeros(B, T, dtype=torch.int64, device=D)
        self.raw = torch.zeros(B, T, dtype=torch.int64, device=D)
        self.lp, self.mk, self.slp = (torch.zeros(B, T, device=D) for _ in range(3))
        self.unf = torch.ones(B, dtype=torch.int32, device=D)
        self.alive = torch.zeros(T + 1, dtype=torch.int32, device=D)
        self.alive[0] = B
        g = torch.Generator().manual_seed(V + W)
        self.emb = torch.randn(V, W, generator=g).to(D) if xt else torch.zeros(V, W, device=D)
        self.add = torch.randn(B, W, generator=g).to(D) if xt and xt_add else None
        self.xt = torch.full((B + 1, W), XT_SENTINEL, device=D) if xt else None
        self.eos_id = eos_id
        self.x = self.out.cpu().double().numpy()

    def step(self, t, u, tau, k, p):
        st = _lib.RolloutStep()
        st.B, st.V, st.T, st.t, st.n_tile, st.W = self.B, self.V, self.T, t, self.pm.shape[1], self.W
        self.uu = u.to(dev()).float().view(self.B, self.T).contiguous()
        st.part_max, st.part_sum, st.part_idx = self.pm.data_ptr(), self.ps.data_ptr(), self.pi.data_ptr()
        st.logits, st.ld_logits = self.out.data_ptr(), self.out.stride(0)
        st.forced, st.sample_u, st.eos_id = None, self.uu.data_ptr(), self.eos_id
        st.seq, st.seq_logprobs, st.seq_masks = self.seq.data_ptr(), self.lp.data_ptr(), self.mk.data_ptr()
        st.unfinished, st.alive, st.raw_tokens = self.unf.data_ptr(), self.alive.data_ptr(), self.raw.data_ptr()
        st.emb, st.xt_add, st.xt_next = self.emb.data_ptr(), ops.ptr(self.add), ops.ptr(self.xt)
        ops.rollout_finalize_filtered(st, tau, k, p, self.slp)
        torch.cuda.synchronize()

    def draw(self, u, tau, k, p):
        """One step on fresh roll-out state: (tokens, seq_logprobs, sampling_logprobs)."""
        self.unf.fill_(1)
        self.alive.zero_()
        self.alive[0:1].fill_(self.B)
        self.step(0, u, tau, k, p)
        return self.raw[:, 0].cpu().numpy(), self.lp[:, 0].cpu().numpy(), self.slp[:, 0].cpu().numpy()


def xt_next_case(cls, B, W, xt_add, V=130, T=3, eos_id=2):
    """Rows (or a subclass) for one step t = 1 of T = 3 that writes xt_next: random logits, row 1 finished, every [B, T]
    output filled with a sentinel."""
    g = torch.Generator().manual_seed(B * 3 + W)
    rows = cls(4.0 * torch.randn(B, V, generator=g), T=T, eos_id=eos_id, W=W, xt=True, xt_add=xt_add)
    rows.alive[0:2].fill_(B)
    rows.unf[1] = 0
    rows.seq.fill_(-7)
    rows.raw.fill_(-7)
    for o in (rows.lp, rows.mk, rows.slp):
        o.fill_(XT_SENTINEL)
    return rows, torch.rand(B, T, generator=g)


def assert_xt_next(rows, t=1):
    """xt_next = relu(emb[seq[:, t]]) (+ xt_add) under torch.equal: one max and at most one IEEE add in float32, nothing
    to round differently.  The finished row 1 feeds <PAD>, whose embedding row is what it gets; the row behind xt_next and
    the other columns of the [B, T] outputs keep their sentinels."""
    B = rows.B
    seq = rows.seq.cpu()
    assert int(seq[1, t]) == 0 and float(rows.mk[1, t]) == 0.0 and int(rows.unf[1]) == 0
    assert bool(((seq[:, t] >= 0) & (seq[:, t] < rows.V)).all())
    live = torch.ones(B, dtype=torch.bool)
    live[1] = False
    assert torch.equal(seq[live, t], rows.raw.cpu()[live, t]) and bool((rows.mk.cpu()[live, t] == 1.0).all())
    want = rows.emb.cpu()[seq[:, t]].clamp_min(0.0)
    assert bool((want[1] > 0).any())                    # (<PAD>'s row is not all zero: a skipped row would show)
    if rows.add is not None:
        want = want + rows.add.cpu()
    assert torch.equal(rows.xt[:B].cpu(), want)
    assert bool((rows.xt[B] == XT_SENTINEL).all())
    others = [c for c in range(rows.T) if c != t]
    assert bool((rows.seq[:, others] == -7).all()) and bool((rows.raw[:, others] == -7).all())
    assert all(bool((o[:, others] == XT_SENTINEL).all()) for o in (rows.lp, rows.mk))


@pytest.mark.parametrize('B,W,xt_add', [(6, 4, True), (1030, 4, True), (6, 1028, False)])
def test_filtered_finalize_writes_xt_next(B, W, xt_add):
    """The commit stage behind the filtered selection, 256 threads per row: B = 1030 is a workgroup's second row trip
    (768 workgroups), W = 1028 the second trip of the 256-thread float4 loop (257 float4s per row)."""
    rows, u = xt_next_case(Rows, B, W, xt_add)
    rows.step(1, u, 0.8, 50, 0.9)
    assert_xt_next(rows)
    assert int(rows.alive[2]) == int(rows.unf.sum())


_ROWS = {}


def _case_rows(V):
    if V not in _ROWS:
        _ROWS.clear()                                # (one [512, V] case resident at a time)
        g = torch.Generator().manual_seed(V)
        logits = 4.0 * torch.randn(512, V, generator=g)
        u = torch.rand(512, generator=g)
        u[:4] = torch.tensor([0.0, 1e-9, 0.999999, 0.5])
        rows = Rows(logits)
        _ROWS[V] = (rows, u, ref.ranking(rows.x))
    return _ROWS[V]


def _check_against_reference(rows, u, orders, tau, k, p, relaxed_cap=0.03, exact_bar=0.98):
    B = rows.B
    un = u.double().numpy()
    checks = [ref.RowCheck(rows.x[b], un[b], tau, k, p, orders[b]) for b in range(B)]
    strict = np.array([c.strict for c in checks])
    # a condition on the inputs, asserted on the reference alone, before the device is looked at
    gap = max(c.n_hi - c.n_lo for c in checks)
    print('tau=%g k=%d p=%g V=%d: relaxed rows %.2f %% (cap %.0f %%), widest K-/K+ gap %d' % (
        tau, k, p, rows.V, 100.0 * (1 - strict.mean()), 100 * relaxed_cap, gap))
    assert (1 - strict.mean()) <= relaxed_cap and gap <= 1
    if p >= 1.0:
        assert strict.all()
    tok, lp, slp = rows.draw(u, tau, k, p)
    assert ((tok >= 0) & (tok < rows.V)).all()
    ok = np.array([c.token_ok(t) for c, t in zip(checks, tok)])
    ref_tok = np.array([c.ref_token() for c in checks])
    near = np.mean([c.near_boundary() for c in checks])
    agree = (tok == ref_tok)[strict].mean()
    x = torch.from_numpy(rows.x)
    lp_ref = torch.log_softmax(x, 1).numpy()[np.arange(B), tok]
    lp_err = np.abs(lp - lp_ref).max()
    slp_ref = np.array([c.sampling_logprob(t) if s else np.nan for c, t, s in zip(checks, tok, strict)], dtype=np.float64)
    in_K = ~np.isnan(slp_ref) | ~strict
    slp_err = np.nanmax(np.abs(slp - slp_ref)) if strict.any() else 0.0
    print('   interval check ok on %d / %d rows; exact agreement on strict rows %.2f %% (reference rows within 2e-6 of a '
          'boundary: %.2f %%); max |seq_logprob - ref| %.2e, max |sampling_logprob - ref| %.2e' % (
              ok.sum(), B, 100 * agree, 100 * near, lp_err, slp_err))
    assert ok.all(), np.nonzero(~ok)[0][:10]
    assert in_K.all()                                 # strict rows: the token lies in the reference's kept set
    assert agree >= exact_bar
    assert lp_err <= LP_TOL
    assert slp_err <= LP_TOL
    return tok


@pytest.mark.parametrize('tau,k,p', PARAMS)
@pytest.mark.parametrize('V', [130, 10000, 20000])
def test_filtered_draw_matches_fp64_reference(V, tau, k, p):
    rows, u, orders = _case_rows(V)
    tok = _check_against_reference(rows, u, orders, tau, k, p)
    if p >= 1.0 and 0 < k < V:                        # top-k alone: every token in the exact top-k set
        assert all(t in set(orders[b][:k].tolist()) for b, t in enumerate(tok))
    # bit-repeatable: the same inputs give the same tokens and the same log-probabilities
    a = rows.draw(u, tau, k, p)
    b = rows.draw(u, tau, k, p)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[0], tok)


@pytest.mark.parametrize('tau,k,p', [(1.0, 300, 1.0), (0.9, 0, 0.8), (1.0, 40, 0.7), (1.0, 1, 1.0), (2.0, 999, 0.999)])
def test_rows_of_tied_logits(tau, k, p):
    """Logits rounded to a few integers (and one constant row): hundreds of equal values fall into the bucket that holds
    the boundary, so the selection resolves it by the bits of (value, id) - ties go to the smaller id."""
    g = torch.Generator().manual_seed(77)
    V, B = 1000, 96
    logits = torch.round(1.2 * torch.randn(B, V, generator=g))
    logits[0] = 0.5
    logits[1] = -3.0
    logits[1, 700] = -2.0
    rows = Rows(logits)
    u = torch.rand(B, generator=g)
    # (equal masses put many cumulative sums exactly ON a multiple of the mass: a boundary within 2e-6 of top_p is a
    # property of such inputs, so the cap on relaxed rows does not apply here; every row still has to pass its check)
    tok = _check_against_reference(rows, u, ref.ranking(rows.x), tau, k, p, relaxed_cap=1.0, exact_bar=0.98)
    if k == 1:
        assert (tok == rows.x.argmax(1)).all() and tok[0] == 0 and tok[1] == 700


def test_finished_rows_and_skipped_steps_at_kernel_level():
    """<EOS> ends a row: from the next step on it is masked and writes <PAD>; once no row is alive a step writes nothing."""
    V, B, T, eos = 130, 40, 3, 2
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(B, V, generator=g)
    logits[:, eos] = -30.0
    logits[::2, eos] = 30.0                           # even rows draw <EOS> at once, odd rows never
    rows = Rows(logits, T=T, eos_id=eos)
    u = torch.rand(B, T, generator=g)
    for t in range(T):
        rows.step(t, u, 0.9, 20, 0.95)
    seq, mk, raw, alive = rows.seq.cpu().numpy(), rows.mk.cpu().numpy(), rows.raw.cpu().numpy(), rows.alive.cpu().numpy()
    assert (raw[::2] == eos).all() and (raw[1::2] != eos).all()
    assert (seq[::2, 0] == eos).all() and (seq[::2, 1:] == 0).all() and (mk[::2] == [1, 0, 0]).all()
    assert (seq[1::2] == raw[1::2]).all() and (mk[1::2] == 1).all()
    assert alive.tolist() == [B, B // 2, B // 2, B // 2]
    assert rows.unf.cpu().numpy().tolist() == [0, 1] * (B // 2)
    # every row ends at step 0: steps 1, 2 must leave their (pre-filled) outputs alone
    logits[:, eos] = 30.0
    rows = Rows(logits, T=T, eos_id=eos)
    rows.lp.fill_(7.0)
    rows.seq.fill_(-1)
    for t in range(T):
        rows.step(t, u, 1.4, 0, 0.9)
    assert rows.alive.cpu().numpy().tolist() == [B, 0, 0, 0]
    assert (rows.seq[:, 0] == eos).all() and (rows.seq[:, 1:] == -1).all()
    assert (rows.lp[:, 1:] == 7.0).all() and (rows.lp[:, 0] != 7.0).all() and (rows.mk[:, 1:] == 0).all()


@pytest.mark.parametrize('tau,k,p', [(0.8, 0, 0.9), (1.2, 40, 1.0)])
def test_frequencies_follow_the_filtered_distribution(tau, k, p):
    g = torch.Generator().manual_seed(3)
    V, B = 300, 4096
    row = torch.randn(V, generator=g) * 1.5
    rows = Rows(row.repeat(B, 1))
    counts = np.zeros(V)
    for rep in range(4):
        tok, _, _ = rows.draw(torch.rand(B, generator=g), tau, k, p)
        counts += np.bincount(tok, minlength=V)
    x = rows.x[0]
    kept = ref.kept_set(x, tau, k, p)
    pr = np.zeros(V)
    pr[kept] = ref.masses(x, tau)[kept]
    pr /= pr.sum()
    n = counts.sum()
    outside = np.ones(V, dtype=bool)
    outside[kept] = False
    assert counts[outside].sum() == 0                 # no token outside the kept set is ever drawn
    z = ((counts - n * pr) / np.sqrt(n * pr * (1 - pr) + 1e-12))[kept]
    print('kept %d of %d tokens; max |z| %.2f, mean |z| over expected counts > 20: %.2f' % (
        len(kept), V, np.abs(z).max(), np.abs(z[(pr * n)[kept] > 20]).mean()))
    assert np.abs(z).max() < 5.5 and np.abs(z[(pr * n)[kept] > 20]).mean() < 1.2


# ----------------------------------------------------------------------------- through the public API
def make_captioner(name):
    c, st, w, d, s2s = case_setup(name)
    cap = Captioner(synth.make_idx2word(c['V']), synth.SENTIMENT_CATEGORIES, st)
    cap.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    cap.to(dev()).eval()
    return cap, c, st, w, d


def inputs(c, st, B, T, seed):
    d = synth.make_inputs(B, c['V'], st, regions=c['R'], seq_len=T, seed=seed)
    return [torch.from_numpy(np.asarray(d[k])).to(dev())
            for k in ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')]


GEOMS = [('tiny', 48, 8), ('cfg1', 160, 12)]


@pytest.mark.parametrize('name,B,T', GEOMS)
def test_top_k_1_is_the_greedy_rollout(name, B, T):
    cap, c, st, w, _ = make_captioner(name)
    cap.rows_step = False                             # both calls on the general step kernels: the same logits
    cap.enable_rollout_graphs(False)
    a = inputs(c, st, B, T, 31)
    with torch.no_grad():
        gs, glp, gm = cap.forward_rl(*a, T, 1)
        for seed in (0, 9):
            torch.manual_seed(seed)
            s, lp, m, slp = cap.forward_rl(*a, T, 0, top_k=1, temperature=1.7, return_sampling_logprobs=True)
            assert torch.equal(s, gs) and torch.equal(m, gm)
            assert (lp - glp).abs().max().item() <= LP_TOL
            assert slp.abs().max().item() <= LP_TOL           # one survivor: probability 1


@pytest.mark.parametrize('name,B,T', GEOMS)
def test_default_controls_take_todays_path(name, B, T):
    cap, c, st, w, _ = make_captioner(name)
    a = inputs(c, st, B, T, 32)
    with torch.no_grad():
        torch.manual_seed(4)
        plain = cap.forward_rl(*a, T, 0)
        torch.manual_seed(4)
        spelt = cap.forward_rl(*a, T, 0, temperature=1.0, top_k=0, top_p=1.0, generator=None,
                               return_sampling_logprobs=False, _uniforms=None)
        torch.manual_seed(4)
        wide = cap.forward_rl(*a, T, 0, top_k=c['V'], top_p=1.5, return_sampling_logprobs=True)
    assert len(plain) == len(spelt) == 3 and len(wide) == 4
    for x, y, z in zip(plain, spelt, wide):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert torch.equal(wide[3], plain[1])             # nothing filtered: the sampled distribution is the model's


@pytest.mark.parametrize('name,B,T', GEOMS)
def test_uniforms_hook_generator_and_repeatability(name, B, T):
    cap, c, st, w, _ = make_captioner(name)
    a = inputs(c, st, B, T, 33)
    kw = dict(temperature=0.8, top_k=30, top_p=0.9, return_sampling_logprobs=True)
    g = torch.Generator(device=dev())
    g.manual_seed(123)
    u = torch.rand(B, T, device=dev(), generator=g)
    with torch.no_grad():
        r1 = cap.forward_rl(*a, T, 0, _uniforms=u, **kw)
        r2 = cap.forward_rl(*a, T, 0, _uniforms=u.clone(), **kw)
        g.manual_seed(123)
        r3 = cap.forward_rl(*a, T, 0, generator=g, **kw)
        r4 = cap.forward_rl(*a, T, 0, _uniforms=torch.rand(B, T, device=dev()), **kw)
        with pytest.raises(ValueError):
            cap.forward_rl(*a, T, 0, _uniforms=u[:, :-1], **kw)
    for x, y, z in zip(r1, r2, r3):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert not torch.equal(r1[0], r4[0])
    live = r1[2].bool()
    assert (r1[3][live] <= 1e-6).all() and torch.isfinite(r1[3]).all() and (r1[3][live] != r1[1][live]).any()


def test_finished_rows_through_the_api():
    """Masks, <PAD> feeding and the `alive` counters are what the raw tokens imply."""
    cap, c, st, w, _ = make_captioner('tiny')
    B, T = 64, 16
    a = inputs(c, st, B, T, 34)
    torch.manual_seed(2)
    filt = cap._sample_filter(3.0, 0, 0.98)           # flat distribution over V = 64: <EOS> comes up
    with torch.no_grad():
        seq, lp, mk, raw, alive = cap._rollout(*a, T, 0, None, None, filt)
    seq, mk, raw, alive = seq.cpu().numpy(), mk.cpu().numpy(), raw.cpu().numpy(), alive.cpu().numpy()
    unf = np.ones(B, dtype=bool)
    steps = 0
    for t in range(T):
        assert alive[t] == unf.sum(), t
        if not unf.any():
            break
        steps += 1
        assert (mk[:, t] == unf).all() and (seq[:, t] == raw[:, t] * unf).all(), t
        unf = unf & (seq[:, t] != cap.eos_id)
    assert (seq[:, steps:] == 0).all() and (mk[:, steps:] == 0).all() and (lp.cpu().numpy()[:, steps:] == 0).all()
    assert (mk.sum(1) < T).any()                      # some row did end early


def test_sample_captions_are_the_repeated_rows_of_forward_rl():
    cap, c, st, w, _ = make_captioner('tiny')
    I, n, T = 5, 3, 8
    a = inputs(c, st, I, T, 35)
    u = torch.rand(I * n, T, generator=torch.Generator().manual_seed(8)).to(dev())
    kw = dict(temperature=1.3, top_k=20, top_p=0.95)
    caps, ids = cap.sample_captions(*a, n=n, max_seq_len=T, _uniforms=u, **kw)
    assert len(caps) == len(ids) == I and all(len(x) == n for x in caps) and all(len(x) == n for x in ids)
    with torch.no_grad():
        seq, _, mk = cap.forward_rl(*[x.repeat_interleave(n, 0) for x in a], T, 0, _uniforms=u, **kw)
    seq, ln = seq.cpu().tolist(), mk.sum(1).long().cpu().tolist()
    i2w = synth.make_idx2word(c['V'])
    for i in range(I):
        for j in range(n):
            words = seq[i * n + j][:ln[i * n + j]]
            assert ids[i][j] == words
            assert caps[i][j] == ' '.join(i2w[t] for t in words if t != cap.eos_id)
    assert len({tuple(x) for x in ids[0]}) > 1 or len({tuple(x) for x in ids[1]}) > 1     # the n draws differ
    g = torch.Generator(device=dev())
    g.manual_seed(5)
    c1 = cap.sample_captions(*a, n=n, max_seq_len=T, generator=g, **kw)
    g.manual_seed(5)
    c2 = cap.sample_captions(*a, n=n, max_seq_len=T, generator=g, **kw)
    assert c1 == c2


# ----------------------------------------------------------------------------- whole roll-out against the oracle
@pytest.mark.parametrize('tau,k,p', [(0.8, 0, 0.9), (1.3, 10, 0.95)])
def test_filtered_rollout_against_the_oracle(tau, k, p):
    """The device's raw tokens fed back into the CPU oracle give the full log-prob row of every (b, t): every token of a
    still-unfinished row passes the reference check against that row, and seq_logprobs is the oracle's (1e-4)."""
    from oracle import captioner_oracle as O
    cap, c, st, w, d = make_captioner('tiny')
    B, T = c['B'], c['T']
    a = [torch.from_numpy(np.asarray(d[k_])).to(dev())
         for k_ in ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')]
    u = torch.rand(B, T, generator=torch.Generator().manual_seed(19))
    filt = cap._sample_filter(tau, k, p, uniforms=u.to(dev()))
    with torch.no_grad():
        seq, lp, mk, raw, alive = cap._rollout(*a, T, 0, None, None, filt)
    seq, lp, mk, raw = seq.cpu(), lp.cpu().numpy(), mk.cpu().numpy(), raw.cpu()
    prm = O.to_params(w)
    oid = O.Ids(synth.make_idx2word(c['V']), synth.SENTIMENT_CATEGORIES)
    ca = [torch.from_numpy(np.asarray(d[k_])) for k_ in ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')]
    checked = 0
    with torch.no_grad():
        P = O.prologue(prm, oid, 'rl', *ca, None, 0.5)
        state = O.init_state(prm, B)
        it = torch.full((B,), oid.sos, dtype=torch.long)
        unf = torch.ones(B, dtype=torch.bool)
        for t in range(T):
            logp, state, _ = O.step(prm, it, state, P.fc_e, P.att_e, P.p_att, P.words_e, P.p_words, P.label_e, None, 0.5)
            rowlp = logp.double().numpy()
            for b in range(B):
                if unf[b]:
                    rc = ref.RowCheck(rowlp[b], float(u[b, t]), tau, k, p)
                    assert rc.token_ok(int(raw[b, t])), (b, t, int(raw[b, t]), rc.n_lo, rc.n, rc.n_hi)
                    checked += 1
            want = rowlp[np.arange(B), raw[:, t].numpy()]
            print('step %d: max |seq_logprobs - oracle| = %.2e' % (t, np.abs(lp[:, t] - want).max()))
            np.testing.assert_allclose(lp[:, t], want, atol=1e-4)
            assert (mk[:, t] == unf.numpy()).all()
            it = raw[:, t] * unf.long()
            assert (seq[:, t] == it).all()
            unf = unf & (it != oid.eos)
            if not unf.any():
                break
    assert checked >= B
