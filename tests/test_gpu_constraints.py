"""The beam search's token constraints in the device roll-out: isc_rollout_finalize_constrained at kernel level against the
fp64 reference of tests/_constraint_ref.py, and Captioner.forward_rl / sample_captions / the differentiable roll-out /
Detector.rollout_constraints on top of it - constrained greedy is the oracle's (and this build's) beam 1.

Bars (the project's own): the greedy token is exact; a drawn token lies in its CDF slot over the reduced row widened by
2e-6; 2e-5 on a log-probability at kernel level (tests/test_gpu_sample_filter.py), 1e-4 against the oracle
(tests/test_gpu_parity.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _constraint_ref as cref
from _constraint_ref import T, setup
from insenticap_model_amd import Captioner, _lib, ops, synth
from insenticap_model_amd.rewards import RewardCriterion
from oracle import captioner_oracle as O
from test_gpu_sample_filter import Rows, assert_xt_next, xt_next_case

pytestmark = pytest.mark.gpu

LP_TOL = 2e-5
ORACLE_TOL = 1e-4
EOS = 2
FILT = (0.8, 50, 0.9)


@pytest.fixture(autouse=True)
def _restore():
    yield
    ops.set_h3_mode(1)


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


# ----------------------------------------------------------------------------- kernel level
class CRows(Rows):
    """Rows of tests/test_gpu_sample_filter.py with the constrained entry point."""

    def cstep(self, t, u, cons, filt=None, greedy=False, forced=None, logits=True, call=True):
        st = _lib.RolloutStep()
        st.B, st.V, st.T, st.t, st.n_tile, st.W = self.B, self.V, self.T, t, self.pm.shape[1], self.W
        self.uu = u.to(dev()).float().view(self.B, self.T).contiguous()
        st.part_max, st.part_sum, st.part_idx = self.pm.data_ptr(), self.ps.data_ptr(), self.pi.data_ptr()
        st.logits, st.ld_logits = (self.out.data_ptr() if logits else None), self.out.stride(0)
        st.forced, st.sample_u, st.eos_id = ops.ptr(forced), (None if greedy else self.uu.data_ptr()), self.eos_id
        st.seq, st.seq_logprobs, st.seq_masks = self.seq.data_ptr(), self.lp.data_ptr(), self.mk.data_ptr()
        st.unfinished, st.alive, st.raw_tokens = self.unf.data_ptr(), self.alive.data_ptr(), self.raw.data_ptr()
        st.emb, st.xt_add, st.xt_next = self.emb.data_ptr(), ops.ptr(self.add), ops.ptr(self.xt)
        if not call:
            return st
        ops.rollout_finalize_constrained(st, cons, filt, self.slp if filt is not None else None)
        torch.cuda.synchronize()

    def fresh(self, prev=None):
        self.unf.fill_(1)
        self.alive.zero_()
        self.alive[0:2].fill_(self.B)
        self.seq.zero_()
        if prev is not None:
            self.seq[:, 0] = torch.as_tensor(prev).to(dev())

    def outputs(self, t):
        return self.raw[:, t].cpu().numpy(), self.lp[:, t].cpu().numpy(), self.slp[:, t].cpu().numpy()


def scenario(V, B):
    """One logits matrix that holds the edge cases by row group, its global ban list and the per-row previous tokens."""
    g = torch.Generator().manual_seed(V * 7 + B)
    x = 4.0 * torch.randn(B, V, generator=g)
    top = x.max(1).values
    if V >= 256:
        hi_a, hi_b = 130, 131                      # the top of tile 1, all banned ids of that tile
    else:
        hi_a, hi_b = V - 2, V - 1                  # V = 130: {128, 129}, the second tile is left empty
    last = V - 1                                   # a banned id in the last (partial) tile
    x[:, hi_a] = top + 30.0                        # banned logits 30 / 29 above every allowed one
    x[:, hi_b] = top + 29.0
    x[:, last] = torch.maximum(x[:, last], top + 10.0)
    ban = [0, 1, 3, 3, hi_a, hi_b, last]           # <PAD>, <SOS>, <UNK>, a duplicate, ...
    tie_a, tie_b = 7, V - 3
    r = torch.arange(B)
    x[r % 8 == 2, tie_a] = top[r % 8 == 2] + 5.0   # tied allowed maxima: the smaller id wins
    x[r % 8 == 2, tie_b] = top[r % 8 == 2] + 5.0
    x[r % 8 == 6, tie_a] = top[r % 8 == 6] + 5.0   # ... in one tile
    x[r % 8 == 6, tie_a + 2] = top[r % 8 == 6] + 5.0
    x[r % 8 == 5, EOS] = top[r % 8 == 5] + 20.0    # <EOS> the best allowed token of these rows
    rows = CRows(x, T=3, eos_id=EOS)
    xd = rows.x
    okg = cref.allowed_from_ids(V, ban)
    best = np.where(okg, xd, -np.inf).argmax(1)
    prev = torch.randint(4, V, (B,), generator=g).numpy()
    prev[r.numpy() % 4 == 0] = best[r.numpy() % 4 == 0]         # the previous token is the row's allowed arg-max
    prev[r.numpy() % 4 == 1] = (r.numpy() % 5)[r.numpy() % 4 == 1]   # ... equals a special in some rows
    prev[r.numpy() % 8 == 2] = 9
    prev[r.numpy() % 8 == 6] = 11
    u = torch.rand(B, 3, generator=g)
    u[:3] = torch.tensor([0.0, 1e-9, 0.999999]).view(3, 1)
    return rows, ban, prev, u, (tie_a, tie_b)


_SCEN = {}


def get_scenario(V, B):
    if (V, B) not in _SCEN:
        _SCEN.clear()
        _SCEN[(V, B)] = scenario(V, B)
    return _SCEN[(V, B)]


def check_rows(B):
    """The rows the fp64 sampler reference is evaluated on: the first and the last launch blocks."""
    return np.arange(B) if B <= 40 else np.concatenate([np.arange(24), np.arange(B - 24, B)])


def assert_step(rows, t, ok_rows, u, mode, sel):
    """ok_rows [B,V] bool.  Reference conditions first, then the device's outputs of step t."""
    x, B = rows.x, rows.B
    tau, k, p = FILT if mode == 'filtered' else (1.0, 0, 1.0)
    checks = None
    if mode != 'greedy':
        checks = {b: cref.RowCheck(x[b], ok_rows[b], float(u[b, t]), tau, k, p) for b in sel}
        strict = np.array([checks[b].strict for b in sel])
        gap = max(checks[b].n_hi - checks[b].n_lo for b in sel)
        print('t=%d %s: relaxed rows %.2f %%, widest K-/K+ gap %d' % (t, mode, 100 * (1 - strict.mean()), gap))
        assert (1 - strict.mean()) <= 0.03 and gap <= 1          # on the reference alone
    tok, lp, slp = rows.outputs(t)
    assert ((tok >= 0) & (tok < rows.V)).all()
    assert ok_rows[np.arange(B), tok].all()                      # no banned token, in any row
    lp_ref = torch.log_softmax(torch.from_numpy(x), 1).numpy()[np.arange(B), tok]
    print('   max |seq_logprob - fp64 log_softmax of the full row| = %.2e' % np.abs(lp - lp_ref).max())
    assert np.abs(lp - lp_ref).max() <= LP_TOL
    if mode == 'greedy':
        want = np.where(ok_rows, x, -np.inf).argmax(1)           # (numpy: the first = the smaller id on ties)
        assert (tok == want).all(), np.nonzero(tok != want)[0][:10]
        return tok
    okk = np.array([checks[b].token_ok(tok[b]) for b in sel])
    agree = np.array([tok[b] == checks[b].ref_token() for b in sel])[strict].mean()
    print('   interval check ok on %d / %d rows; exact agreement on strict rows %.2f %%' % (okk.sum(), len(sel), 100 * agree))
    assert okk.all(), sel[~okk][:10]
    assert agree >= 0.98
    if mode == 'filtered':
        ref_slp = np.array([checks[b].sampling_logprob(tok[b]) if checks[b].strict else np.nan for b in sel], dtype=np.float64)
        assert not np.isnan(ref_slp[strict]).any()               # strict rows: the token lies in the kept set
        err = np.nanmax(np.abs(slp[sel] - ref_slp)) if strict.any() else 0.0
        print('   max |sampling_logprob - ref over the restricted set| = %.2e' % err)
        assert err <= LP_TOL
    return tok


GEOMS = [(V, B, m) for V in (128, 130, 10000) for B in (40, 1040) for m in ('greedy', 'sample', 'filtered')] + \
    [(20000, 40, 'filtered')]


@pytest.mark.parametrize('V,B,mode', GEOMS)
def test_constrained_finalize_against_fp64(V, B, mode):
    rows, ban, prev, u, (tie_a, tie_b) = get_scenario(V, B)
    sel = check_rows(B)
    filt = FILT if mode == 'filtered' else None
    greedy = mode == 'greedy'
    okg = cref.allowed_from_ids(V, ban)
    r = np.arange(B)

    def ok_for(prev_ids, eos_banned):
        ok = np.repeat(okg[None], B, 0)
        ok[r, prev_ids] = False
        if eos_banned:
            ok[:, EOS] = False
        return ok
    # ---- t = 0: the fed token is first_id (here an ordinary word, the best allowed one of row 0)
    first = int(np.where(okg, rows.x[0], -np.inf).argmax())
    rows.fresh()
    rows.cstep(0, u, ops.decode_constraints(ban, True, first, 0), filt, greedy)
    assert_step(rows, 0, ok_for(np.full(B, first), False), u, mode, sel)
    # ---- t = 1 < min_len = 2: the row's own previous token and <EOS> are out
    rows.fresh(prev)
    rows.cstep(1, u, ops.decode_constraints(ban, True, first, 2), filt, greedy)
    tok = assert_step(rows, 1, ok_for(prev, True), u, mode, sel)
    assert (tok != EOS).all() and rows.alive.cpu().numpy()[2] == B
    a = rows.outputs(1)
    rows.fresh(prev)
    rows.cstep(1, u, ops.decode_constraints(ban, True, first, 2), filt, greedy)
    assert all(np.array_equal(p, q) for p, q in zip(a, rows.outputs(1)))         # two launches, equal bits
    # ---- t = 1 = min_len: <EOS> is allowed again
    rows.fresh(prev)
    rows.cstep(1, u, ops.decode_constraints(ban, True, first, 1), filt, greedy)
    tok = assert_step(rows, 1, ok_for(prev, False), u, mode, sel)
    if greedy:
        assert (tok[(r % 8 == 5) & (prev != EOS)] == EOS).all()
        assert (tok[r % 8 == 2] == tie_a).all() and (tok[r % 8 == 6] == tie_a).all()          # ties: the smaller id
    ended = tok == EOS
    assert rows.alive.cpu().numpy()[2] == B - ended.sum()
    assert (rows.unf.cpu().numpy() == ~ended).all()
    assert (rows.seq[:, 1].cpu().numpy() == tok).all() and (rows.mk[:, 1] == 1).all()
    # ---- t = 2 on that state: finished rows write <PAD> with mask 0, the others go on without repeating themselves
    rows.cstep(2, u, ops.decode_constraints(ban, True, first, 1), filt, greedy)
    tok2 = rows.raw[:, 2].cpu().numpy()
    seq2, mk2 = rows.seq[:, 2].cpu().numpy(), rows.mk[:, 2].cpu().numpy()
    assert (seq2[ended] == 0).all() and (mk2[ended] == 0).all() and (mk2[~ended] == 1).all()
    assert (seq2[~ended] == tok2[~ended]).all() and (tok2[~ended] != tok[~ended]).all()
    assert okg[tok2[~ended]].all()


# (B, W, xt_add) per form: the wide row is the second trip of the form's own float4 loop - 64 lanes or 256 threads a row
XT_GEOMS = [(B, 4, True, m) for B in (6, 1030) for m in ('greedy', 'sample', 'filtered')] + \
    [(6, 260, False, 'greedy'), (6, 260, False, 'sample'), (6, 1028, False, 'filtered')]


@pytest.mark.parametrize('B,W,xt_add,mode', XT_GEOMS)
def test_constrained_finalize_writes_xt_next(B, W, xt_add, mode):
    """The commit stage behind the constrained choices: 64 lanes per row (greedy, sample; B = 1030 is the sixteen-wave
    kernel with six rows in its last block) or 256 threads (filtered; B = 1030 is a workgroup's second row trip)."""
    rows, u = xt_next_case(CRows, B, W, xt_add, eos_id=EOS)
    rows.cstep(1, u, ops.decode_constraints([0, 1, 3], False, 0, 0), FILT if mode == 'filtered' else None, mode == 'greedy')
    assert_xt_next(rows)
    assert not np.isin(rows.raw[:, 1].cpu().numpy(), [0, 1, 3]).any()
    assert int(rows.alive[2]) == int(rows.unf.sum())


def test_dead_step_refusals_and_the_all_zero_struct():
    V, B = 130, 40
    rows, ban, prev, u, _ = get_scenario(V, B)
    cons = ops.decode_constraints(ban, True, 5, 0)
    # a dead step (alive[t] == 0) writes nothing
    for filt, greedy in ((None, True), (None, False), (FILT, False)):
        rows.fresh(prev)
        rows.alive[1:2].fill_(0)
        rows.lp.fill_(7.0)
        rows.raw.fill_(-1)
        rows.seq[:, 1].fill_(-1)
        rows.cstep(1, u, cons, filt, greedy)
        assert (rows.lp == 7.0).all() and (rows.raw == -1).all() and (rows.seq[:, 1] == -1).all()
        assert rows.alive.cpu().numpy()[2] == 0 and (rows.unf == 1).all()
    # refusals, before any launch: the sentinel-filled outputs stay untouched
    lib = _lib.load()
    rows.fresh(prev)
    rows.lp.fill_(7.0)
    rows.raw.fill_(-1)
    forced = torch.zeros(B, 3, dtype=torch.int64, device=dev())

    def call(st, c, f=None):
        return lib.isc_rollout_finalize_constrained(C.byref(st), f, None if c is None else C.byref(c), ops.stream())
    st = rows.cstep(1, u, None, call=False)
    bad = []
    bad.append(call(st, None))                                                   # null struct
    c = ops.decode_constraints(ban, True, 5, 0); c.n_ban = 9; bad.append(call(st, c))
    c = ops.decode_constraints(ban, True, 5, 0); c.n_ban = -1; bad.append(call(st, c))
    bad.append(call(st, ops.decode_constraints([V], False, 0, 0)))               # an id outside [0, V)
    bad.append(call(st, ops.decode_constraints([-1], False, 0, 0)))
    bad.append(call(st, ops.decode_constraints([], True, V, 0)))
    bad.append(call(st, ops.decode_constraints([], False, 0, 4)))                # min_len > T = 3
    bad.append(call(st, ops.decode_constraints([], False, 0, -1)))
    bad.append(call(rows.cstep(1, u, None, forced=forced, call=False), cons))    # forced + a constraint
    bad.append(call(rows.cstep(1, u, None, logits=False, call=False), cons))     # logits missing
    st5 = rows.cstep(1, u, None, call=False)
    st5.V = 5                                                                    # V <= n_ban + 2: nothing left to choose
    bad.append(call(st5, ops.decode_constraints([0, 1, 3], True, 1, 0)))
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad), bad
    assert bad[0] == bad[-2]                                                     # ISC_E_NULL both
    assert (rows.lp == 7.0).all() and (rows.raw == -1).all()
    assert rows.alive.cpu().numpy()[2] == 0
    # an all-zero struct: the two existing entry points, bit for bit
    zero = _lib.DecodeConstraints()
    for filt, greedy in ((None, True), (None, False), (FILT, False)):
        rows.fresh(prev)
        rows.cstep(1, u, zero, filt, greedy)
        a = [x.clone() for x in (rows.raw, rows.seq, rows.lp, rows.mk, rows.unf, rows.alive)] + \
            ([rows.slp.clone()] if filt else [])
        rows.fresh(prev)
        st = rows.cstep(1, u, None, greedy=greedy, call=False)
        if filt:
            ops.rollout_finalize_filtered(st, *filt, rows.slp)
        else:
            ops.rollout_finalize(st)
        torch.cuda.synchronize()
        b = [rows.raw, rows.seq, rows.lp, rows.mk, rows.unf, rows.alive] + ([rows.slp] if filt else [])
        assert all(torch.equal(p, q) for p, q in zip(a, b))


# ----------------------------------------------------------------------------- end to end
_E2E = {}


def e2e(V):
    """The captioner on the inputs of the beam-1 identity, the fp64 reference roll-outs and the oracle's beam 1."""
    if V not in _E2E:
        st, w, i2w, prm, oid, ins = setup(V)
        cap = Captioner(i2w, synth.SENTIMENT_CATEGORIES, st)
        cap.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
        cap.to(dev()).eval()
        a = [x.float().to(dev()) if x.is_floating_point() else x.to(dev()) for x in ins]
        con = cref.rollout(prm, oid, ins, T, 1, suppress_special=True, decoding_constraint=1)
        beams = []
        with torch.no_grad():
            for b in range(8):
                beams.append(O.beam_search(prm, oid, i2w, ins[0][b], ins[1][b], ins[3][b], ins[4][b:b + 1], beam_size=1,
                                           decoding_constraint=1, max_seq_len=T))
        _E2E[V] = dict(cap=cap, a=a, prm=prm, oid=oid, ins=ins, con=con, beams=beams, st=st, w=w, i2w=i2w)
    return _E2E[V]


def assert_rules(seq, masks, oid, special=True, repeat=True, min_len=0):
    seq, live = np.asarray(seq), np.asarray(masks) > 0
    if special:
        assert not np.isin(seq[live], [oid.pad, oid.sos, oid.unk]).any()
    if repeat:
        prev = np.concatenate([np.full((seq.shape[0], 1), oid.sos), seq[:, :-1]], 1)
        assert (seq[live] != prev[live]).all()
    if min_len:
        assert not (seq[:, :min_len] == oid.eos).any()


@pytest.mark.parametrize('engine', [1, 0], ids=['split_f16', 'exact_fp32'])
@pytest.mark.parametrize('V', [64, 200])
def test_constrained_greedy_is_beam_1(V, engine):
    e = e2e(V)
    cap, a, con, oid = e['cap'], e['a'], e['con'], e['oid']
    margin = con['margins'].min()
    print('V=%d: smallest fp64 margin between the best and the second-best allowed token %.4f' % (V, margin))
    assert margin >= 1e-3                                        # a condition on the reference
    ops.set_h3_mode(engine)
    with torch.no_grad():
        seq, lp, mk = cap.forward_rl(*a, T, 1, suppress_special=True, decoding_constraint=1)
        plain = cap.forward_rl(*a, T, 1)
        _, _, beam_ids = cap.sample_batch(a[0], a[1], a[3], a[4], beam_size=1, decoding_constraint=1, max_seq_len=T)
    seq, lp, mk = seq.cpu().numpy(), lp.cpu().numpy().astype(np.float64), mk.cpu().numpy()
    assert (mk == con['masks']).all() and (seq == con['seq']).all()
    for b, (_, scores, ids) in enumerate(e['beams']):
        n = int(mk[b].sum())
        assert seq[b, :n].tolist() == ids[0] == list(beam_ids[b][0]), b
        err = abs((lp[b] * mk[b]).sum() - scores[0])
        assert err <= ORACLE_TOL * n, (b, err)
    assert_rules(seq, mk, oid)
    assert not torch.equal(plain[0].cpu(), torch.from_numpy(seq))
    ps, pm = plain[0].cpu().numpy(), plain[2].cpu().numpy() > 0
    assert (ps[pm] == oid.unk).any()                             # what the plain greedy roll-out does on these inputs


@pytest.mark.parametrize('engine', [1, 0], ids=['split_f16', 'exact_fp32'])
@pytest.mark.parametrize('V', [64, 200])
def test_min_len_against_the_reference_loop(V, engine):
    e = e2e(V)
    cap, a, oid = e['cap'], e['a'], e['oid']
    want = cref.rollout(e['prm'], oid, e['ins'], T, 1, suppress_special=True, decoding_constraint=1, min_len=4)
    print('V=%d min_len=4: smallest fp64 margin %.4f' % (V, want['margins'].min()))
    assert want['margins'].min() >= 1e-3
    ops.set_h3_mode(engine)
    with torch.no_grad():
        seq, lp, mk = cap.forward_rl(*a, T, 1, suppress_special=True, decoding_constraint=1, min_len=4)
    seq, lp, mk = seq.cpu().numpy(), lp.cpu().numpy(), mk.cpu().numpy()
    assert (seq == want['seq']).all() and (mk == want['masks']).all()
    np.testing.assert_allclose(lp * mk, want['logprobs'] * want['masks'], atol=ORACLE_TOL)
    assert (mk.sum(1) >= 5).all()                                # no <EOS> before t = 4
    short = e['con']['masks'].sum(1) < 4
    assert (mk.sum(1)[short] > e['con']['masks'].sum(1)[short]).all()
    assert_rules(seq, mk, oid, min_len=4)


@pytest.mark.parametrize('engine', [1, 0], ids=['split_f16', 'exact_fp32'])
@pytest.mark.parametrize('ctl', [(1.0, 0, 1.0, False), (1.0, 0, 1.0, True), (0.8, 50, 0.9, True)],
                         ids=['default_controls', 'default_controls_slp', 'filtered'])
@pytest.mark.parametrize('V', [64, 200])
def test_constrained_sampled_rollout_against_the_oracle(V, ctl, engine):
    e = e2e(V)
    cap, a, oid = e['cap'], e['a'], e['oid']
    tau, k, p, want_slp = ctl
    u = torch.rand(8, T, generator=torch.Generator().manual_seed(19))
    ops.set_h3_mode(engine)
    kw = dict(suppress_special=True, decoding_constraint=1, min_len=3)
    with torch.no_grad():
        out = cap.forward_rl(*a, T, 0, _uniforms=u.to(dev()), temperature=tau, top_k=k, top_p=p,
                             return_sampling_logprobs=want_slp, **kw)
    seq, lp, mk = (x.cpu().numpy() for x in out[:3])
    slp = out[3].cpu().numpy() if want_slp else None
    assert_rules(seq, mk, oid, min_len=3)
    # the reference loop fed the device's tokens: every live draw passes the interval check against the loop's row
    want = cref.rollout(e['prm'], oid, e['ins'], T, 0, replay=seq, **kw)
    assert (want['seq'] == seq).all() and (want['masks'] == mk).all()
    checked = 0
    for t, (x, fed, live) in enumerate(zip(want['rows'], want['fed'], want['live'])):
        for b in range(8):
            if live[b]:
                ok = cref.allowed(V, oid, int(fed[b]), t, True, 1, 3)
                rc = cref.RowCheck(x[b], ok, float(u[b, t]), tau, k, p)
                assert rc.token_ok(int(seq[b, t])), (b, t, int(seq[b, t]))
                if want_slp and rc.strict:
                    assert abs(slp[b, t] - rc.sampling_logprob(int(seq[b, t]))) <= ORACLE_TOL
                checked += 1
        np.testing.assert_allclose(lp[live, t], want['logprobs'][live, t], atol=ORACLE_TOL)
    assert checked >= 8 * 3


def test_grouped_form_equals_the_repeated_form():
    e = e2e(64)
    cap, a = e['cap'], e['a']
    n = 3
    u = torch.rand(8 * n, T, generator=torch.Generator().manual_seed(8)).to(dev())
    for ctl in (dict(), dict(temperature=1.3, top_k=20, top_p=0.95)):
        kw = dict(suppress_special=True, decoding_constraint=1, min_len=2, return_sampling_logprobs=True, **ctl)
        with torch.no_grad():
            g = cap.forward_rl(*a, T, 0, _uniforms=u, captions_per_image=n, **kw)
            r = cap.forward_rl(*[x.repeat_interleave(n, 0).contiguous() for x in a], T, 0, _uniforms=u, **kw)
        assert g[0].shape == (8 * n, T) and torch.equal(g[0], r[0]) and torch.equal(g[2], r[2])
        assert float((g[1] - r[1]).abs().max()) <= ORACLE_TOL and float((g[3] - r[3]).abs().max()) <= ORACLE_TOL
        assert_rules(g[0].cpu().numpy(), g[2].cpu().numpy(), e['oid'], min_len=2)


@pytest.mark.parametrize('share', [False, True])
def test_sample_captions_takes_the_constraints(share):
    e = e2e(64)
    cap, a, oid = e['cap'], e['a'], e['oid']
    g = torch.Generator(device=dev())
    g.manual_seed(5)
    caps, ids = cap.sample_captions(*a, n=3, max_seq_len=T, generator=g, share_image=share, temperature=1.2,
                                    suppress_special=True, decoding_constraint=1, min_len=2)
    assert len(caps) == 8 and all(len(c) == 3 for c in caps)
    for per_image, per_ids in zip(caps, ids):
        for s, words in zip(per_image, per_ids):
            toks = s.split()
            assert '<UNK>' not in toks and '<PAD>' not in toks and '<SOS>' not in toks
            assert all(x != y for x, y in zip(toks, toks[1:]))                   # no stutter
            assert len(words) >= 3 and oid.eos not in words[:2]


def test_training_mode_rollout_with_gradients():
    """The differentiable sampled roll-out under constraints: the constraints decide the tokens, the log-probabilities
    and the gradient are the model's own of those tokens - those of the unconstrained call replaying them."""
    st, w, i2w, prm, oid, ins = setup(64, torch.float32)
    cap = Captioner(i2w, synth.SENTIMENT_CATEGORIES, dict(st, dropout_p=0.0))
    cap.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    cap.to(dev()).train()
    a = [x.to(dev()) for x in ins]
    crit = RewardCriterion()
    reward = torch.randn(8, T, generator=torch.Generator().manual_seed(3)).to(dev())
    torch.manual_seed(21)
    seq, lp, mk = cap.forward_rl(*a, T, 0, suppress_special=True, decoding_constraint=1, min_len=2)
    assert lp.requires_grad
    assert_rules(seq.cpu().numpy(), mk.cpu().numpy(), oid, min_len=2)
    cap.zero_grad()
    crit(lp, mk, reward).backward()
    got = {k: q.grad.clone() for k, q in cap.named_parameters() if q.grad is not None}
    seq2, lp2, mk2 = cap.forward_rl(*a, T, 0, _replay=seq)
    assert torch.equal(seq2, seq) and torch.equal(mk2, mk)
    live = mk > 0
    assert float((lp - lp2).detach().abs()[live].max()) <= 1e-5
    cap.zero_grad()
    crit(lp2, mk2, reward).backward()
    assert len(got) > 10
    for k, q in cap.named_parameters():
        if q.grad is not None:
            ref = q.grad
            assert float((got[k] - ref).abs().max()) <= 1e-4 * float(ref.abs().max()) + 1e-7, k


def test_defaults_issue_todays_launches():
    e = e2e(64)
    cap, a = e['cap'], e['a']
    off = dict(suppress_special=False, decoding_constraint=0, min_len=0)
    with torch.no_grad():
        g0, g1 = cap.forward_rl(*a, T, 1), cap.forward_rl(*a, T, 1, **off)
        torch.manual_seed(4)
        s0 = cap.forward_rl(*a, T, 0)
        torch.manual_seed(4)
        s1 = cap.forward_rl(*a, T, 0, **off)
    for x, y in zip(g0 + s0, g1 + s1):
        assert torch.equal(x, y)


def test_detector_rollout_constraints_are_served_eagerly():
    from insenticap_model_amd.detector import Detector
    from test_detector import load_helper
    V, TN, B = 64, 8, 8
    st = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
    det = Detector(synth.make_idx2word(V), TN, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-4}, st)
    det.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=3).items()})
    load_helper(det.senti_detector, 51)
    load_helper(det.sent_senti_cls, 52)
    det.to(dev())
    assert det.train_graphs and det.rollout_constraints is None
    det.rollout_constraints = dict(suppress_special=True, decoding_constraint=1, min_len=2)
    batches, split = synth.make_rl_batches(1, B, V, st, seq_len=TN, seed=70)
    t = torch.from_numpy
    items = [(b[0], t(b[1]), t(b[2]), (t(b[3][0]), b[3][1]), t(b[4]), t(b[5]), b[6]) for b in batches]
    s = synth.make_inputs(4, V, st, regions=6, seq_len=TN, seed=72)
    scs = [((t(s['captions']), s['lengths']), t(s['cpt_words']), t(s['senti_words']), t(s['senti_labels']))]
    det.set_ciderd_scorer(split)
    seen = []
    orig = det.captioner.forward_rl

    def spy(*args, **kw):
        out = orig(*args, **kw)
        seen.append((kw.get('sample_max'), {k: kw.get(k) for k in det.rollout_constraints}, out[0].cpu(), out[2].cpu()))
        return out
    det.captioner.forward_rl = spy
    stats = det((items, scs), 'fact', True)
    torch.cuda.synchronize()
    assert det._rl_graph is None                                  # served eagerly
    assert sorted(x[0] for x in seen) == [0, 1]                   # the sampled roll-out and the greedy baseline
    oid = O.Ids(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES)
    for _, kw, seq, mk in seen:
        assert kw == det.rollout_constraints
        assert_rules(seq.numpy(), mk.numpy(), oid, min_len=2)
    assert stats and all(np.isfinite(float(v)) for v in stats.values())
