"""The helper the beam-kernel tests stand on (tests/_beam_ref.py), on the host: its merge agrees with the two host merges
of insenticap_model_amd.beam over whole searches full of ties, the generated select inputs say what the logits say (a
k-way merge of the tile lists is the row's top-k; exact rows have S == 1.0 in float32), and the comparison the GPU tests
use can fail - one injected defect at a time, on the very scenarios those tests run."""
import numpy as np
import pytest

import _beam_ref as B
from insenticap_model_amd import beam as host_beam

PAD, SOS, EOS, UNK = B.PAD, B.SOS, B.EOS, B.UNK


# ------------------------------------------------------------------------------------------------ vs the host mirrors
@pytest.mark.parametrize('beam', [1, 3, 8])
def test_merge_ref_equals_both_host_merges_over_a_search(beam):
    """7 images from t = 0, T = 9, a vocabulary of 12 words (so <EOS> is frequent), log-probs on a grid of 0.25 (so sums
    tie all the time): gather, fed tokens and done step by step, words and fp64 scores at the end."""
    n_img, T, V = 7, 9, 12
    rows = n_img * beam
    rng = np.random.default_rng(beam)
    lm = host_beam._ListMerge(n_img, beam, SOS, EOS)
    vm = host_beam._VectorMerge(n_img, beam, T, SOS, EOS)
    st = dict(score=[0.0] * rows, last=[SOS] * rows, words=[[0] * T for _ in range(rows)], length=[0] * rows, done=[0] * n_img)
    last_l, gat_l = np.full(rows, SOS, np.int64), np.zeros(rows, np.int64)
    last_v, gat_v = np.full(rows, SOS, np.int64), np.zeros(rows, np.int64)
    ties = 0
    for t in range(T):
        ti = np.stack([rng.choice(np.arange(4 if t < 2 else 2, V), size=beam, replace=False) for _ in range(rows)]).astype(np.int64)
        tv = -np.sort(rng.integers(0, 9, size=(rows, beam)), axis=1).astype(np.float32) * 0.25
        out = B.merge_ref(tv.tolist(), ti.tolist(), st['score'], st['last'], st['words'], st['length'], st['done'], t, T, EOS, beam)
        live_l = lm.step(t, ti, tv, last_l, gat_l)
        live_v = vm.step(t, ti, tv, last_v, gat_v)
        assert live_l == live_v == (out['live_inc'] > 0), t
        assert gat_l.tolist() == out['gather'] and gat_v.tolist() == out['gather'], t
        assert last_l.tolist() == out['last'] and last_v.tolist() == out['last'], t
        assert lm.done == [bool(x) for x in out['done']] and vm.done.tolist() == lm.done, t
        for i in range(n_img):
            sc = out['score'][i * beam:(i + 1) * beam]
            ties += len(set(sc)) < len(sc)
        st = out
        if not live_l:
            break
    assert beam == 1 or ties > 3                     # the stable order was exercised, not assumed
    for res in (lm.result(), vm.result()):
        for i in range(n_img):
            for k, (score, words) in enumerate(res[i]):
                row = i * beam + k
                assert score == st['score'][row] and list(words) == st['words'][row][:st['length'][row]], (i, k)


# ------------------------------------------------------------------------------------------------ the generated inputs
@pytest.mark.parametrize('V,tw,special,cons', [(300, 16, 1, 1), (257, 8, 0, 1), (96, 64, 1, 0), (130, 128, 0, 0)])
def test_tile_lists_of_grid_rows_merge_to_the_rows_topk(V, tw, special, cons):
    """topk_ref (log-probs, float64) and the k-way merge of tile_inputs' lists (raw logits) pick the same ids in the same
    order on grid rows, and the tile statistics fold to the row's normaliser."""
    rng = np.random.default_rng(V)
    rows, beam = 6, 8
    x = B.grid_rows(rng, rows, V, -0.03125, 0.03125)         # 65 grid values: every row's top 8 holds ties
    last = rng.integers(4, V, size=rows).tolist()
    pm, ps, cv, ci = B.tile_inputs(x, tw, last, PAD, SOS, UNK, special, cons)
    assert pm.shape == (rows, (V + tw - 1) // tw) and cv.shape == pm.shape + (8,)
    tied = 0
    for r in range(rows):
        vals, ids = B.topk_ref(x[r], last[r], beam, PAD, SOS, UNK, special, cons)
        kv, ki = B.kway_topk(cv[r], ci[r], beam)
        assert ids == ki and kv == [float(x[r, i]) for i in ids]
        assert not (set(ids) & B.masked(V, last[r], PAD, SOS, UNK, special, cons))
        tied += len(set(kv)) < beam
        lp, S = B.row_logp(x[r], np.float64)
        m, Sf = B.fold_stats(pm[r], ps[r], np.float64)
        assert m == x[r].max() and abs(Sf - S) <= 1e-6 * S
        assert vals == [float(lp[i]) for i in ids] and len(set(vals)) == len(set(kv))     # different logits stay different
        # inside a list: value descending, equal values in ascending id
        for j in range(cv.shape[1]):
            for s in range(7):
                assert cv[r, j, s] > cv[r, j, s + 1] or (cv[r, j, s] == cv[r, j, s + 1] and
                                                        (ci[r, j, s] < ci[r, j, s + 1] or ci[r, j, s + 1] == 0))
    assert tied == rows


def test_exact_rows_have_unit_normaliser_in_float32():
    """S == 1.0 and log S == 0 in float32, summed directly and folded from tile statistics of any width: log-prob ==
    logit, bit for bit."""
    rng = np.random.default_rng(5)
    x = B.exact_rows(rng, 4, 1000, PAD)
    for r in range(4):
        lp, S = B.row_logp(x[r], np.float32)
        assert S == np.float32(1.0) and S.dtype == np.float32
        keep = np.arange(1000) != PAD
        assert np.array_equal(lp[keep], x[r][keep]) and lp[PAD] == 0.0
    for tw in (8, 16, 128):
        pm, ps, _, _ = B.tile_inputs(x, tw, [5] * 4, PAD, SOS, UNK, 1, 1)
        for r in range(4):
            m, S = B.fold_stats(pm[r], ps[r], np.float32)
            assert m == 0.0 and S == np.float32(1.0)


def test_scenarios_plant_what_they_promise():
    """Every scenario's rows give back the planted (value, id) pairs of the rows that count, the planted ties are ties in
    fp64, every kind occurs, and on grid rows the distinct scores around the cut stay 1e-5 apart (no fp32 near-tie can
    reorder the winners)."""
    kinds, tie_carry, tie_twin = set(), 0, 0
    for kw in B.scenarios():
        for grid in (False, True):
            S = B.make_step(grid=grid, V=96, **kw)
            beam, t = S['beam'], S['t']
            x = B.rows_of(S)
            kinds |= set(S['kinds'])
            for i in range(S['n_img']):
                for k in range(1 if t == 0 else beam):
                    r = i * beam + k
                    if S['done'][i] or (t > 0 and S['last_in'][r] == EOS):
                        continue
                    vals, ids = B.topk_ref(x[r], S['last_in'][r], beam, PAD, SOS, UNK, 1, 1)
                    assert ids == S['top_idx'][r] and [float(x[r, w]) for w in ids] == S['top_val'][r]
                    if not grid:
                        assert B.row_logp(x[r], np.float32)[1] == np.float32(1.0)
            if grid:
                tv = B.topk_rows(x, S['last_in'], beam, PAD, SOS, UNK, 1, 1)[0]
                for i in range(S['n_img']):
                    sc = sorted({S['score_in'][i * beam + k] + v for k in range(beam) for v in tv[i * beam + k]
                                 if np.isfinite(S['score_in'][i * beam + k])}, reverse=True)[:beam + 1]
                    assert all(a - b > 1e-5 for a, b in zip(sc, sc[1:]))      # (fp32 log-probs of |lp| < 32 err by < 4e-6)
                continue
            for i, kind in enumerate(S['kinds']):
                sc, tv = S['score_in'][i * beam:(i + 1) * beam], S['top_val'][i * beam:(i + 1) * beam]
                if kind in ('carry_first', 'carry_last'):
                    a, b = (0, beam - 1) if kind == 'carry_first' else (beam - 1, 0)
                    assert sc[a] == sc[b] + tv[b][0] and S['last_in'][i * beam + a] == EOS
                    tie_carry += 1
                if kind == 'twins':
                    tie_twin += any(sc[p] == sc[q] and tv[p] == tv[q] for p in range(beam) for q in range(p))
    assert kinds == set(B.KINDS) and tie_carry >= 8 and tie_twin >= 8


# ------------------------------------------------------------------------------------------------ injected defects
def _model(S, x, state, defect=None):
    """The beam step as a kernel computes it (index arithmetic over flat buffers, rank by counting), on exact rows - with
    ONE defect injected.  Returns what the GPU tests collect from a kernel: top_val / top_idx, the new bookkeeping,
    parent, gather, done, live_inc, state."""
    beam, T, t, eos, n_img, V = S['beam'], S['T'], S['t'], S['eos'], S['n_img'], S['V']
    rows = n_img * beam
    tv, ti = [], []
    for r in range(rows):
        ban = B.masked(V, S['last_in'][r], PAD, SOS, -1 if defect == 'unk_unmasked' else UNK, 1,
                       0 if defect == 'last_word_unmasked' else 1)
        lp = [B.NEG if c in ban else (0.0 if c == PAD else float(x[r, c])) for c in range(V)]
        order = sorted(range(V), key=lambda c: (-lp[c], -c if defect == 'ties_to_larger_id' else c))[:beam]
        tv.append([lp[c] for c in order])
        ti.append(order)
    score, last, length = list(S['score_in']), list(S['last_in']), list(S['len_in'])
    words = [w for row in S['words_in'] for w in row] + [0] * T       # flat, one row of slack behind the last row
    words_in = list(words)
    done, parent, gather, live_inc = list(S['done']), list(range(rows)), [r + rows for r in range(rows)], 0
    stray = []
    for i in range(n_img):
        base = i * beam
        if S['done'][i] and defect != 'frozen_updated':
            continue
        cs = []                                                       # (score, token, parent, carried)
        ncand = beam if (t > 0 or defect == 't0_every_row_a_parent') else 1
        all_ended = True
        for k in range(ncand):
            r = base + k
            ended = t > 0 and S['last_in'][r] == eos
            all_ended &= ended
            if ended and defect != 'carried_expanded':
                cs.append((S['score_in'][r], eos, r, True))
                continue
            for j in range(beam):
                s = (float(np.float32(S['score_in'][r]) + np.float32(tv[r][j])) if defect == 'fp32_score_sums'
                     else S['score_in'][r] + tv[r][j])
                cs.append((s, ti[r][j], r, False))
        for c, (s, tok, par, car) in enumerate(cs):
            def before(j):
                if cs[j][0] != s:
                    return cs[j][0] > s
                if defect == 'unstable_sort':
                    return j > c
                if defect == 'carried_loses_to_equal_child' and car != cs[j][3]:
                    return car
                return j < c
            rank = sum(before(j) for j in range(len(cs)) if j != c)
            if rank >= beam:
                continue
            dst, n = base + rank, S['len_in'][par]
            score[dst], last[dst], parent[dst] = s, tok, par
            gather[dst] = par + rows if (car and defect != 'gather_without_rows') else par
            words[dst * T:(dst + 1) * T] = words_in[par * T:(par + 1) * T]
            length[dst] = n + (0 if car else 1)
            if not car:
                at = n + 1 if defect == 'token_at_len_plus_1' else n
                if at < T:
                    words[dst * T + at] = tok
                elif defect == 'token_written_when_full':
                    stray.append((dst * T + at, tok))
        if all_ended and defect != 'done_not_latched':
            done[i] = 1
        if not all_ended or defect == 'live_counts_all_ended':
            live_inc += 1
    for at, tok in stray:                                             # (the next row's first slot)
        words[at] = tok
    src = list(range(rows)) if defect == 'state_from_own_row' else parent
    return dict(top_val=tv, top_idx=ti, score=score, last=last, length=length,
                words=words, done=done, parent=parent,
                gather=gather, live_inc=live_inc, state=B.state_ref(state, src))


def _want(S, x, state):
    """What the GPU tests expect of a step on exact rows (test_gpu_beam_kernels.expected_exact)."""
    tv, ti = B.topk_rows(x, S['last_in'], S['beam'], PAD, SOS, UNK, 1, 1, np.float32)
    w = B.merge_ref(tv, ti, S['score_in'], S['last_in'], S['words_in'], S['len_in'], S['done'], S['t'], S['T'], S['eos'], S['beam'])
    w['words'] = [v for row in w['words'] for v in row] + [0] * S['T']     # flat, with the buffer's row of slack
    w['top_val'], w['top_idx'], w['state'] = tv, ti, B.state_ref(state, w['parent'])
    return w


DEFECTS = ['ties_to_larger_id', 'unstable_sort', 'carried_expanded', 'carried_loses_to_equal_child', 'fp32_score_sums',
           'last_word_unmasked', 'unk_unmasked', 'gather_without_rows', 'token_at_len_plus_1', 'token_written_when_full',
           'frozen_updated', 'done_not_latched', 'live_counts_all_ended', 'state_from_own_row', 't0_every_row_a_parent']


@pytest.fixture(scope='module')
def cases():
    out = []
    for kw in B.scenarios():
        S = B.make_step(V=96, **kw)
        x = B.rows_of(S)
        state = np.random.default_rng(1).standard_normal((2, S['n_img'] * S['beam'], 4)).astype(np.float32)
        out.append((S, x, state, _want(S, x, state)))
    return out


def test_the_model_without_a_defect_passes_every_scenario(cases):
    for n, (S, x, state, want) in enumerate(cases):
        B.check_step(_model(S, x, state), want, 'scenario %d' % n)


@pytest.mark.parametrize('defect', DEFECTS)
def test_every_single_defect_raises(cases, defect):
    raised = 0
    for n, (S, x, state, want) in enumerate(cases):
        try:
            B.check_step(_model(S, x, state, defect), want, 'scenario %d' % n)
        except AssertionError:
            raised += 1
    assert raised >= 1, defect
    print('%s: caught on %d of %d scenarios' % (defect, raised, len(cases)))
