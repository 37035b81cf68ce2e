"""The diverse beam search's two kernels - isc_beam_merge_groups, isc_beam_select_groups (csrc/pointwise.hip) - each run
alone on hand-built steps against the restatement of tests/_diverse_beam_ref.py.  The inputs are exact (log-probs on a
2^-6 lattice in rows whose float32 normaliser is 1, scores and lambda multiples of 2^-2), so every output must match bit
for bit: scores, words, lengths, last words, gather / src_row, done, live - whole buffers, one sentinel row behind the
kernel's.  pytest -m gpu."""
import ctypes as C

import numpy as np
import pytest
import torch

import _beam_ref as B
import _diverse_beam_ref as D
from insenticap_model_amd import _lib, ops
from test_gpu_beam_kernels import (DEV, E_NULL, E_SHAPE, ISENT, SEL_KEYS, SENT, STEP_KEYS, TW, collect, dev, fill_common, host,
                                   sent, step_buffers, whole, whole_select)

pytestmark = pytest.mark.gpu
PAD, SOS, EOS, UNK = B.PAD, B.SOS, B.EOS, B.UNK
SHAPES = ((2, 2), (4, 2), (6, 3), (6, 2), (8, 2), (8, 4), (8, 8))
T, V = 4, 40                                  # V = 40: three tiles of TW = 16 columns, the last one half full
KINDS = ('live', 'ended_in_group', 'group_ended', 'frozen', 'all_ended', 'last_group_ended')
TOKENS = [w for w in range(4, 16) if w != EOS]          # a small vocabulary of likely words: the groups meet on tokens


def group_step(seed, n_img, beam, G, t, kinds=KINDS):
    """One step's inputs (the dictionary of _beam_ref.make_step).  Per row `beam` children out of TOKENS with log-probs
    -130 - j / 4 (few values: ties inside rows, across parents, and - lambda a multiple of 1/4 - between a penalised and an
    un-penalised key), scores multiples of 1/4 in [-3, 0]; image i is of kind kinds[i % len]:
    live              every parent expands;
    ended_in_group    one parent of group 0 has ended (the group's second where it has two), the others live;
    group_ended       every parent of group 0 has ended, the other groups live;
    last_group_ended  every parent of the last group has ended;
    all_ended         every parent has ended: latches done, live[t + 1] gets nothing;
    frozen            done at entry: copied through.
    At t == 0 every row holds <SOS> and nothing has ended (rows other than a group's first hold scores that would win)."""
    rng = np.random.default_rng(seed)
    bp = beam // G
    S = dict(n_img=n_img, beam=beam, T=T, t=t, eos=EOS, V=V, grid=False, score_in=[], last_in=[], words_in=[], len_in=[],
             done=[], top_val=[], top_idx=[], kinds=[])
    for i in range(n_img):
        kind = kinds[i % len(kinds)]
        if t == 0 and kind != 'frozen':
            kind = 'live'
        S['kinds'].append(kind)
        S['done'].append(1 if kind == 'frozen' else 0)
        ended = [False] * beam
        if kind == 'ended_in_group':
            ended[1 if bp > 1 else 0] = True
        elif kind == 'group_ended':
            ended[:bp] = [True] * bp
        elif kind == 'last_group_ended':
            ended[beam - bp:] = [True] * bp
        elif kind == 'all_ended':
            ended = [True] * beam
        elif kind == 'frozen':
            ended = [bool(k % 2) for k in range(beam)]
        for k in range(beam):
            score = float(rng.integers(-12, 1)) / 4.0
            if t == 0 and k % bp:
                score = 50.0 + k
            last = SOS if t == 0 else (EOS if ended[k] else int(rng.choice(TOKENS)))
            ids = [int(w) for w in rng.choice([w for w in TOKENS + [EOS] if w != last], size=beam, replace=False)]
            vals = sorted((-130.0 - float(j) / 4.0 for j in rng.integers(0, 4, size=beam)), reverse=True)
            for a in range(beam):                          # equal values: ascending ids, as the top-k leaves them
                b = a
                while b < beam and vals[b] == vals[a]:
                    b += 1
                ids[a:b] = sorted(ids[a:b])
            S['score_in'].append(score)
            S['last_in'].append(last)
            S['len_in'].append(t if (t == 0 or not ended[k]) else int(rng.integers(1, t + 1)))
            S['words_in'].append([int(x) for x in rng.integers(4, V, size=T)])
            S['top_val'].append(vals)
            S['top_idx'].append(ids)
    return S


def want_of(S, tv, ti, G, lam):
    return D.merge_groups_ref(tv, ti, S['score_in'], S['last_in'], S['words_in'], S['len_in'], S['done'], S['t'], S['T'],
                              S['eos'], S['beam'], G, lam)


def run_merge(S, G, lam, **over):
    b = step_buffers(S)
    b['tv'], b['ti'] = dev(S['top_val'], torch.float32), dev(S['top_idx'], torch.int64)
    a = _lib.BeamMergeArgs()
    fill_common(a, S, b)
    a.top_val, a.top_idx, a.gather = b['tv'].data_ptr(), b['ti'].data_ptr(), b['src'].data_ptr()
    for k, v in over.items():
        setattr(a, k, v)
    rc = _lib.load().isc_beam_merge_groups(C.byref(a), G, lam, ops.stream())
    return rc, collect(b, 'gather')


def run_select(S, x, G, lam, state=None, live_in=None, **over):
    n_img, beam = S['n_img'], S['beam']
    rows = n_img * beam
    pm, ps, cv, ci = B.tile_inputs(x, TW, S['last_in'], PAD, SOS, UNK, 1, 1)
    b = step_buffers(S)
    b.update(pm=dev(pm, torch.float32), ps=dev(ps, torch.float32), cv=dev(cv, torch.float32), ci=dev(ci, torch.int32),
             tv=sent(rows + 1, beam), ti=sent(rows + 1, beam, dtype=torch.int64))
    a = _lib.BeamSelectArgs()
    fill_common(a, S, b)
    a.n_tile, a.V = pm.shape[1], S['V']
    a.part_max, a.part_sum, a.cand_val, a.cand_idx = b['pm'].data_ptr(), b['ps'].data_ptr(), b['cv'].data_ptr(), b['ci'].data_ptr()
    a.src_row, a.top_val, a.top_idx = b['src'].data_ptr(), b['tv'].data_ptr(), b['ti'].data_ptr()
    if live_in is not None:
        b['live_in'] = dev([live_in], torch.int32)
        a.live_in = b['live_in'].data_ptr()
    st_in = None
    if state is not None:
        planes, H = state
        st_in = np.random.default_rng(planes * 1000 + H).standard_normal((planes, rows, H)).astype(np.float32)
        b['st_in'], b['st_out'] = dev(st_in, torch.float32), sent(planes * rows * H + H)
        a.state_in, a.state_out, a.state_planes, a.H = b['st_in'].data_ptr(), b['st_out'].data_ptr(), planes, H
    for k, v in over.items():
        setattr(a, k, v)
    rc = _lib.load().isc_beam_select_groups(C.byref(a), G, lam, ops.stream())
    g = collect(b, 'parent')
    g['top_val'], g['top_idx'] = host(b['tv']), host(b['ti'])
    if state is not None:
        g['state'] = host(b['st_out'])
    return rc, g, st_in, b


def hold_both(S, G, lam, name, state=(4, 8)):
    """The merge on the planted pairs and the select on rows that hold them, each whole and exact; the select's state
    re-ordering equals isc_beam_gather on the merge's gather.  -> the restatement's step."""
    w = want_of(S, S['top_val'], S['top_idx'], G, lam)
    rc, got = run_merge(S, G, lam)
    assert rc == 0, name
    B.check_step(got, whole(S, w), name + ' merge', STEP_KEYS + ('gather',))
    x = B.rows_of(S)
    tv, ti = B.topk_rows(x, S['last_in'], S['beam'], PAD, SOS, UNK, 1, 1, np.float32)
    ws = want_of(S, tv, ti, G, lam)
    rc, sel, st_in, b = run_select(S, x, G, lam, state)
    assert rc == 0, name
    B.check_step(sel, whole_select(S, ws, tv, ti, st_in), name + ' select', SEL_KEYS + ('top_val', 'state'))
    live = [r for r in range(len(S['score_in'])) if not S['done'][r // S['beam']]]
    for k in ('score', 'last', 'words', 'length'):         # (live rows: the rows' top-k is the planted one - both kernels agree)
        assert all(np.array_equal(np.asarray(ws[k][r]), np.asarray(w[k][r])) for r in live), (name, k)
    rows = len(S['score_in'])
    planes, H = state
    gat = dev(got['gather'][:rows], torch.int64)
    out = torch.empty(planes, rows, H, device=DEV)
    ops.beam_gather(b['st_in'], b['st_in'], gat, out)
    torch.cuda.synchronize()
    assert np.array_equal(host(out).ravel(), sel['state'][:planes * rows * H]), name
    return w


@pytest.mark.parametrize('n_img', [1, 3])
@pytest.mark.parametrize('beam,G', SHAPES)
def test_both_kernels_are_the_restatement_bit_for_bit(beam, G, n_img):
    """t = 0 and t > 0; an ended parent inside a live group, a whole group ended while others live, all ended (done latches,
    live[t + 1] stays), an already-done image copied through; lambda = 0, 1/4 and 1/2 (exact ties between penalised and
    un-penalised keys and across parents) and 1e3."""
    for t, lam, rot in ((0, 0.25, 0), (2, 0.25, 0), (1, 0.5, 1), (3, 0.0, 2), (2, 1e3, 3), (T - 1, 0.5, 4)):
        kinds = KINDS[rot:] + KINDS[:rot] if n_img == 1 else KINDS[rot % 2::2]
        S = group_step(100 * beam + 10 * G + t + rot, n_img, beam, G, t, kinds)
        w = hold_both(S, G, lam, 'beam %d G %d x%d t %d lam %g' % (beam, G, n_img, t, lam))
        for i, kind in enumerate(S['kinds']):
            assert w['done'][i] == (kind in ('frozen', 'all_ended')), (kind, w['done'])


def test_every_kind_of_image_in_one_launch():
    for (beam, G) in ((6, 3), (8, 2), (4, 2)):
        S = group_step(7 + beam, len(KINDS), beam, G, 2)
        w = hold_both(S, G, 0.5, 'all kinds beam %d' % beam)
        assert w['live_inc'] == len(KINDS) - 2 and S['kinds'] == list(KINDS)


def test_the_planted_steps_hold_ties_and_double_counts():
    """What the shapes above rest on (host arithmetic on the same generator): some group ranks a penalised key EQUAL to an
    un-penalised one, some candidate's token was chosen twice by the groups in front (count 2), and the carried candidates
    are ranked among children."""
    ties = twice = carried = 0
    for beam, G in SHAPES:
        for t, lam in ((2, 0.25), (1, 0.5), (T - 1, 0.5)):
            S = group_step(100 * beam + 10 * G + t, 3, beam, G, t)
            for i in range(S['n_img']):
                if S['done'][i]:
                    continue
                base = i * beam
                parents = [(S['score_in'][base + k], S['last_in'][base + k],
                            list(zip(S['top_val'][base + k], S['top_idx'][base + k]))) for k in range(beam)]
                trace = []
                D.select_step(parents, G, lam, t, EOS, trace)
                for ranked in trace:
                    pen = {c[0] for c in ranked if c[0] != c[1]}
                    ties += any(c[0] in pen for c in ranked if c[0] == c[1])
                    twice += any(c[1] - c[0] == 2 * lam for c in ranked)
                    carried += any(c[4] for c in ranked) and not all(c[4] for c in ranked)
    assert ties > 0 and twice > 0 and carried > 0, (ties, twice, carried)


def test_large_lambda_spreads_the_tokens():
    """lambda = 1e3, every parent live: a token a group appends is none of those the groups in front of it appended at this
    step - every row holds `beam` different finite words and at most g * bp < beam of them are penalised, so a group always
    has bp un-penalised candidates.  (Inside a group nothing is penalised - c_g counts the groups in front only - so two
    parents of one group may still append the same word; with one rank per group every token of the step is distinct.)
    Both kernels, over every appended token."""
    for beam, G in ((6, 3), (8, 8), (4, 2), (8, 4), (6, 2)):
        S = group_step(31 + beam + G, 2, beam, G, 2, ('live',))
        bp = beam // G
        w = want_of(S, S['top_val'], S['top_idx'], G, 1e3)
        rc, got = run_merge(S, G, 1e3)
        assert rc == 0
        B.check_step(got, whole(S, w), 'lambda 1e3 merge', STEP_KEYS + ('gather',))
        rc, sel, _, _ = run_select(S, B.rows_of(S), G, 1e3)
        assert rc == 0
        B.check_step(sel, whole(S, w), 'lambda 1e3 select', STEP_KEYS + ('parent',))
        for out in (got, sel):
            for i in range(2):
                toks = [int(x) for x in out['last'][i * beam:(i + 1) * beam]]
                for g in range(1, G):
                    assert not set(toks[g * bp:(g + 1) * bp]) & set(toks[:g * bp]), (beam, G, toks)
                if bp == 1:
                    assert len(set(toks)) == beam, toks


@pytest.mark.parametrize('beam', [6, 7, 8])
def test_one_group_is_the_plain_entry_point(beam):
    """groups = 1: the outputs of isc_beam_merge / isc_beam_select, for any lambda - on steps with beam^2 = 36, 49, 64
    candidates whose winners are the LAST parent's children (candidate indices past 32: the later a parent, the higher
    its score), and on a step with ended parents."""
    for seed in range(4):
        S = group_step(50 + 10 * beam + seed, 2, beam, 1, 2, ('live',))
        S['score_in'] = [float(k % beam) + s for k, s in enumerate(S['score_in'])]       # (scores in [-3, 0]: rank order reversed)
        w = B.merge_ref(S['top_val'], S['top_idx'], S['score_in'], S['last_in'], S['words_in'], S['len_in'], S['done'], 2, T, EOS,
                        beam)
        assert all(p % beam >= beam - 4 for p in w['parent']) and any(p % beam == beam - 1 for p in w['parent'])
        # (some image keeps four or more children of its last parent: candidate indices up to (beam - 1) * beam + 3 >= 33)
        assert any(sum(p % beam == beam - 1 for p in w['parent'][i * beam:(i + 1) * beam]) >= 4 for i in range(2))
        x = B.rows_of(S)
        for lam in (0.0, 0.5):
            rc, got = run_merge(S, 1, lam)
            assert rc == 0
            B.check_step(got, whole(S, w), 'one group beam %d seed %d' % (beam, seed), STEP_KEYS + ('gather',))
            rc, sel, _, _ = run_select(S, x, 1, lam)
            assert rc == 0
            B.check_step(sel, whole(S, w), 'one group select beam %d seed %d' % (beam, seed), STEP_KEYS + ('parent',))
    S = group_step(5, 3, beam, 1, 2, ('live', 'ended_in_group', 'all_ended'))
    w = B.merge_ref(S['top_val'], S['top_idx'], S['score_in'], S['last_in'], S['words_in'], S['len_in'], S['done'], 2, T, EOS, beam)
    rc, got = run_merge(S, 1, 0.5)
    assert rc == 0
    B.check_step(got, whole(S, w), 'one group', STEP_KEYS + ('gather',))
    rc, sel, _, _ = run_select(S, B.rows_of(S), 1, 0.5)
    assert rc == 0
    B.check_step(sel, whole(S, w), 'one group select', STEP_KEYS + ('parent',))


def test_select_with_live_in_zero_touches_nothing():
    S = group_step(9, 3, 6, 3, 2)
    x = B.rows_of(S)
    rc, sel, st_in, _ = run_select(S, x, 3, 0.5, state=(4, 8), live_in=0)
    assert rc == 0
    B.check_step(sel, whole_select(S, None, None, None, st_in, touched=False), 'live_in 0', SEL_KEYS + ('top_val', 'state'))
    tv, ti = B.topk_rows(x, S['last_in'], 6, PAD, SOS, UNK, 1, 1, np.float32)
    rc, sel, st_in, _ = run_select(S, x, 3, 0.5, state=(4, 8), live_in=5)
    assert rc == 0
    B.check_step(sel, whole_select(S, want_of(S, tv, ti, 3, 0.5), tv, ti, st_in), 'live_in 5', SEL_KEYS + ('top_val', 'state'))


def test_refusals_before_the_launch():
    S = group_step(3, 2, 6, 3, 2)
    x = B.rows_of(S)
    for G, lam in ((0, 0.5), (-3, 0.5), (4, 0.5), (5, 0.0), (3, -0.25), (3, float('inf')), (3, float('nan'))):
        rc, got = run_merge(S, G, lam)
        assert rc == E_SHAPE, (G, lam)
        B.check_step(dict(got, parent=got['gather']), whole(S, None, touched=False), 'merge refusal %r' % ((G, lam),))
        rc, sel, _, _ = run_select(S, x, G, lam)
        assert rc == E_SHAPE, (G, lam)
        B.check_step(sel, whole_select(S, None, None, None, touched=False), 'select refusal %r' % ((G, lam),),
                     SEL_KEYS + ('top_val',))
    assert run_merge(S, 3, 0.5, beam=9)[0] == E_SHAPE and run_merge(S, 3, 0.5, t=T)[0] == E_SHAPE
    assert run_merge(S, 3, 0.5, top_val=None)[0] == E_NULL and run_select(S, x, 3, 0.5, src_row=None)[0] == E_NULL
    assert run_select(S, x, 3, 0.5, n_tile=0)[0] == E_SHAPE
