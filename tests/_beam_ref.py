"""The beam-search step in plain Python, for tests/test_gpu_beam_kernels.py (checked on the host by
tests/test_beam_ref_host.py): the masked top-k, the candidate merge and what the one-launch select reads.

Written from the reference's `sample()` (captioner.py:378-411): per image a candidate loop - a candidate that ended at
t > 0 is carried as ONE candidate, every other one is expanded into its `beam` best words, scores are Python floats
(fp64 sums of fp32 log-probs) - and `sorted(..., reverse=True)[:beam]`, a STABLE descending sort in insertion order.
Lists and Python floats; numpy only for the log-softmax of a row and for arrays handed to a kernel.  Nothing here imports
insenticap_model_amd.beam.

The one place the reference leaves an order open is two words of EQUAL fp32 log-prob inside a row (`torch.sort` is not
stable); the kernels resolve it to the smaller id, and so does `topk_ref`.  The two input generators stay away from the
neighbouring trap - two DIFFERENT logits rounding to the same log-prob, where a kernel that compares raw logits
(isc_beam_select) and one that compares log-probs (isc_beam_topk) could legitimately differ:

  grid rows   logits = multiples of 2^-10 in [-8, 8]: x - max is exact and (x - max) - log S keeps different logits
              different, so the expected ids are the (raw logit descending, id ascending) order for every kernel;
  exact rows  one masked word at logit 0, every other a multiple of 2^-6 in [-160, -128]: in float32 S == 1.0 and
              log S == 0 exactly (also folded from tile statistics), so log-prob == logit bit for bit and every fp64 sum
              with a dyadic score is exact - scores, ties between a carried candidate and a child, ties between
              children of two parents are all decided exactly."""
import numpy as np

NEG = float('-inf')
KC = 8                   # entries per tile candidate list (ROWS_KC)
PAD, SOS, EOS, UNK = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------ top-k
def masked(V, last, pad, sos, unk, mask_special, cons):
    """The set of word ids a step may not produce (captioner.py:394-399)."""
    ban = set()
    if mask_special:
        ban |= {int(pad), int(sos), int(unk)}
    if cons:
        ban.add(int(last))
    return {i for i in ban if 0 <= i < V}


def row_logp(logits, dtype):
    """((x - max) - log(sum exp(x - max)), the sum) of one row of raw logits, evaluated in `dtype`."""
    x = np.asarray(logits, dtype=dtype)
    m = x.max()
    S = np.exp(x - m).sum(dtype=dtype)
    return (x - m) - np.log(S), S


def topk_ref(logits, last, beam, pad, sos, unk, mask_special, cons, dtype=np.float64):
    """One row: the `beam` best (log-prob, id) of the masked log_softmax in `dtype` (float64: the reference; float32:
    err32), value descending, id ascending; masked words take part as -inf, at the tail.  -> (values, ids) as lists."""
    lp, _ = row_logp(logits, dtype)
    lp = [float(v) for v in lp]
    for i in masked(len(lp), last, pad, sos, unk, mask_special, cons):
        lp[i] = NEG
    order = sorted(range(len(lp)), key=lambda i: (-lp[i], i))[:beam]
    return [lp[i] for i in order], order


def topk_rows(logits, last, beam, pad, sos, unk, mask_special, cons, dtype=np.float64):
    out = [topk_ref(logits[r], last[r], beam, pad, sos, unk, mask_special, cons, dtype) for r in range(len(logits))]
    return [v for v, _ in out], [i for _, i in out]


# ------------------------------------------------------------------------------------------------ merge
def merge_ref(top_val, top_idx, score_in, last_in, words_in, len_in, done, t, T, eos, beam):
    """One step for every image.  Rows are image-major (row = image * beam + rank).  Returns a dict:
    score / last / words / length  the new rows' bookkeeping (words: the whole T-slot list, the new token at the
                                   parent's length when that is < T);
    done      the latches after the step (set on the step where every parent has ended - whose carried candidates are
              still re-sorted, stably, as `sorted` does);
    parent    source row of every new row; gather = parent (+ rows for a carried candidate, which keeps its old state);
    live_inc  the increment of live[t + 1]: images neither frozen at entry nor all-ended.
    A frozen image (done at entry) carries everything over: parent = the row itself, gather = row + rows."""
    n_img = len(done)
    rows = n_img * beam
    out = dict(score=[float(s) for s in score_in], last=[int(w) for w in last_in], words=[list(map(int, w)) for w in words_in],
               length=[int(n) for n in len_in], done=[int(bool(x)) for x in done], parent=list(range(rows)),
               gather=[r + rows for r in range(rows)], live_inc=0)
    for i in range(n_img):
        base = i * beam
        if done[i]:
            continue
        tmp = []                                            # (score, last word, parent row, carried)
        end_flag = True
        for k in range(1 if t == 0 else beam):
            row = base + k
            if t > 0 and int(last_in[row]) == eos:
                tmp.append((float(score_in[row]), int(last_in[row]), row, True))
                continue
            end_flag = False
            for j in range(beam):
                tmp.append((float(score_in[row]) + float(top_val[row][j]), int(top_idx[row][j]), row, False))
        tmp = sorted(tmp, key=lambda c: c[0], reverse=True)[:beam]
        assert len(tmp) == beam
        for r, (score, word, par, carried) in enumerate(tmp):
            dst = base + r
            n = int(len_in[par])
            words = list(map(int, words_in[par]))
            if not carried and n < T:
                words[n] = word
            out['score'][dst], out['last'][dst], out['words'][dst] = score, word, words
            out['length'][dst] = n + (0 if carried else 1)
            out['parent'][dst], out['gather'][dst] = par, par + rows if carried else par
        if end_flag:
            out['done'][i] = 1
        else:
            out['live_inc'] += 1
    return out


def state_ref(state_in, parent):
    """The recurrent state follows the candidates: out[p, r, :] = in[p, parent[r], :] ([planes, rows, H] numpy)."""
    return np.ascontiguousarray(state_in[:, np.asarray(parent, dtype=np.int64), :])


EXACT_KEYS = ('last', 'words', 'length', 'done', 'parent', 'gather', 'live_inc', 'live', 'score', 'state', 'top_idx', 'top_val')


def check_step(got, want, name, keys=None):
    """The comparison of the kernel tests: every output named in `keys` (default: every key both hold) equal element by
    element, shape included - ids, parents, latches and counters always, fp64 scores and fp32 values wherever the inputs
    make them exact.  -inf equals -inf; a NaN equals nothing."""
    for k in (keys if keys is not None else [k for k in EXACT_KEYS if k in got and k in want]):
        g, w = np.atleast_1d(np.asarray(got[k])), np.atleast_1d(np.asarray(want[k]))
        assert g.shape == w.shape, '%s/%s: shape %r, not %r' % (name, k, g.shape, w.shape)
        bad = np.argwhere(~(g == w))
        assert bad.size == 0, '%s/%s: element %s holds %r, not %r (%d differ)' % (
            name, k, tuple(bad[0].tolist()), g[tuple(bad[0])].item(), w[tuple(bad[0])].item(), len(bad))


# ------------------------------------------------------------------------------------------------ the select's inputs
def tile_inputs(logits, tw, last, pad, sos, unk, mask_special, cons):
    """What isc_beam_select reads, from float32 rows `logits` [rows, V] cut into tiles of `tw` >= 8 columns:
    pmax, psum [rows, n_tile] float32   max and float32(sum in float64 of exp(x - max)) of the RAW logits of every tile;
    cand_val, cand_idx [rows, n_tile, 8]  the 8 largest MASKED logits of every tile with their ids: value descending, id
                                        ascending (a masked word is a -inf entry under its own id), padded with (-inf, 0).
    The select takes n_tile and ids, never a tile width."""
    x = np.asarray(logits, dtype=np.float32)
    rows, V = x.shape
    assert tw >= KC
    nt = (V + tw - 1) // tw
    pmax, psum = np.zeros((rows, nt), np.float32), np.zeros((rows, nt), np.float32)
    cv, ci = np.full((rows, nt, KC), NEG, np.float32), np.zeros((rows, nt, KC), np.int32)
    for r in range(rows):
        ban = masked(V, last[r], pad, sos, unk, mask_special, cons)
        for j in range(nt):
            c0, c1 = j * tw, min(V, (j + 1) * tw)
            seg = x[r, c0:c1].astype(np.float64)
            pmax[r, j] = seg.max()
            psum[r, j] = np.exp(seg - seg.max()).sum()
            ent = sorted(((NEG if c in ban else float(x[r, c]), c) for c in range(c0, c1)), key=lambda e: (-e[0], e[1]))[:KC]
            for s, (v, c) in enumerate(ent):
                cv[r, j, s], ci[r, j, s] = v, c
    return pmax, psum, cv, ci


def fold_stats(pmax, psum, dtype=np.float32):
    """(max, S = sum_j psum_j exp(pmax_j - max)) of one row's tile statistics in `dtype`: every decode path's normaliser."""
    pm, ps = np.asarray(pmax, dtype=dtype), np.asarray(psum, dtype=dtype)
    m = pm.max()
    return m, (ps * np.exp(pm - m)).sum(dtype=dtype)


def kway_topk(cv, ci, beam):
    """The `beam` best (value, id) of one row's tile lists [n_tile, 8]: value descending, id ascending."""
    ent = sorted(((float(cv[j, s]), int(ci[j, s])) for j in range(cv.shape[0]) for s in range(KC)),
                 key=lambda e: (-e[0], e[1]))[:beam]
    return [v for v, _ in ent], [c for _, c in ent]


# ------------------------------------------------------------------------------------------------ input generators
GRID_UNIT, EXACT_UNIT, SCORE_LOW = 2.0 ** -10, 2.0 ** -6, 2.0 ** -30


def grid_rows(rng, rows, V, lo=-8.0, hi=8.0):
    """float32 [rows, V]: multiples of 2^-10 in [lo, hi] (within [-8, 8]): plenty of exact ties."""
    assert -8.0 <= lo < hi <= 8.0
    return (rng.integers(int(lo / GRID_UNIT), int(hi / GRID_UNIT) + 1, size=(rows, V)) * GRID_UNIT).astype(np.float32)


def exact_rows(rng, rows, V, hot, lo=-160.0, hi=-128.0):
    """float32 [rows, V]: word `hot` (a masked one) at 0, every other a multiple of 2^-6 in [lo, hi] (within
    [-160, -128]): S == 1.0 in float32, so log-prob == logit."""
    assert -160.0 <= lo < hi <= -128.0
    x = (rng.integers(int(lo / EXACT_UNIT), int(hi / EXACT_UNIT) + 1, size=(rows, V)) * EXACT_UNIT).astype(np.float32)
    x[:, hot] = 0.0
    return x


# ------------------------------------------------------------------------------------------------ scenarios
KINDS = ('live', 'frozen', 'ended_all', 'ended_some', 'carry_first', 'carry_last', 'twins', 'neginf_all', 'neginf_some')


def make_step(seed, n_img, beam, T, t, V, kinds=KINDS, grid=False, lens=None, eos=EOS):
    """One step's inputs for `n_img` images whose kinds cycle through `kinds` (image i: kinds[i % len]):
    live         every parent expands; scores carry low bits (multiples of 2^-30), which float32 sums would lose;
    frozen       done at entry (its rows hold anything, <EOS> among the last words): carried over untouched;
    ended_all    every parent has ended, scores unsorted and with ties: latches, and the carried rows are re-sorted;
    ended_some   some parents ended;
    carry_first  / carry_last: an ended parent whose score EQUALS the best child of a live parent of higher / lower
                 rank - the stable order decides (carried before the child, or after it);
    twins        two parents with identical score, words and children: insertion order decides;
    neginf_all   every score -inf (some parents ended): every candidate ties at -inf, none may turn into NaN;
    neginf_some  parent 0 at -inf, the others finite.
    At t == 0 rows 1 .. beam - 1 hold unequal garbage everywhere (high scores, <EOS> last words): only row 0 counts, and
    the kinds that need an ended parent fall back to 'live'.  beam == 1 has no second parent: those kinds fall back too.
    Planted per row: `beam` distinct unmasked ids with values drawn from a small pool (ties inside a row resolve to
    ascending ids, as the top-k leaves them) - log-probs of exact rows (multiples of 2^-6 in [-136, -129]) or, grid =
    True, raw logits on the 2^-10 grid in (2, 7].  `lens`: len_in per row (cycled; default t, an ended row's <= t).
    -> dict of lists (n_img, beam, T, t, eos, V, score_in, last_in, words_in, len_in, done, top_val, top_idx, kinds)."""
    rng = np.random.default_rng(seed)
    rows = n_img * beam
    unit = GRID_UNIT if grid else EXACT_UNIT
    pool_lo, pool_hi = (int(2.0 / unit) + 1, int(7.0 / unit)) if grid else (int(-136.0 / unit), int(-129.0 / unit))
    S = dict(n_img=n_img, beam=beam, T=T, t=t, eos=eos, V=V, grid=grid, score_in=[], last_in=[], words_in=[], len_in=[],
             done=[], top_val=[], top_idx=[], kinds=[])
    free = [w for w in range(V) if w not in (PAD, SOS, UNK)]
    for i in range(n_img):
        kind = kinds[i % len(kinds)]
        if kind != 'frozen' and (t == 0 or beam == 1) and kind not in ('live', 'neginf_all'):
            kind = 'ended_all' if (beam == 1 and t > 0 and kind == 'ended_all') else 'live'
        S['kinds'].append(kind)
        S['done'].append(1 if kind == 'frozen' else 0)
        pool = rng.integers(pool_lo, pool_hi + 1, size=4)                       # few values: ties inside and across rows
        score = [float(rng.integers(-640, 1)) * EXACT_UNIT for _ in range(beam)]
        if kind == 'live':
            score = [s + float(rng.integers(1, 1024)) * SCORE_LOW for s in score]
        last = [int(rng.choice([w for w in free if w != eos])) for _ in range(beam)]
        ended = [False] * beam
        if kind == 'frozen':
            ended = [bool(rng.integers(0, 2)) for _ in range(beam)]
        elif kind == 'ended_all':
            ended = [True] * beam
            score = [float(rng.integers(-3, 0)) for _ in range(beam)]           # three values: unsorted, tied
        elif kind in ('ended_some', 'neginf_all'):
            ended = [bool(k % 2) for k in range(beam)] if beam > 1 else [False]
            if kind == 'ended_some' and beam > 2:
                ended[int(rng.integers(0, beam))] ^= True
                if all(ended) or not any(ended):
                    ended[0] ^= True
        vals, ids = [], []
        for k in range(beam):
            v = sorted((float(x) * unit for x in rng.choice(pool, size=beam)), reverse=True)
            w = [int(x) for x in rng.choice([c for c in free if c != last[k]], size=beam, replace=False)]
            for a in range(beam):                                               # equal values: ascending ids
                b = a
                while b < beam and v[b] == v[a]:
                    b += 1
                w[a:b] = sorted(w[a:b])
            vals.append(v)
            ids.append(w)
        if kind in ('carry_first', 'carry_last'):
            a, b = (0, beam - 1) if kind == 'carry_first' else (beam - 1, 0)
            ended[a] = True
            score[a] = score[b] + vals[b][0]          # dyadic: the sum is exact in fp64 (and the tie too)
            if grid:
                score[a] = score[b]                   # (grid rows: the child's log-prob is not known exactly - no planted tie)
        if kind == 'twins':
            p, q = (0, 1) if beam == 2 else sorted(int(x) for x in rng.choice(beam, size=2, replace=False))
            score[q], vals[q], ids[q], last[q] = score[p], list(vals[p]), list(ids[p]), last[p]
        if kind == 'neginf_all':
            score = [NEG] * beam
        if kind == 'neginf_some':
            score[0] = NEG
        if t == 0 and kind != 'frozen':               # rows 1..: garbage that would win if it counted
            ended = [False] + [bool(k % 2) for k in range(1, beam)]
            score = score[:1] + [100.0 + k for k in range(1, beam)]
        for k in range(beam):
            if ended[k]:
                last[k] = eos
            n = t if lens is None else int(lens[(i * beam + k) % len(lens)])
            if lens is None and ended[k] and t > 0:
                n = int(rng.integers(1, t + 1))
            if lens is None and t == 0 and k > 0:
                n = int(rng.integers(0, T + 1))
            S['len_in'].append(n)
            S['words_in'].append([int(x) for x in rng.integers(4, V, size=T)])
        if kind == 'twins':
            S['words_in'][i * beam + q] = list(S['words_in'][i * beam + p])
        S['score_in'] += score
        S['last_in'] += last
        S['top_val'] += vals
        S['top_idx'] += ids
    assert len(S['score_in']) == rows
    return S


def rows_of(S, seed=0, hot=PAD):
    """Logit rows [rows, V] float32 whose masked top-`beam` are the scenario's planted (value, id) pairs: exact rows
    (every other word in [-160, -137], the masked word `hot` at 0) or grid rows (every other word in [-8, 2])."""
    rng = np.random.default_rng(seed + 977)
    rows, V = S['n_img'] * S['beam'], S['V']
    x = grid_rows(rng, rows, V, -8.0, 2.0) if S['grid'] else exact_rows(rng, rows, V, hot, -160.0, -137.0)
    top = 8.0 if S['grid'] else -128.0                # above every planted value: a word left unmasked would win
    for r in range(rows):
        for v, w in zip(S['top_val'][r], S['top_idx'][r]):
            x[r, w] = v
        x[r, [PAD, SOS, UNK, S['last_in'][r]]] = top
    if not S['grid']:
        x[:, hot] = 0.0
    return x


def scenarios():
    """The steps both the merge and the select are held to (make_step arguments): beams 1, 2, 5, 8 with 37 images of
    every kind in one launch and with one image of each kind, t = 0 with garbage in rows 1.., t = T - 1, len_in == T on
    live parents, T = 1 and T = 70 with lengths on both sides of 64."""
    out = []
    for b, beam in enumerate((1, 2, 5, 8)):
        out.append(dict(seed=10 + b, n_img=37, beam=beam, T=6, t=3))
        for k in range(len(KINDS)):
            out.append(dict(seed=20 + 10 * b + k, n_img=1, beam=beam, T=6, t=2, kinds=KINDS[k:] + KINDS[:k]))
        out.append(dict(seed=60 + b, n_img=5, beam=beam, T=6, t=0, kinds=('live', 'frozen', 'neginf_all')))
    out.append(dict(seed=70, n_img=9, beam=5, T=6, t=5))                                   # t == T - 1
    out.append(dict(seed=71, n_img=9, beam=5, T=6, t=2, lens=[6, 2, 6, 1, 6, 6, 0]))      # len_in == T: no token written
    out.append(dict(seed=72, n_img=3, beam=5, T=1, t=0, kinds=('live', 'frozen')))
    out.append(dict(seed=73, n_img=9, beam=8, T=70, t=66, lens=[0, 63, 64, 69, 65]))
    return out
