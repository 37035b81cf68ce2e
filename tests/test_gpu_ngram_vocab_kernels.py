"""The two consumers of a beam step's ban lists, each alone on inputs whose results are determined bit for bit:

  isc_rows_vocab_banned_fwd (isc_rows_ban)  integer lattice operands (the hi planes of tests/_lattice.py: every product and
      every partial sum is a small integer, exact in fp32 in any order) - the logits are then known in bits and hold
      plenty of ties; the tile candidate lists must equal the masked restatement (value descending, ties to the smaller
      id, a banned word a -inf entry), the statistics and the logits must be the bits of the launch without a list.
  isc_beam_topk_banned  `exact rows` of tests/_beam_ref.py (the float32 normaliser is exactly 1: log-prob == logit), on
      both kernels (V = 70: round-based; V = 10000: tile-selecting): ids and values equal the restatement in bits.

Every row of a launch gets another ban case; one launch without a list and one with all counts zero frame each set.
pytest -m gpu."""
import numpy as np
import pytest
import torch

import _beam_ref as B
import _fwd_ref as R
import _lattice as L
from insenticap_model_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PAD, SOS, EOS, UNK = B.PAD, B.SOS, B.EOS, B.UNK
NEG = float('-inf')
SENT, ISENT = R.SENTINEL, -77
K = 64
N_CASES = 8


def ban_case(case, x, V, tw, last):
    """The ordered ban list of ban case `case` for the row of (raw) values x; tw: the tile width of the consumer."""
    nt = (V + tw - 1) // tw
    tmax = [max(x[j * tw:min(V, (j + 1) * tw)]) for j in range(nt)]
    best_tiles = sorted(range(nt), key=lambda j: (-tmax[j], j))
    amax = [j * tw + int(np.argmax(x[j * tw:min(V, (j + 1) * tw)])) for j in range(nt)]
    if case == 0:                                      # the arg-max of the best tile (the row's best word)
        return [amax[best_tiles[0]]]
    if case == 1:                                      # all but 6 words of the best tile: fewer than 8 survive (9+ bans)
        j = best_tiles[0]
        cols = list(range(j * tw, min(V, (j + 1) * tw)))
        return cols[:2] + cols[8:]
    if case == 2:                                      # the last (partial) tile: its last two words and its arg-max
        return [V - 1, V - 2, amax[nt - 1]]
    if case == 3:                                      # a special and the last word: banned twice over
        return [PAD, int(last), UNK]
    if case == 4:                                      # duplicates
        a, b = amax[best_tiles[0]], amax[best_tiles[min(1, nt - 1)]]
        return [a, a, b, a, b]
    if case == 5:                                      # the arg-max of each of the 12 best tiles, and an id outside [0, V)
        return [amax[j] for j in best_tiles[:12]] + [V + 5]
    if case == 6:                                      # nothing, with the pointers set
        return []
    return [amax[j] for j in best_tiles[:4]] + [4, 5, 6, 7]       # exactly 8: the last entry the lanes hold


def ban_tensors(lists, ld):
    ids = torch.full((len(lists), ld), ISENT, dtype=torch.int64)
    for r, b in enumerate(lists):
        assert len(b) <= ld
        ids[r, :len(b)] = torch.tensor(b, dtype=torch.int64) if b else ids[r, :0]
    return ids.to(DEV), torch.tensor([len(b) for b in lists], dtype=torch.int32).to(DEV)


def banned_set(V, last, extra):
    return B.masked(V, last, PAD, SOS, UNK, 1, 1) | {int(i) for i in extra if 0 <= i < V}


# ------------------------------------------------------------------------------------------------ isc_rows_vocab_fwd
_problems = {}


def vocab_problem(M, V):
    """Integer operands and the exact logits; built once per shape and left unchanged."""
    if (M, V) not in _problems:
        g = L.gen(1000 * M + V)
        h = L.operand(g, M, K, 2)[1].float()
        W = L.operand(g, V, K, 2)[1].float()
        bias = torch.randint(-2, 3, (V,), generator=g).float()
        want = L.expect([((h.double(), torch.zeros(M, K, dtype=L.F64)), (W.double(), torch.zeros(V, K, dtype=L.F64)))],
                        [bias.double()]).float()
        last = torch.randint(4, V, (M,), generator=g)
        _problems[(M, V)] = (h.to(DEV), W.to(DEV), bias.to(DEV), want, last)
    return _problems[(M, V)]


def run_vocab(M, V, beam, ban=None):
    h, W, bias, _, last = vocab_problem(M, V)
    tw = ops.rows_stats_tile(V)
    nt = (V + tw - 1) // tw
    out = dict(pm=torch.full((M, nt), SENT, device=DEV), ps=torch.full((M, nt), SENT, device=DEV),
               pi=torch.full((M, nt), ISENT, device=DEV, dtype=torch.int32), lg=torch.full((M, V), SENT, device=DEV),
               cv=torch.full((M, nt, 8), SENT, device=DEV), ci=torch.full((M, nt, 8), ISENT, device=DEV, dtype=torch.int32))
    x = _lib.RowsExt()
    x.stats_tile, x.beam, x.pad_id, x.sos_id, x.unk_id, x.mask_special, x.decoding_constraint = tw, beam, PAD, SOS, UNK, 1, 1
    last_d = last.to(DEV)
    x.last_word, x.cand_val, x.cand_idx = last_d.data_ptr(), out['cv'].data_ptr(), out['ci'].data_ptr()
    rb = None if ban is None else _lib.RowsBan(ban[0].data_ptr(), ban[1].data_ptr(), ban[0].stride(0))
    ops.rows_vocab_fwd(h, W, bias, out['pm'], out['ps'], out['pi'], x, out['lg'], ban=rb)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def tile_lists(x, tw, banned):
    """[n_tile, 8] (value, id) of one row: the 8 best masked entries per tile, value descending, id ascending."""
    V = len(x)
    nt = (V + tw - 1) // tw
    cv, ci = np.full((nt, 8), NEG, np.float32), np.zeros((nt, 8), np.int32)
    for j in range(nt):
        ent = sorted(((NEG if c in banned else float(x[c]), c) for c in range(j * tw, min(V, (j + 1) * tw))),
                     key=lambda e: (-e[0], e[1]))[:8]
        for s, (v, c) in enumerate(ent):
            cv[j, s], ci[j, s] = v, c
    return cv, ci


@pytest.mark.parametrize('M,shift', [(1, s) for s in range(N_CASES)] + [(5, 0), (5, 3), (8, 0)])
@pytest.mark.parametrize('V', [70, 10000])
def test_rows_vocab_lists_under_a_ban_list(V, M, shift):
    beam = {1: 3, 5: 5, 8: 8}[M]
    _, _, _, want, last = vocab_problem(M, V)
    tw = ops.rows_stats_tile(V)
    assert V != 70 or V % tw                                          # V = 70: a partial last tile
    xs = want.numpy()
    lists = [ban_case((r + shift) % N_CASES, xs[r], V, tw, last[r]) for r in range(M)]
    ld = max(40, tw + 2)
    plain = run_vocab(M, V, beam)
    got = run_vocab(M, V, beam, ban_tensors(lists, ld))
    zero = run_vocab(M, V, beam, ban_tensors([[]] * M, ld))
    assert np.array_equal(plain['lg'], xs)                            # the lattice's promise: exact logits
    for k in ('pm', 'ps', 'pi', 'lg'):                                # untouched by the list, bit for bit
        assert np.array_equal(got[k].view(np.int32), plain[k].view(np.int32)), k
    for k in plain:                                                   # zero bans with the pointers set == no list
        assert np.array_equal(zero[k].view(np.int32), plain[k].view(np.int32)), k
    for r in range(M):
        for out, extra in ((plain, []), (got, lists[r])):
            cv, ci = tile_lists(xs[r], tw, banned_set(V, int(last[r]), extra))
            fin = np.isfinite(cv)
            assert np.array_equal(out['cv'][r].view(np.int32), cv.view(np.int32)), (r, lists[r])
            assert np.array_equal(out['ci'][r][fin], ci[fin]), (r, lists[r])
        if (r + shift) % N_CASES == 1 and V > 70:                     # fewer than 8 survive in that (full) tile
            assert (np.isfinite(got['cv'][r]).sum(axis=1) <= 6).any() and (np.isfinite(plain['cv'][r]).sum(axis=1) == 8).all()
        if (r + shift) % N_CASES == 0 and lists[r][0] not in banned_set(V, int(last[r]), []):
            assert not np.array_equal(got['cv'][r], plain['cv'][r])   # (the list reached the kernel)


def test_rows_vocab_refuses_half_a_list():
    M, V = 1, 70
    h, W, bias, _, last = vocab_problem(M, V)
    tw = ops.rows_stats_tile(V)
    nt = (V + tw - 1) // tw
    buf = torch.zeros(M * nt * 8, device=DEV)
    ibuf = torch.zeros(M * nt * 8 + 64, device=DEV, dtype=torch.int64)
    x, b = _lib.RowsExt(), _lib.RowsBan()
    x.stats_tile, x.beam, x.mask_special = tw, 3, 1
    x.cand_val, x.cand_idx = buf.data_ptr(), ibuf.data_ptr()
    lib = _lib.load()

    def call(ban=b):
        import ctypes
        return lib.isc_rows_vocab_banned_fwd(h.data_ptr(), K, W.data_ptr(), K, bias.data_ptr(), M, V, K, buf.data_ptr(),
                                             buf.data_ptr(), ibuf.data_ptr(), None, 0, ctypes.byref(x),
                                             None if ban is None else ctypes.byref(ban), ops.stream())
    assert call(None) == -1
    b.ids, b.cnt, b.ld = ibuf.data_ptr(), None, 10
    assert call() == -1
    b.ids, b.cnt = None, ibuf.data_ptr()
    assert call() == -1
    b.ids, b.ld = ibuf.data_ptr(), 0
    assert call() == -2
    b.ld, x.beam = 10, 0
    assert call() == -2                                             # a list without tile candidates
    torch.cuda.synchronize()
    assert (buf == 0).all() and (ibuf == 0).all()


# ------------------------------------------------------------------------------------------------ isc_beam_topk_banned
def run_topk(x, V, last, beam, ban):
    rows = x.shape[0]
    xd = torch.from_numpy(x).to(DEV)
    pm, ps, _ = R.tile_stats(torch.from_numpy(np.ascontiguousarray(x[:, :V])))
    pm, ps, lw = pm.to(DEV), ps.to(DEV), torch.tensor(last, dtype=torch.int64).to(DEV)
    tv = torch.full((rows + 1, beam), SENT, device=DEV)
    ti = torch.full((rows + 1, beam), ISENT, device=DEV, dtype=torch.int64)
    if ban is None:
        ops.beam_topk(xd, pm, ps, lw, beam, PAD, SOS, UNK, 1, 1, tv, ti)
    else:
        ops.beam_topk_banned(xd, pm, ps, lw, beam, PAD, SOS, UNK, 1, 1, ban[0], ban[1], tv, ti)
    torch.cuda.synchronize()
    return tv.cpu().numpy(), ti.cpu().numpy()


@pytest.mark.parametrize('rows,shift', [(1, s) for s in range(N_CASES)] + [(5, 0), (5, 3), (8, 0)])
@pytest.mark.parametrize('V', [70, 10000])
def test_topk_under_a_ban_list(V, rows, shift):
    beam = {1: 3, 5: 5, 8: 8}[rows]
    rng = np.random.default_rng(V + 10 * rows)
    x = B.exact_rows(rng, rows, V, PAD)                       # <PAD> (masked) at 0: the normaliser is exactly 1
    last = [int(c) for c in rng.integers(4, V, size=rows)]
    tw = 128 if V > 128 else 16                               # (ban cases think in tiles; the one-tile row gets groups of 16)
    lists = [ban_case((r + shift) % N_CASES, np.where(np.arange(V) == PAD, -200.0, x[r]), V, tw, last[r]) for r in range(rows)]
    ld = 136
    plain = run_topk(x, V, last, beam, None)
    got = run_topk(x, V, last, beam, ban_tensors(lists, ld))
    zero = run_topk(x, V, last, beam, ban_tensors([[]] * rows, ld))
    for a, b in zip(zero, plain):                             # zero bans == isc_beam_topk, sentinel row included
        assert np.array_equal(a, b)
    for r in range(rows):
        for (tv, ti), extra in ((plain, []), (got, lists[r])):
            ban = banned_set(V, last[r], extra)
            order = sorted((c for c in range(V) if c not in ban), key=lambda c: (-float(x[r, c]), c))[:beam]
            assert ti[r].tolist() == order, (r, lists[r])
            assert np.array_equal(tv[r].view(np.int32), x[r, order].view(np.int32)), (r, lists[r])
        if (r + shift) % N_CASES == 0 and lists[r][0] not in banned_set(V, last[r], []):
            assert got[1][r].tolist() != plain[1][r].tolist()         # (the row's best word was banned)
    assert (got[0][rows] == SENT).all() and (got[1][rows] == ISENT).all()


def test_topk_banned_refuses_before_the_launch():
    lib = _lib.load()
    buf = torch.zeros(256, device=DEV)
    ib = torch.zeros(256, device=DEV, dtype=torch.int64)
    p, q = buf.data_ptr(), ib.data_ptr()

    def call(ids, cnt, ld, beam=3):
        return lib.isc_beam_topk_banned(p, 40, p, p, 1, 2, 40, beam, q, PAD, SOS, UNK, 1, 1, ids, cnt, ld, p, q, ops.stream())
    assert call(None, q, 10) == -1 and call(q, None, 10) == -1
    assert call(q, q, 0) == -2 and call(q, q, 10, beam=17) == -2
    torch.cuda.synchronize()
    assert (buf == 0).all() and (ib == 0).all()
