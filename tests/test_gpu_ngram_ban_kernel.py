"""isc_beam_ngram_ban alone against the rule of tests/_ngram_beam_ref.py (ban_list): the lists equal entry for entry
(order and duplicates included), the counts equal, nothing written behind a list, two runs bit-equal, every refusal of
the header.  pytest -m gpu."""
import ctypes

import pytest
import torch

import _ngram_beam_ref as NB
from insenticap_model_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FILL = -7            # what the ban buffer holds before a launch: entries behind a list must keep it
A, B_, C_, D = 11, 12, 13, 14
EOS, PAD = 2, 0


def _history(kind, r, T, seed=0):
    """T words of row r: the kinds the rule can go wrong on."""
    if kind == 'aaaa':
        return [A] * T
    if kind == 'abab':
        return [A if j % 2 == 0 else B_ for j in range(T)]
    if kind == 'abcab':
        return [(A, B_, C_)[j % 3] for j in range(T)]
    if kind == 'none':                                        # all different: no (n - 1)-gram returns (n >= 2)
        return [20 + j for j in range(T)]
    g = torch.Generator().manual_seed(seed * 131 + r)         # 'random': four ids, many repeats
    return (A + torch.randint(0, 4, (T,), generator=g)).tolist()


def _run(words, lens, T, t, n, min_len, eos=EOS, ld=None, live=None, rows=None):
    rows = len(words) if rows is None else rows
    ld = T if ld is None else ld
    w = torch.tensor(words, dtype=torch.int64).reshape(rows, T).to(DEV)
    ln = torch.tensor(lens, dtype=torch.int32).to(DEV)
    ids = torch.full((rows, ld), FILL, dtype=torch.int64, device=DEV)
    cnt = torch.full((rows,), FILL, dtype=torch.int32, device=DEV)
    g = _lib.BeamNgramBanArgs()
    g.rows, g.T, g.t, g.no_repeat_ngram, g.min_len, g.eos_id, g.ban_ld = rows, T, t, n, min_len, eos, ld
    g.words, g.len, g.ban_ids, g.ban_cnt = w.data_ptr(), ln.data_ptr(), ids.data_ptr(), cnt.data_ptr()
    lv = None
    if live is not None:
        lv = torch.tensor([live], dtype=torch.int32, device=DEV)
        g.live_in = lv.data_ptr()
    ops.beam_ngram_ban(g)
    torch.cuda.synchronize()
    return ids.cpu(), cnt.cpu()


def _check(words, lens, T, t, n, min_len, eos=EOS, ld=None):
    ids, cnt = _run(words, lens, T, t, n, min_len, eos, ld)
    ids2, cnt2 = _run(words, lens, T, t, n, min_len, eos, ld)
    assert torch.equal(ids, ids2) and torch.equal(cnt, cnt2)             # bit-repeatable
    total = 0
    for r, (w, L) in enumerate(zip(words, lens)):
        want = NB.ban_list(w[:min(L, t)], n, t, min_len, eos)
        assert int(cnt[r]) == len(want), (r, n, t, int(cnt[r]), want)
        assert ids[r, :len(want)].tolist() == want, (r, n, t)
        assert (ids[r, len(want):] == FILL).all(), (r, n, t)             # nothing behind the list
        total += len(want)
    return total


@pytest.mark.parametrize('n', [1, 2, 3, 4])
@pytest.mark.parametrize('T', [1, 2, 10, 65, 130])
def test_lists_equal_the_rule(n, T):
    """Live candidates (len == t) of every history kind, at t = 0, n - 2 (too short), n - 1, mid-way, past each 64-lane
    chunk and T - 1; rows 1, 5, 8, 9, 20."""
    kinds = ('aaaa', 'abab', 'abcab', 'none', 'random')
    steps = sorted({s for s in (0, n - 2, n - 1, n, 5, 63, 64, 65, 66, 127, 128, 129, T - 1) if 0 <= s < T})
    found = 0
    for rows in (1, 5, 8, 9, 20):
        words = [_history(kinds[r % len(kinds)], r, T, seed=rows) for r in range(rows)]
        for t in steps:
            found += _check(words, [t] * rows, T, t, n, 0)
    if T > n:
        assert found > 0                                      # (the histories do repeat)


def test_several_bans_and_duplicates():
    T = 10
    ab = _history('abab', 0, T)
    ids, cnt = _run([ab], [6], T, 6, 2, 0)                    # a b a b a b: pre = (b), b -> a twice
    assert cnt.tolist() == [2] and ids[0, :2].tolist() == [A, A]
    ids, cnt = _run([ab], [5], T, 5, 2, 0)                    # a b a b a: pre = (a), a -> b twice
    assert cnt.tolist() == [2] and ids[0, :2].tolist() == [B_, B_]
    ids, cnt = _run([[A] * T], [5], T, 5, 3, 0)               # a a a a a: (a a) -> a at j = 2, 3, 4
    assert cnt.tolist() == [3] and ids[0, :3].tolist() == [A] * 3
    ids, cnt = _run([_history('none', 0, T)], [9], T, 9, 2, 0)
    assert cnt.tolist() == [0] and (ids == FILL).all()


@pytest.mark.parametrize('n', [0, 2])
def test_min_len_bans_eos_up_to_its_last_step(n):
    T = 10
    words = [_history('abab', r, T) for r in range(5)]
    for min_len in (1, 4, 10):
        for t in (min_len - 1, min_len):
            if t < T:
                _check(words, [t] * 5, T, t, n, min_len)
    ids, cnt = _run(words, [3] * 5, T, 3, 0, 4)
    assert cnt.tolist() == [1] * 5 and ids[:, 0].tolist() == [EOS] * 5
    ids, cnt = _run(words, [4] * 5, T, 4, 0, 4)
    assert cnt.tolist() == [0] * 5
    # eos == pad (a vocabulary without a <PAD> of its own): the id is banned all the same
    ids, cnt = _run(words, [3] * 5, T, 3, 2, 4, eos=PAD)
    assert ids[0, :int(cnt[0])].tolist() == NB.ban_list(words[0][:3], 2, 3, 4, PAD) and ids[0, int(cnt[0]) - 1] == PAD


def test_ended_candidates_and_wide_rows():
    """An ended candidate is shorter than t: its list is that of its own words (nobody reads it).  ban_ld > T: rows are
    ban_ld apart."""
    T = 10
    words = [_history('abab', r, T) for r in range(9)]
    lens = [min(r, 7) for r in range(9)]
    _check(words, lens, T, 7, 2, 9)
    _check(words, lens, T, 7, 2, 9, ld=T + 6)
    _check(words, [7] * 9, T, 7, 1, 8, ld=64)


def test_live_in_zero_writes_nothing():
    T = 10
    words = [_history('aaaa', r, T) for r in range(5)]
    ids, cnt = _run(words, [6] * 5, T, 6, 2, 8, live=0)
    assert (ids == FILL).all() and (cnt == FILL).all()
    ids, cnt = _run(words, [6] * 5, T, 6, 2, 8, live=3)
    assert cnt.tolist() == [6] * 5


def test_refusals():
    T = 10
    buf = torch.zeros(64, dtype=torch.int64, device=DEV)
    lib = _lib.load()

    def args():
        g = _lib.BeamNgramBanArgs()
        g.rows, g.T, g.t, g.no_repeat_ngram, g.min_len, g.eos_id, g.ban_ld = 2, T, 3, 3, 4, EOS, T
        g.words = g.len = g.ban_ids = g.ban_cnt = buf.data_ptr()
        return g
    assert lib.isc_beam_ngram_ban(None, None) == -1
    for f in ('words', 'len', 'ban_ids', 'ban_cnt'):
        g = args()
        setattr(g, f, None)
        assert lib.isc_beam_ngram_ban(ctypes.byref(g), None) == -1, f
    for f, bad in (('no_repeat_ngram', -1), ('no_repeat_ngram', 5), ('min_len', -1), ('min_len', T + 1), ('t', -1), ('t', T),
                   ('ban_ld', T - 1)):
        g = args()
        setattr(g, f, bad)
        assert lib.isc_beam_ngram_ban(ctypes.byref(g), None) == -2, (f, bad)
    torch.cuda.synchronize()
    assert (buf == 0).all()
