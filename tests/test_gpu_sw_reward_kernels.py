"""isc_sw_reward / isc_sw_decay alone against the numpy restatement of tests/_sw_ref.py, in bits: reward_io, reward64,
row_hits and state over row counts around the four rows of a workgroup, lengths around the 64 lanes of a wave, vocabularies
from one word to the product's 10 000 and one or three labels; ids and labels outside their ranges; weights 0.0 and
negative; absent outputs; the accumulating form against torch's float32 expression on the CPU; marks over two launches and
the decay against the Python loop; refused shapes; one capture of reward + decay.  pytest -m gpu."""
import numpy as np
import pytest
import torch

import _sw_ref as S
from insenticap_model_amd import _lib, ops, rewards

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NS, TS = (1, 4, 5, 9), (1, 20, 63, 64, 65, 130)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def lexicon(V, n_labels, seed):
    """Per label about a third of the words, weights 0.9 ** k by repeated multiplication; where the vocabulary has room:
    word 2 in every lexicon, a word of weight 0.0 and one of negative weight."""
    rng = np.random.default_rng(seed)
    pw = S.powers(0.9, 12)
    lex = {}
    for lab in range(n_labels):
        words = rng.choice(V, size=max(1, V // 3), replace=False)
        lex[lab] = {int(w): pw[int(rng.integers(0, 12))] for w in words}
        if V > 2:
            lex[lab][2] = pw[3 + lab]
        if V >= 7:
            lex[lab][4], lex[lab][5] = 0.0, -0.75
    return lex


def rows(N, T, V, n_labels, seed):
    """Token rows with ids -1, V and 2 ** 32 + 2 among them and, from four rows on, labels -1, n_labels and 2 ** 32."""
    rng = np.random.default_rng(seed)
    tok = rng.integers(0, V, size=(N, T)).astype(np.int64)
    flat = tok.reshape(-1)
    for at, bad in zip(rng.permutation(flat.size)[:3], (-1, V, 2 ** 32 + 2)):
        flat[at] = bad
    labels = rng.integers(0, n_labels, size=N).astype(np.int64)
    if N >= 4:
        labels[1:4] = (-1, n_labels, 2 ** 32)
    return tok, labels


def launch(tok, labels, weights, state, flag=0.0, base=None, accumulate=False, mark=True, want=('io', '64', 'hits')):
    """One launch on fresh device copies -> (reward_io, reward64, row_hits, state) as numpy (None where not asked for)."""
    N, T = tok.shape
    d_w, d_s = dev(weights), dev(state)
    io = r64 = hits = None
    if 'io' in want:
        io = dev(base) if base is not None else torch.full((N, T), -7.0, dtype=torch.float32, device=DEV)
    if '64' in want:
        r64 = torch.full((N, T), -7.0, dtype=torch.float64, device=DEV)
    if 'hits' in want:
        hits = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    ops.sw_reward(dev(tok), dev(labels), d_w, d_s, flag, io, accumulate, r64, hits, mark)
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_w.cpu().numpy()), bits(weights))             # the weights are read only
    return tuple(None if x is None else x.cpu().numpy() for x in (io, r64, hits)) + (d_s.cpu().numpy(),)


def same(got, want, what):
    for g, w, name in zip(got, want, ('reward_io', 'reward64', 'row_hits', 'state')):
        if g is not None:
            assert g.dtype == w.dtype and np.array_equal(bits(g), bits(w)), (what, name)


@pytest.mark.parametrize('n_labels', [1, 3])
@pytest.mark.parametrize('V', [1, 7, 64, 10000])
def test_reward_in_bits_over_the_shapes(V, n_labels):
    weights, state = S.table(lexicon(V, n_labels, seed=V + n_labels), V, n_labels)
    paid = nan_rows = 0
    for N in NS:
        for T in TS:
            tok, labels = rows(N, T, V, n_labels, seed=1000 * N + T)
            want = S.reward(tok, labels, weights, state)
            same(launch(tok, labels, weights, state), want, (N, T))
            paid += int((want[2] > 0).sum())
            nan_rows += int((want[2] == -1).sum())
            # the accumulating form on a random base, mark = 0: the state stays as it is
            base = np.random.default_rng(N + T).standard_normal((N, T)).astype(np.float32)
            want = S.reward(tok, labels, weights, state, 0.05, base, accumulate=True, mark=False)
            got = launch(tok, labels, weights, state, 0.05, base, accumulate=True, mark=False)
            same(got, want, (N, T, 'accumulate'))
            assert np.array_equal(got[3], state)
    assert paid > 20 and nan_rows == 3 * 3 * len(TS)


def test_ids_and_labels_outside_their_ranges_and_odd_weights():
    V, n_labels = 64, 3
    lex = lexicon(V, n_labels, seed=9)
    weights, state = S.table(lex, V, n_labels)
    tok = np.asarray([[-1, V, 2 ** 32 + 2, 2, 4, 5, -2 ** 63, 2 ** 63 - 1, 2 ** 32 + V, 0]], dtype=np.int64)
    want = S.reward(tok, [1], weights, state)
    assert (want[1][0, :3] == 0).all() and want[1][0, 3] == lex[1][2] and want[2][0] == 3 + (0 in lex[1])
    assert want[1][0, 4] == 0.0 and want[1][0, 5] == -0.75 and (want[3][1, [4, 5]] == 2).all()    # paid as stored, marked
    same(launch(tok, np.asarray([1]), weights, state), want, 'ids')
    for bad in (-1, n_labels, 2 ** 32, 2 ** 32 + 1, -2 ** 63):                # a single row of a label outside the table
        got = launch(tok, np.asarray([bad]), weights, state)
        assert np.isnan(got[0]).all() and np.isnan(got[1]).all() and got[2][0] == -1 and np.array_equal(got[3], state)
        same(got, S.reward(tok, [bad], weights, state), bad)
    # every row and every position hits the same word
    tok = np.full((9, 65), 2, dtype=np.int64)
    want = S.reward(tok, np.zeros(9, dtype=np.int64), weights, state)
    assert (want[2] == 65).all() and int((want[3] == 2).sum()) == 1
    same(launch(tok, np.zeros(9, dtype=np.int64), weights, state), want, 'one word')


def test_each_optional_output_absent():
    V, n_labels = 64, 3
    weights, state = S.table(lexicon(V, n_labels, seed=4), V, n_labels)
    tok, labels = rows(5, 20, V, n_labels, seed=8)
    want = S.reward(tok, labels, weights, state)
    for outs in (('64', 'hits'), ('io', 'hits'), ('io', '64'), ('hits',), ()):
        same(launch(tok, labels, weights, state, want=outs), want, outs)


def test_accumulate_gives_the_bits_of_torchs_float32_expression():
    """4096 elements, base standard-normal, weights 0.9 ** k, flag 0.05: `base + 0.05 * sw` on float32 CPU tensors.
    tests/test_sw_reward_host.py shows that a contracted multiply-add would differ in 186 of them."""
    base, k, pw = S.accumulate_case()
    weights, state = pw[None, :].copy(), np.ones((1, 12), dtype=np.uint8)
    tok = k.reshape(64, 64).astype(np.int64)
    base = base.reshape(64, 64)
    sw = torch.from_numpy(pw[k].reshape(64, 64)).float()
    want = (torch.from_numpy(base) + 0.05 * sw).numpy()
    got = launch(tok, np.zeros(64, dtype=np.int64), weights, state, 0.05, base, accumulate=True)
    assert np.array_equal(bits(got[0]), bits(want))
    assert np.array_equal(bits(got[1]), bits(pw[k].reshape(64, 64)))
    # without `accumulate` the flag is not applied: (float)w, what torch.from_numpy(r).float() gives
    got = launch(tok, np.zeros(64, dtype=np.int64), weights, state, 0.05, base)
    assert np.array_equal(bits(got[0]), bits(sw.numpy()))


def test_marks_accumulate_over_two_launches_and_decay_in_bits():
    V, n_labels = 64, 3
    lex = lexicon(V, n_labels, seed=6)
    table = rewards.SentimentWordWeights.from_dict(lex, V, n_labels, DEV)
    w0, s0 = S.table(lex, V, n_labels)
    loop = {lab: dict(ws) for lab, ws in lex.items()}
    for rnd in range(3):
        state = table.state.cpu().numpy()
        used = {}
        for seed in (rnd, 50 + rnd):
            tok, labels = rows(9, 20, V, n_labels, seed=seed)
            r = table.reward(dev(tok), dev(labels))
            want = S.reward(tok, labels, table.weights.cpu().numpy(), state)
            assert np.array_equal(bits(r.cpu().numpy()), bits(want[0]))
            for lab, ws in S.accur(state, want[3]).items():
                used.setdefault(lab, set()).update(ws)
            state = want[3]
        assert np.array_equal(table.state.cpu().numpy(), state) and sum(len(ws) for ws in used.values()) > 3
        table.decay(0.9)
        for lab, ws in used.items():                               # decoder.py:174-176
            for w in ws:
                loop[lab][w] *= 0.9
        assert table.to_dict() == loop
        assert np.array_equal(table.state.cpu().numpy(), s0)        # back to 1
        before = table.weights.clone()
        table.decay(0.9)                                            # no new hits: nothing changes
        assert torch.equal(before, table.weights) and np.array_equal(table.state.cpu().numpy(), s0)
    assert len({x for ws in loop.values() for x in ws.values()}) > 6
    mine = {lab: dict(ws) for lab, ws in lex.items()}
    assert table.update_dict(mine) == loop


def test_refused_shapes_launch_and_write_nothing():
    V, n_labels = 7, 3
    weights, state = S.table(lexicon(V, n_labels, seed=2), V, n_labels)
    tok, labels = rows(5, 20, V, 1, seed=3)
    d_tok, d_lab, d_w, d_s = dev(tok), dev(labels), dev(weights), dev(state)
    io = torch.full((5, 20), -7.0, dtype=torch.float32, device=DEV)
    r64 = torch.full((5, 20), -7.0, dtype=torch.float64, device=DEV)
    hits = torch.full((5,), -7, dtype=torch.int32, device=DEV)
    lib = _lib.load()

    def call(N=5, T=20, n_labels=n_labels, V=V, tok=d_tok.data_ptr(), lab=d_lab.data_ptr(), w=d_w.data_ptr(),
             s=d_s.data_ptr()):
        return lib.isc_sw_reward(tok, N, T, lab, n_labels, V, w, s, 0.05, io.data_ptr(), 1, r64.data_ptr(),
                                 hits.data_ptr(), 1, None)
    for kw in (dict(N=0), dict(N=-1), dict(T=0), dict(T=-5), dict(n_labels=0), dict(V=0), dict(V=-1)):
        assert call(**kw) == -2, kw
    for kw in (dict(tok=None), dict(lab=None), dict(w=None), dict(s=None)):
        assert call(**kw) == -1, kw
    assert lib.isc_sw_decay(d_w.data_ptr(), d_s.data_ptr(), 0, 0.9, None) == -2
    assert lib.isc_sw_decay(None, d_s.data_ptr(), 21, 0.9, None) == -1
    assert lib.isc_sw_decay(d_w.data_ptr(), None, 21, 0.9, None) == -1
    torch.cuda.synchronize()
    assert bool((io == -7.0).all()) and bool((r64 == -7.0).all()) and bool((hits == -7).all())
    assert np.array_equal(d_s.cpu().numpy(), state) and np.array_equal(bits(d_w.cpu().numpy()), bits(weights))
    with pytest.raises(_lib.HipLibraryError, match='isc_sw_reward failed'):       # (no rows: the wrapper raises)
        ops.sw_reward(torch.zeros(0, 4, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV),
                      d_w, d_s)


def test_one_captured_graph_of_reward_and_decay_replays_the_eager_bits():
    V, n_labels = 64, 3
    lex = lexicon(V, n_labels, seed=12)
    tok, labels = rows(9, 65, V, n_labels, seed=13)
    d_tok, d_lab = dev(tok), dev(labels)
    base = np.random.default_rng(14).standard_normal(tok.shape).astype(np.float32)

    def run(table, io, r64, hits):
        table.reward(d_tok, d_lab, 0.05, io, True, r64, hits)
        table.decay(0.9)

    def outs():
        return dev(base), torch.zeros(tok.shape, dtype=torch.float64, device=DEV), \
            torch.zeros(9, dtype=torch.int32, device=DEV)
    eager = rewards.SentimentWordWeights.from_dict(lex, V, n_labels, DEV)
    e = outs()
    run(eager, *e)
    torch.cuda.synchronize()
    assert not torch.equal(e[0], dev(base)) and int((eager.state == 2).sum()) == 0
    table = rewards.SentimentWordWeights.from_dict(lex, V, n_labels, DEV)
    fresh = (table.weights.clone(), table.state.clone())
    g = outs()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            run(table, *g)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    table.weights.copy_(fresh[0])                                   # (a capture runs nothing; start from the same state)
    table.state.copy_(fresh[1])
    g[0].copy_(dev(base))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(e + (eager.weights, eager.state), g + (table.weights, table.state)):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
    assert not torch.equal(table.weights, fresh[0]) and bool(torch.isnan(g[0][1]).all()) and int(g[2][0]) >= 0
