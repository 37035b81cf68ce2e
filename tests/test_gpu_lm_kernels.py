"""isc_lm_dev_score alone against the fp64 restatement (tests/_lm_ref.py), IN BITS - score, tok_logp, n_scored, n_oov: only
float32 -> float64 conversions and float64 additions in one order are involved.  The cases are those of tests/_lm_cases.py
(the host scorer is held to the same ones in tests/test_lm_host.py): N in {1, 4, 5, 9} x T in {1, 5, 62}, all 64 lanes, a
leading <SOS>, <EOS> at position 0, no <EOS>, garbage behind the <EOS>, orders 1 to 4, every back-off depth with the
contexts present and absent, out-of-vocabulary words scored and in contexts with and without <unk> under both
unk_as_word values, both eos_modes, ids >= V and negative, tables at their tightest capacity, two models adjacent in the
slot array, three labels in one workgroup, labels out of range, no label array, V = 65531.  Then: every optional output
absent, two launches, a HIP-graph capture.  No test sends the kernel anything it does not take: the refusals are host
checks."""
import numpy as np
import pytest
import torch

import _lm_cases as K
from insenticap_model_amd import _lib, rewards

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def device_result(c, guard=3):
    """The kernel's (score, n_scored, n_oov, tok_logp) of a case, with `guard` rows behind every output that must stay
    untouched."""
    dev = K.host_set(c).to_device(DEV)
    hyps = torch.from_numpy(c['hyps']).to(DEV)
    labels = None if c['labels'] is None else torch.from_numpy(c['labels']).to(DEV)
    N, T = hyps.shape
    score = torch.full((N + guard,), -7.0, dtype=torch.float64, device=DEV)
    ns = torch.full((N + guard,), -7, dtype=torch.int32, device=DEV)
    no = torch.full((N + guard,), -7, dtype=torch.int32, device=DEV)
    tok = torch.full((N + guard, T + 2), -7.0, dtype=torch.float64, device=DEV)
    dev.score(hyps, labels, out=score[:N], n_scored=ns[:N], n_oov=no[:N], tok_logp=tok[:N])
    torch.cuda.synchronize()
    assert bool((score[N:] == -7.0).all()) and bool((ns[N:] == -7).all()) and bool((no[N:] == -7).all()), c['name']
    assert bool((tok[N:] == -7.0).all()), c['name']
    return score[:N].cpu().numpy(), ns[:N].cpu().numpy(), no[:N].cpu().numpy(), tok[:N].cpu().numpy()


def check(prefix):
    cs = [c for c in K.build() if c['name'].startswith(prefix)]
    assert cs, prefix
    for c in cs:
        K.same_bits(device_result(c), K.expected(c), c['name'])
    return cs


def test_shapes():
    assert len(check('shape')) == 12
    c, = check('64 positions')
    assert K.expected(c)[1][0] == 64                                  # every lane scored a position


def test_orders_unk_and_eos_modes():
    assert len(check('order')) == 32


def test_hand_built_order_4_model():
    cs = check('hand4')
    assert len(cs) == 4
    seen = set().union(*[K.traces(c) for c in cs])
    # a hit at full order; one, two and three levels with every context present and with none
    assert {(0, 0, 'hit'), (1, 1, 'hit'), (1, 0, 'hit'), (2, 0, 'hit'), (3, 3, 'hit'), (3, 0, 'hit'), (2, 2, 'unk'),
            (2, 2, 'skip'), (3, 3, 'unk'), (3, 0, 'skip')} <= seen


def test_tight_and_adjacent_tables():
    check('tight')
    c, = check('adjacent')
    s = K.host_set(c)
    assert s.lm_off.tolist() == [0, 64] and int((s.slots['key'][:64] != 0).sum()) == 63
    assert s.slots['key'][64] != 0 and s.slots['key'][63] != 0        # a chain ends at the first range's last slot ...
    assert int((s.slots['key'][64:] != 0).sum()) >= 12                # ... and the second one's starts at its first


def test_labels():
    check('one workgroup')
    c, = check('labels out of range')
    want = K.expected(c)
    assert np.isnan(want[0]).sum() == 4 and (want[1] == -1).sum() == 4
    check('no labels')


def test_largest_vocabulary():
    assert len(check('V = 65531')) == 2
    with pytest.raises(ValueError):
        rewards.NgramLMSet([rewards.NgramLM.from_arpa(K.HAND4, 65531)], 65532)


def test_optional_outputs_absent_and_refused_shapes():
    c = K.named('hand4 unk_as_word 1 word')
    dev = K.host_set(c).to_device(DEV)
    hyps = torch.from_numpy(c['hyps']).to(DEV)
    N, T = hyps.shape
    score = torch.full((N,), -7.0, dtype=torch.float64, device=DEV)
    lib = _lib.load()

    def call(N=N, T=T, n_lm=1, V=c['V'], mode=0):
        return lib.isc_lm_dev_score(hyps.data_ptr(), N, T, None, n_lm, dev.slots.data_ptr(), dev.lm_off.data_ptr(),
                                    dev.lm_capacity.data_ptr(), dev.lm_order.data_ptr(), V, mode, 1, c['sos'], c['eos'],
                                    score.data_ptr(), None, None, None, None)
    for kw in (dict(N=0), dict(T=0), dict(T=63), dict(n_lm=0), dict(V=0), dict(V=65532), dict(mode=2), dict(mode=-1)):
        assert call(**kw) == -2, kw
    torch.cuda.synchronize()
    assert bool((score == -7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(score.cpu().numpy().view(np.int64), K.expected(c)[0].view(np.int64))
    with pytest.raises(_lib.HipLibraryError, match='ISC_E_SHAPE'):
        dev.score(torch.zeros(2, 63, dtype=torch.int64, device=DEV))


def test_two_launches_and_a_graph_replay_give_the_eager_bits():
    c = K.named('order 3 unk-in-model 1 unk_as_word 1 word')
    dev = K.host_set(c).to_device(DEV)
    first = torch.from_numpy(c['hyps']).to(DEV)
    second = first.flip(0).contiguous()
    N, T = first.shape

    def run(rows, out=None):
        tok = torch.zeros(N, T + 2, dtype=torch.float64, device=DEV) if out is None else out[3]
        kw = {} if out is None else dict(out=out[0], n_scored=out[1], n_oov=out[2])
        s, a, b = dev.score(rows, None, tok_logp=tok, **kw)
        return s, a, b, tok
    a, b, e2 = run(first), run(first), run(second)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    K.same_bits([x.cpu().numpy() for x in a], K.expected(c), 'eager')
    rows = first.clone()
    outs = (torch.zeros(N, dtype=torch.float64, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV),
            torch.zeros(N, dtype=torch.int32, device=DEV), torch.zeros(N, T + 2, dtype=torch.float64, device=DEV))
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        run(rows, outs)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            run(rows, outs)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(outs, a))
    rows.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(outs, e2)) and not torch.equal(a[0], e2[0])
