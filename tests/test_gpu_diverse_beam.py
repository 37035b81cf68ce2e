"""Diverse beam search (beam_groups / diversity) end to end against the fp64 driver of tests/_diverse_beam_ref.py on its
cases (tests/test_diverse_beam_ref_host.py asserts on the CPU that they are decided: at every (step, group) the
neighbouring keys down to the first rejected one are more than 2e-3 apart, fp32 and fp64 select the same tokens - so no
flip allowance here): the tiny golden model (conftest.CASES['tiny']) and the unequal-width set 'h_wide'.

Tokens equal the driver's, token for token; scores within BEAM_SCORE_TOL = 1e-3 (the bound the beam tests hold against
the oracle, tests/test_gpu_widths.py).  Graph-served searches equal the eager ones in bits, two replays are equal in
bits, a few-row search is one graph.  Without the feature every call here raises TypeError.  pytest -m gpu."""
import gc

import numpy as np
import pytest
import torch

import _diverse_beam_ref as D
import _widths as Wd
from insenticap_model_amd import Captioner, ops, synth

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BEAM_SCORE_TOL = 1e-3
PATH_TOL = 2e-4
CONTROLS = ((0, 0), D.TRIGRAM)
_caps = {}


def _cap(name):
    if name not in _caps:
        st, w, _, _, V = D.model(name)
        cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)
        cap.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
        _caps[name] = cap.to(DEV).eval()
    return _caps[name]


@pytest.fixture(scope='module', autouse=True)
def _free_the_models():
    yield
    _caps.clear()
    gc.collect()


def _n():
    return ops._lib.load().isc_rows_launches()


def _inputs(name, pairs):
    """fc, att, words of the searches' images and their labels."""
    d = D.model(name)[2]
    idx = torch.tensor([i for i, _ in pairs])
    fc, att, sw = (Wd.cpu(d, k)[idx].to(DEV) for k in ('fc_feats', 'att_feats', 'senti_words'))
    return fc, att, sw, torch.tensor([l for _, l in pairs], device=DEV)


def _close(got, ref, tol, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    print('%s: max error %.3g (bound %g)' % (what, err, tol))
    assert err <= tol, (what, err, tol)


def _assert_ref(case, control, caps, scores, ids):
    want = D.expected(case, control)
    assert len(want) == len(ids)
    for k, (rc, rs, ri, _) in enumerate(want):
        assert [list(x) for x in ids[k]] == ri, (case, control, k)
        assert caps[k] == rc
        _close(scores[k], rs, BEAM_SCORE_TOL, '%s %r search %d vs the fp64 driver' % (case, control, k))


def _kw(case, control):
    G, lam = D.CASES[case][4:6]
    return dict(beam_groups=G, diversity=lam, no_repeat_ngram=control[0], min_len=control[1])


def _served(cap, call, few):
    """`call` eager, then from graphs: first sight, capture, two replays - all equal in bits; -> the eager result."""
    cap.enable_beam_graphs(False)
    eager = call()
    cap.enable_beam_graphs(True)
    try:
        outs = [call() for _ in range(2)]
        n0 = _n()
        outs += [call() for _ in range(2)]
        assert _n() == n0                                          # (nothing enqueued by the library: served from the graph)
        entries = [e for e in cap._beam_graphs.values() if isinstance(e, tuple)]
        assert len(entries) == 1
        assert entries[0][2].rows_mode == few and (len(entries[0][0]) == 1) == few       # few rows: ONE graph
        assert entries[0][2].div is not None
        for o in outs:
            assert o == eager                                      # graphs on == graphs off, replay == replay: in bits
    finally:
        cap.enable_beam_graphs(False)
    return eager


@pytest.mark.parametrize('control', CONTROLS, ids=['plain', 'trigram_min6'])
@pytest.mark.parametrize('case', ['tiny_one', 'wide_one'])
def test_sample_one_image(case, control):
    """Captioner.sample, beam 6 in 3 groups: 6 rows on the few-row step, one graph."""
    name, _, pairs, beam, G, lam = D.CASES[case]
    cap, T_ = _cap(name), D.model(name)[3]
    fc, att, sw, lab = _inputs(name, pairs)
    cap.enable_beam_graphs(False)
    n0 = _n()
    caps, scores = cap.sample(fc[0], att[0], sw[0], lab, beam, 1, T_, **_kw(case, control))
    torch.cuda.synchronize()
    launched = _n() - n0
    # both models are eligible for the few-row step (equal A = E = W; h_wide: _widths.WIDTHS): five counted launches per step
    few = True
    assert name == 'tiny' or Wd.WIDTHS[name]['rows_step']
    assert launched % 5 == 0 and launched >= 5 * cap.last_beam_steps > 0, (launched, cap.last_beam_steps)
    want = D.expected(case, control)[0]
    assert caps == want[0]
    _close(scores, want[1], BEAM_SCORE_TOL, '%s %r eager vs the fp64 driver' % (case, control))
    out = _served(cap, lambda: cap.sample_batch(fc, att, sw, lab, beam, 1, T_, **_kw(case, control)), few)
    _assert_ref(case, control, *out)
    assert out[0][0] == caps and out[1][0] == scores


@pytest.mark.parametrize('control', CONTROLS, ids=['plain', 'trigram_min6'])
@pytest.mark.parametrize('case', ['tiny_batch', 'wide_batch'])
def test_sample_batch_on_the_general_kernels(case, control):
    name, _, pairs, beam, G, lam = D.CASES[case]
    cap, T_ = _cap(name), D.model(name)[3]
    fc, att, sw, lab = _inputs(name, pairs)
    cap.enable_beam_graphs(False)
    outs = {}
    for share in (False, True):
        n0 = _n()
        outs[share] = cap.sample_batch(fc, att, sw, lab, beam, 1, T_, share_image=share, **_kw(case, control))
        torch.cuda.synchronize()
        assert _n() - n0 <= T_                                     # nothing of the few-row step
        _assert_ref(case, control, *outs[share])
    assert outs[True][2] == outs[False][2]
    _close(outs[True][1], outs[False][1], PATH_TOL, '%s shared vs expanded' % case)
    out = _served(cap, lambda: cap.sample_batch(fc, att, sw, lab, beam, 1, T_, **_kw(case, control)), False)
    assert out == outs[False]


@pytest.mark.parametrize('control', CONTROLS, ids=['plain', 'trigram_min6'])
@pytest.mark.parametrize('case', ['tiny_senti', 'wide_senti'])
def test_sample_sentiments(case, control):
    """One image under two labels x beam 4 in 2 groups = 8 rows: the few-row step on both models, one graph."""
    name, _, pairs, beam, G, lam = D.CASES[case]
    cap, T_ = _cap(name), D.model(name)[3]
    fc, att, sw, lab = _inputs(name, pairs[:1])
    labels = torch.tensor([[l for _, l in pairs]], device=DEV)

    def call():
        return cap.sample_sentiments(fc, att, sw, labels, beam, 1, T_, **_kw(case, control))
    cap.enable_beam_graphs(False)
    n0 = _n()
    caps, scores, ids = call()
    torch.cuda.synchronize()
    launched = _n() - n0
    assert launched % 5 == 0 and launched >= 5 * cap.last_beam_steps > 0, (launched, cap.last_beam_steps)
    few = True
    assert cap.last_beam_region_entries == 1
    _assert_ref(case, control, caps[0], scores[0], ids[0])
    assert _served(cap, call, few) == (caps, scores, ids)


def test_one_group_is_the_call_without_the_keywords(monkeypatch):
    """beam_groups = 1 (any diversity): same results in bits, same launches, one graph entry, and the group entry points
    are never reached; with groups they are, under a key of their own."""
    name = D.WIDTH_SET                                             # (one image: the few-row step and its select)
    cap = _cap(name)
    T_ = D.model(name)[3]

    def boom(*a, **k):
        raise AssertionError('one group reached a group entry point')
    real = ops.beam_merge_groups, ops.beam_select_groups
    calls = []
    for pairs, beam in ((D.CASES['wide_one'][2], 6), (D.CASES['wide_batch'][2], 6)):
        fc, att, sw, lab = _inputs(name, pairs)
        cap.enable_beam_graphs(False)
        monkeypatch.setattr(ops, 'beam_merge_groups', boom)
        monkeypatch.setattr(ops, 'beam_select_groups', boom)
        n0 = _n()
        ref = cap.sample_batch(fc, att, sw, lab, beam, 1, T_)
        torch.cuda.synchronize()
        base = _n() - n0
        for kw in (dict(beam_groups=1), dict(beam_groups=1, diversity=0.75), dict(diversity=2)):
            n1 = _n()
            assert cap.sample_batch(fc, att, sw, lab, beam, 1, T_, **kw) == ref
            torch.cuda.synchronize()
            assert _n() - n1 == base
        cap.enable_beam_graphs(True)
        try:
            for k in range(4):
                kw = {} if k % 2 else dict(beam_groups=1, diversity=0.5)
                assert cap.sample_batch(fc, att, sw, lab, beam, 1, T_, **kw) == ref
            assert len(cap._beam_graphs) == 1
            monkeypatch.setattr(ops, 'beam_merge_groups', lambda *a: (calls.append('merge'), real[0](*a))[1])
            monkeypatch.setattr(ops, 'beam_select_groups', lambda *a: (calls.append('select'), real[1](*a))[1])
            cap.sample_batch(fc, att, sw, lab, beam, 1, T_, beam_groups=3, diversity=0.5)
            cap.sample_batch(fc, att, sw, lab, beam, 1, T_, beam_groups=3, diversity=0.25)
            assert len(cap._beam_graphs) == 3                      # (G, lambda) is part of the key
        finally:
            cap.enable_beam_graphs(False)
    assert 'merge' in calls and 'select' in calls


@pytest.mark.parametrize('case', ['tiny_one', 'wide_one'])
def test_zero_diversity_groups_are_plain_beams(case):
    """lambda = 0: each group's captions are sample(beam_size = beam / G)'s (the fp64 driver's gaps at lambda = 0 are
    above the margin for these images: test_diverse_beam_ref_host.py)."""
    name, _, pairs, beam, G, _ = D.CASES[case]
    cap, T_ = _cap(name), D.model(name)[3]
    fc, att, sw, lab = _inputs(name, pairs)
    cap.enable_beam_graphs(False)
    bp = beam // G
    caps, scores = cap.sample(fc[0], att[0], sw[0], lab, beam, 1, T_, beam_groups=G, diversity=0.0)
    plain, pscores = cap.sample(fc[0], att[0], sw[0], lab, bp, 1, T_)
    for g in range(G):
        assert caps[g * bp:(g + 1) * bp] == plain
        _close(scores[g * bp:(g + 1) * bp], pscores, PATH_TOL, '%s group %d vs beam %d' % (case, g, bp))


def test_value_errors():
    name = 'tiny'
    cap = _cap(name)
    T_ = D.model(name)[3]
    fc, att, sw, lab = _inputs(name, ((0, 0),))
    cap.enable_beam_graphs(False)
    n0 = _n()
    for kw in (dict(beam_groups=4), dict(beam_groups=0), dict(beam_groups=-1), dict(beam_groups=2.0), dict(beam_groups=True),
               dict(beam_groups=None), dict(beam_groups=2, diversity=-0.5), dict(beam_groups=2, diversity=float('inf')),
               dict(beam_groups=2, diversity=float('nan')), dict(beam_groups=2, diversity=None), dict(diversity='1')):
        with pytest.raises(ValueError):
            cap.sample_batch(fc, att, sw, lab, 6, 1, T_, **kw)
        with pytest.raises(ValueError):
            cap.sample(fc[0], att[0], sw[0], lab, 6, 1, T_, **kw)
        with pytest.raises(ValueError):
            cap.sample_sentiments(fc, att, sw, torch.tensor([[0, 1]], device=DEV), 6, 1, T_, **kw)
    with pytest.raises(ValueError, match='not built'):
        cap.sample_batch(fc, att, sw, lab, 9, 1, T_, beam_groups=3)
    cap.beam_device_merge = False
    try:
        with pytest.raises(ValueError, match='not built'):
            cap.sample_batch(fc, att, sw, lab, 6, 1, T_, beam_groups=2)
    finally:
        del cap.beam_device_merge
    assert not cap.__dict__.get('_beam_graphs')
    torch.cuda.synchronize()
    assert _n() == n0                                              # nothing was launched


def test_detector_passes_the_groups_through():
    from test_gpu_concept import B, ST, TN, V, _detector
    det, cd, table, _ = _detector()
    det.captioner.enable_beam_graphs(False)
    batches, _ = synth.make_rl_batches(1, B, V, ST, seq_len=TN)
    det.set_concept_detector(cd, table, num_concepts=5, num_sentiments=10)
    cats = list(synth.SENTIMENT_CATEGORIES)
    t = torch.from_numpy
    differ = 0
    kw = dict(beam_groups=2, diversity=0.5)
    for i in range(2):
        fc, att = t(batches[0][1][i]).to(DEV), t(batches[0][2][i]).to(DEV)
        derived = det.tag(fc.reshape(1, -1))[1]
        plain, detected = det.sample(fc, att, derived, 4)
        got, detected2 = det.sample(fc, att, derived, 4, **kw)
        assert detected2 == detected
        label = torch.tensor([cats.index(detected[0] if isinstance(detected, (list, tuple)) else detected)],
                             dtype=torch.int64, device=DEV)
        assert got == det.captioner.sample(fc, att, derived, label, 4, 1, det.max_seq_len, **kw)[0]
        differ += got != plain
        both, _ = det.sample_sentiments(fc, att, derived, ['neutral', 'positive'], beam_size=4, **kw)
        for s in ('neutral', 'positive'):
            lab = torch.tensor([cats.index(s)], dtype=torch.int64, device=DEV)
            assert both[s] == det.captioner.sample(fc, att, derived, lab, 4, 1, det.max_seq_len, **kw)[0]
    assert differ                                                  # the groups reach the captions
    with pytest.raises(ValueError):
        det.sample(fc, att, derived, 4, beam_groups=3)
    with pytest.raises(ValueError):
        det.sample_sentiments(fc, att, derived, ['neutral'], beam_size=4, beam_groups=2, diversity=-1.0)
    del det, cd, table
    gc.collect()
