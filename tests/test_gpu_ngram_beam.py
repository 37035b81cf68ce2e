"""The beam search under no_repeat_ngram / min_len, end to end against the fp64 restatement of tests/_ngram_beam_ref.py
on its kept cases (tests/test_ngram_beam_ref_host.py asserts on the CPU that they are decided: fp32 and fp64 agree on
the ids, neighbouring final scores at least 2e-3 apart, the controls bind in at least 30 of them).

ids and captions equal; scores within BEAM_SCORE_TOL = 1e-3 (the bound of tests/test_gpu_widths.py).  Two paths of one
search: ids equal, scores within PATH_TOL = 2e-4 (tests/test_gpu_rows.py).  The path - few-row step or general kernels,
eager or replayed - is asserted by the library's launch counter.  pytest -m gpu."""
import gc

import numpy as np
import pytest
import torch

import _ngram_beam_ref as NB
import _widths as Wd
from insenticap_model_amd import Captioner, ops, synth

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BEAM_SCORE_TOL = 1e-3
PATH_TOL = 2e-4
T = NB.T
_caps = {}


def _cap(name):
    if name not in _caps:
        st, w, _, _ = Wd.setup(name)
        cap = Captioner(Wd.idx2word(), synth.SENTIMENT_CATEGORIES, st)
        cap.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
        _caps[name] = cap.to(DEV).eval()
    return _caps[name]


def _n():
    return ops._lib.load().isc_rows_launches()


@pytest.fixture(scope='module', autouse=True)
def _free_the_models():
    yield
    _caps.clear()
    gc.collect()


def _inputs(name, images):
    """fc, att, words, labels (= image index) of the listed images."""
    _, _, d, _ = Wd.setup(name)
    idx = torch.tensor(list(images))
    fc, att, sw = (Wd.cpu(d, k)[idx].to(DEV) for k in ('fc_feats', 'att_feats', 'senti_words'))
    return fc, att, sw, idx.to(DEV)


def _close(got, ref, tol, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    print('%s: max error %.3g (bound %g)' % (what, err, tol))
    assert err <= tol, (what, err, tol)


def _assert_ref(name, images, control, out, labels=None):
    caps, scores, ids = out
    for k, image in enumerate(images):
        rc, rs, ri, _ = NB.run(name, image, control, label=None if labels is None else labels[k])
        assert [list(x) for x in ids[k]] == ri, (name, image, control)
        assert caps[k] == rc
        _close(scores[k], rs, BEAM_SCORE_TOL, '%s image %d %r vs the restatement' % (name, image, control))
        n, min_len = control[:2]
        assert all(NB.repeated_ngrams(w, n) == 0 and (len(w) >= min_len or len(w) == T) for w in ids[k])


def _kw(control):
    return dict(no_repeat_ngram=control[0], min_len=control[1])


def _images_of(name, control, count):
    """`count` images of the kept cases of (name, control), cycled."""
    kept = [i for i in NB.IMAGES if (name, i, control) in NB.CASES]
    return [kept[k % len(kept)] for k in range(count)]


@pytest.mark.parametrize('control', NB.CONTROLS, ids=lambda c: '_'.join(map(str, c)))
@pytest.mark.parametrize('name', NB.WIDTH_SETS)
def test_sample_one_image_eager_and_from_its_graph(name, control):
    """Captioner.sample: the few-row step where the width set has it (ONE graph), the general kernels otherwise."""
    cap = _cap(name)
    n, min_len, dc, beam = control
    few = Wd.WIDTHS[name]['rows_step']
    for image in [i for i in NB.IMAGES if (name, i, control) in NB.CASES]:         # every kept case runs here
        fc, att, sw, lab = _inputs(name, [image])
        cap.enable_beam_graphs(False)
        n0 = _n()
        caps, scores = cap.sample(fc[0], att[0], sw[0], lab, beam, dc, T, **_kw(control))
        torch.cuda.synchronize()
        launched = _n() - n0
        if few:
            assert launched % 5 == 0 and launched >= 5 * cap.last_beam_steps > 0, (launched, cap.last_beam_steps)
        else:
            assert launched <= T
        rc, rs, ri, _ = NB.run(name, image, control)
        assert caps == rc
        _close(scores, rs, BEAM_SCORE_TOL, '%s image %d %r eager vs the restatement' % (name, image, control))
        eager = cap.sample_batch(fc, att, sw, lab, beam, dc, T, **_kw(control))
        assert eager[2][0] == ri
        cap.enable_beam_graphs(True)
        try:
            outs = [cap.sample_batch(fc, att, sw, lab, beam, dc, T, **_kw(control)) for _ in range(2)]   # first sight, capture
            n0 = _n()
            outs += [cap.sample_batch(fc, att, sw, lab, beam, dc, T, **_kw(control)) for _ in range(2)]  # replays
            assert _n() == n0                                      # (nothing enqueued by the library: served from the graph)
            entries = [e for e in cap._beam_graphs.values() if isinstance(e, tuple)]
            assert len(entries) == 1 and (len(entries[0][0]) == 1) == few        # few rows: ONE graph
            for o in outs:
                assert o[2] == eager[2] and o[0] == eager[0]
                _close(o[1], eager[1], PATH_TOL, '%s image %d %r graph vs eager' % (name, image, control))
            assert outs[2] == outs[3]                              # the replay is bit-repeatable
        finally:
            cap.enable_beam_graphs(False)


@pytest.mark.parametrize('images,control', [(3, NB.CONTROLS[0]), (3, NB.CONTROLS[1]), (4, NB.CONTROLS[2])],
                         ids=['3x3_bigram', '3x3_trigram_min8', '4x5_trigram'])
@pytest.mark.parametrize('name', NB.WIDTH_SETS)
def test_sample_batch_on_the_general_kernels(name, images, control):
    cap = _cap(name)
    n, min_len, dc, beam = control
    imgs = _images_of(name, control, images)
    fc, att, sw, lab = _inputs(name, imgs)
    cap.enable_beam_graphs(False)
    fused = Wd.fused_gate_eligible(Wd.WIDTHS[name]['settings'], images * beam)
    outs = {}
    for share in (False, True):
        n0 = _n()
        outs[share] = cap.sample_batch(fc, att, sw, lab, beam, dc, T, share_image=share, **_kw(control))
        torch.cuda.synchronize()
        launched = _n() - n0
        assert (0 < launched <= T) if fused else launched == 0, (name, launched)     # nothing of the few-row step
        assert cap.last_beam_region_entries == (images if share else images * beam)
        _assert_ref(name, imgs, control, outs[share])
    assert outs[True][2] == outs[False][2]
    _close(outs[True][1], outs[False][1], PATH_TOL, '%s shared vs expanded' % name)
    cap.enable_beam_graphs(True)
    try:
        for k in range(3):                                         # first sight, capture, replay
            n0 = _n()
            out = cap.sample_batch(fc, att, sw, lab, beam, dc, T, **_kw(control))
            assert out[2] == outs[False][2] and out[0] == outs[False][0]
            _close(out[1], outs[False][1], PATH_TOL, '%s graph-served vs eager' % name)
        assert _n() == n0
        entries = [e for e in cap._beam_graphs.values() if isinstance(e, tuple)]
        assert len(entries) == 1 and len(entries[0][0]) == (T + 3) // 4         # graphs of four steps
    finally:
        cap.enable_beam_graphs(False)


@pytest.mark.parametrize('S', [2, 3])
@pytest.mark.parametrize('control', NB.SENTI_CONTROLS, ids=lambda c: '_'.join(map(str, c)))
@pytest.mark.parametrize('name', NB.WIDTH_SETS)
def test_sample_sentiments_with_rotated_labels(name, control, S):
    """1 image x 2 labels x beam 3 = 6 rows (the few-row step where the width set has it), 1 x 3 x 3 = 9 rows (general)."""
    cap = _cap(name)
    cap.enable_beam_graphs(False)
    n, min_len, dc, beam = control
    image = NB.SENTI_IMAGE
    fc, att, sw, _ = _inputs(name, [image])
    labels = [(image + 1 + s) % 3 for s in range(S)]                # rotated: the group index is not the label id
    n0 = _n()
    caps, scores, ids = cap.sample_sentiments(fc, att, sw, torch.tensor([labels], device=DEV), beam, dc, T, **_kw(control))
    torch.cuda.synchronize()
    launched = _n() - n0
    if S * beam <= cap.ROWS_STEP_MAX and Wd.WIDTHS[name]['rows_step']:
        assert launched % 5 == 0 and launched >= 5 * cap.last_beam_steps > 0, (launched, cap.last_beam_steps)
    else:
        assert launched <= T
    assert cap.last_beam_region_entries == 1
    _assert_ref(name, [image] * S, control, (caps[0], scores[0], ids[0]), labels)


def test_defaults_are_the_call_without_the_keywords(monkeypatch):
    """no_repeat_ngram = 0, min_len = 0: same results, same launches, one graph entry for both spellings, and the new
    entry points are never reached; with a control on they are."""
    name = 'h_wide'
    cap = _cap(name)
    calls = []

    def boom(*a, **k):
        raise AssertionError('the default path reached a ban-list entry point')
    real_ban, real_topk, real_rows = ops.beam_ngram_ban, ops.beam_topk_banned, ops.rows_step_fwd
    rows_bans = []

    def rows_step(plan, ext, ban=None):            # the few-row step's route to isc_rows_step_banned_fwd: ban is not None
        rows_bans.append(ban)
        return real_rows(plan, ext, ban)
    monkeypatch.setattr(ops, 'rows_step_fwd', rows_step)
    for images, beam in ((1, 3), (3, 3)):
        fc, att, sw, lab = _inputs(name, range(images))
        cap.enable_beam_graphs(False)
        monkeypatch.setattr(ops, 'beam_ngram_ban', boom)
        monkeypatch.setattr(ops, 'beam_topk_banned', boom)
        del rows_bans[:]
        n0 = _n()
        ref = cap.sample_batch(fc, att, sw, lab, beam, 1, T)
        torch.cuda.synchronize()
        n1 = _n()
        out = cap.sample_batch(fc, att, sw, lab, beam, 1, T, no_repeat_ngram=0, min_len=0)
        torch.cuda.synchronize()
        assert out == ref and _n() - n1 == n1 - n0
        cap.enable_beam_graphs(True)
        try:
            for k in range(4):
                kw = {} if k % 2 else dict(no_repeat_ngram=0, min_len=0)
                got = cap.sample_batch(fc, att, sw, lab, beam, 1, T, **kw)
                assert got[2] == ref[2]
                _close(got[1], ref[1], PATH_TOL, 'defaults, graph-served')
            assert len(cap._beam_graphs) == 1
            # every few-row step of the default searches went without a list (one image: the few-row path was taken)
            assert all(b is None for b in rows_bans) and (len(rows_bans) > 0) == (images == 1)
            monkeypatch.setattr(ops, 'beam_ngram_ban', lambda g: (calls.append('ban'), real_ban(g))[1])
            monkeypatch.setattr(ops, 'beam_topk_banned', lambda *a: (calls.append('topk'), real_topk(*a))[1])
            cap.sample_batch(fc, att, sw, lab, beam, 1, T, no_repeat_ngram=2)
            assert len(cap._beam_graphs) == 2                      # the controls are part of the key
            if images == 1:
                assert rows_bans and all(b is not None for b in rows_bans[-cap.last_beam_steps:])   # ... and with one on, with it
        finally:
            cap.enable_beam_graphs(False)
    assert 'ban' in calls and 'topk' in calls


def test_value_errors():
    name = 'h_wide'
    cap = _cap(name)
    fc, att, sw, lab = _inputs(name, [0])
    n0 = _n()
    for kw in (dict(no_repeat_ngram=5), dict(no_repeat_ngram=-1), dict(no_repeat_ngram=2.0), dict(no_repeat_ngram=True),
               dict(min_len=T + 1), dict(min_len=-1), dict(min_len=None)):
        with pytest.raises(ValueError):
            cap.sample_batch(fc, att, sw, lab, 3, 1, T, **kw)
        with pytest.raises(ValueError):
            cap.sample(fc[0], att[0], sw[0], lab, 3, 1, T, **kw)
        with pytest.raises(ValueError):
            cap.sample_sentiments(fc, att, sw, torch.tensor([[0, 1]], device=DEV), 3, 1, T, **kw)
    with pytest.raises(ValueError, match='not built'):
        cap.sample_batch(fc, att, sw, lab, 9, 1, T, no_repeat_ngram=3)
    cap.beam_device_merge = False
    try:
        with pytest.raises(ValueError, match='not built'):
            cap.sample_batch(fc, att, sw, lab, 3, 1, T, min_len=4)
    finally:
        del cap.beam_device_merge
    with pytest.raises(ValueError, match='vocabulary'):
        cap.sample_batch(fc, att, sw, lab, 3, 1, Wd.V - 7, no_repeat_ngram=3)      # V <= max_seq_len + 4 + beam
    assert not cap.__dict__.get('_beam_graphs')                      # (no cache entry was marked on the way to a refusal)
    torch.cuda.synchronize()
    assert _n() == n0                                                # nothing was launched


def test_detector_passes_the_controls_through():
    from test_gpu_concept import B, ST, TN, V, _detector
    det, cd, table, _ = _detector()
    det.captioner.enable_beam_graphs(False)
    batches, _ = synth.make_rl_batches(1, B, V, ST, seq_len=TN)
    det.set_concept_detector(cd, table, num_concepts=5, num_sentiments=10)
    cats = list(synth.SENTIMENT_CATEGORIES)
    t = torch.from_numpy
    differ = 0
    for i in range(2):
        fc, att = t(batches[0][1][i]).to(DEV), t(batches[0][2][i]).to(DEV)
        derived = det.tag(fc.reshape(1, -1))[1]
        plain, detected = det.sample(fc, att, derived, 3)
        got, detected2 = det.sample(fc, att, derived, 3, no_repeat_ngram=2, min_len=TN - 2)
        assert detected2 == detected
        label = torch.tensor([cats.index(detected[0] if isinstance(detected, (list, tuple)) else detected)],
                             dtype=torch.int64, device=DEV)
        want, _ = det.captioner.sample(fc, att, derived, label, 3, 1, det.max_seq_len, no_repeat_ngram=2, min_len=TN - 2)
        assert got == want
        differ += got != plain
        both, _ = det.sample_sentiments(fc, att, derived, ['neutral', 'positive'], beam_size=3, no_repeat_ngram=2,
                                        min_len=TN - 2)
        for s in ('neutral', 'positive'):
            lab = torch.tensor([cats.index(s)], dtype=torch.int64, device=DEV)
            assert both[s] == det.captioner.sample(fc, att, derived, lab, 3, 1, det.max_seq_len, no_repeat_ngram=2,
                                                   min_len=TN - 2)[0]
    assert differ                                                    # the controls reach the captions
    with pytest.raises(ValueError):
        det.sample(fc, att, derived, 3, no_repeat_ngram=7)
    del det, cd, table
    gc.collect()
