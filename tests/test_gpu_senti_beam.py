"""Beam search of one image under several sentiment labels with the image's tensors shared (Captioner.sample_sentiments,
sample_batch(share_image=True), Detector.sample_sentiments, grouped roll-outs with a label per row), end to end.

Against the fp64 oracle per (image, label): captions and ids equal, scores within BEAM_SCORE_TOL = 1e-3 (the bound of
tests/test_gpu_widths.py) - tests/test_senti_beam_host.py asserts on the CPU that these searches are decided (fp32 and
fp64 oracle agree, neighbouring scores further apart than 2e-3) and that the three labels give three different results,
so a wrong label index cannot pass.  Against the same search on repeated inputs (sample_batch): ids equal, scores within
PATH_TOL = 2e-4 (the path bound of tests/test_gpu_rows.py).  The path - few-row step or general kernels - is asserted by
the launch counter.  pytest -m gpu."""
import gc

import numpy as np
import pytest
import torch

import _senti_beam as SB
import _widths as Wd
from insenticap_model_amd import Captioner, ops, synth

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BEAM_SCORE_TOL = 1e-3
PATH_TOL = 2e-4
LOGP_TOL = 1e-4
T = Wd.T
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
    """The cached captioners (one holds the capture stream of its beam graphs: the pool has 32 per device and the suite's
    other modules keep theirs) go with the module."""
    yield
    _caps.clear()
    gc.collect()


def _inputs(name, images):
    _, _, d, _ = Wd.setup(name)
    return [Wd.cpu(d, k, images).to(DEV) for k in ('fc_feats', 'att_feats', 'senti_words')]


def _close(got, ref, tol, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    print('%s: max error %.3g (bound %g)' % (what, err, tol))
    assert err <= tol, (what, err, tol)


def _repeated(cap, fc, att, sw, labels, beam):
    """The same searches as one sample_batch over inputs repeated S times: [I][S][beam] lists."""
    I, S = labels.shape
    caps, scores, ids = cap.sample_batch(fc.repeat_interleave(S, 0), att.repeat_interleave(S, 0), sw.repeat_interleave(S, 0),
                                         labels.reshape(-1), beam, 1, T)
    return tuple([x[i * S:(i + 1) * S] for i in range(I)] for x in (caps, scores, ids))


def _assert_oracle(name, out, labels, beam):
    caps, scores, ids = out
    for i, row in enumerate(labels.tolist()):
        for s, label in enumerate(row):
            ocaps, osc, oids = SB.oracle(name, i, label, beam)
            assert [list(x) for x in ids[i][s]] == oids, (name, i, label, beam)
            assert caps[i][s] == ocaps
            _close(scores[i][s], osc, BEAM_SCORE_TOL, '%s image %d label %d beam %d vs oracle' % (name, i, label, beam))


@pytest.mark.parametrize('beam', SB.BEAMS)
@pytest.mark.parametrize('name', SB.WIDTH_SETS)
def test_three_images_three_labels_on_the_general_kernels(name, beam):
    """3 images x 3 labels (order rotated per image: the group index is not the label id) x beam rows = 18 / 27 rows."""
    cap = _cap(name)
    cap.enable_beam_graphs(False)
    fc, att, sw = _inputs(name, 3)
    labels = SB.rotated_labels(3).to(DEV)
    n0 = _n()
    out = cap.sample_sentiments(fc, att, sw, labels, beam, 1, T)
    torch.cuda.synchronize()
    launched = _n() - n0
    # general kernels: nothing of the few-row step (5 launches per step); with the fused gate scan one row-kernel scan per step
    fused = Wd.fused_gate_eligible(Wd.WIDTHS[name]['settings'], 9 * beam)
    assert (0 < launched <= T) if fused else launched == 0, (name, launched)
    assert cap.last_beam_region_entries == 3                     # one entry per image, not per row
    assert len(out[0]) == 3 and all(len(x) == 3 and all(len(b) == beam for b in x) for x in out[0])
    _assert_oracle(name, out, labels.cpu(), beam)
    rep = _repeated(cap, fc, att, sw, labels, beam)
    assert cap.last_beam_region_entries == 9 * beam               # (the repeated form: one entry per row)
    assert out[2] == rep[2] and out[0] == rep[0]
    _close(out[1], rep[1], PATH_TOL, '%s beam %d vs repeated inputs' % (name, beam))
    # words given per (image, label), [I, S, M]: the same words under every label is the same call
    out3 = cap.sample_sentiments(fc, att, sw.unsqueeze(1).expand(3, 3, sw.shape[1]).contiguous(), labels, beam, 1, T)
    assert out3 == out


@pytest.mark.parametrize('S,beam', [(2, 3), (2, 4), (3, 2)])
@pytest.mark.parametrize('name', ['h_wide', 'h_768'])
def test_one_image_on_the_few_row_step(name, S, beam):
    cap = _cap(name)
    cap.enable_beam_graphs(False)
    image = 1
    fc, att, sw = (x[image:image + 1] for x in _inputs(name, 3))
    labels = torch.tensor([[(image + s) % 3 for s in range(S)]], dtype=torch.int64, device=DEV)
    n0 = _n()
    caps, scores, ids = cap.sample_sentiments(fc, att, sw, labels, beam, 1, T)
    torch.cuda.synchronize()
    launched = _n() - n0
    assert launched % 5 == 0 and launched >= 5 * cap.last_beam_steps > 0, (launched, cap.last_beam_steps)
    assert cap.last_beam_region_entries == 1
    for s, label in enumerate(labels[0].tolist()):
        ocaps, osc, oids = SB.oracle(name, image, label, beam)
        assert [list(x) for x in ids[0][s]] == oids and caps[0][s] == ocaps, (name, label, beam)
        _close(scores[0][s], osc, BEAM_SCORE_TOL, '%s %dx%d label %d vs oracle' % (name, S, beam, label))
    rep = _repeated(cap, fc, att, sw, labels, beam)
    assert ids == rep[2]
    _close(scores, rep[1], PATH_TOL, '%s %dx%d vs repeated inputs' % (name, S, beam))


@pytest.mark.parametrize('images,beam', [(5, 3), (1, 5)])
@pytest.mark.parametrize('name', ['h_wide', 'all_differ'])
def test_share_image_with_one_label_per_image(name, images, beam):
    cap = _cap(name)
    cap.enable_beam_graphs(False)
    _, _, d, _ = Wd.setup(name)
    fc, att, sw = _inputs(name, images)
    lab = Wd.cpu(d, 'senti_labels', images).to(DEV)
    ref = cap.sample_batch(fc, att, sw, lab, beam, 1, T)
    few = images * beam <= cap.ROWS_STEP_MAX and Wd.WIDTHS[name]['rows_step']
    assert cap.last_beam_region_entries == (images if few else images * beam)      # (the few-row step never expanded)
    out = cap.sample_batch(fc, att, sw, lab, beam, 1, T, share_image=True)
    assert cap.last_beam_region_entries == images
    assert out[2] == ref[2] and out[0] == ref[0]
    _close(out[1], ref[1], PATH_TOL, '%s %d images beam %d shared vs expanded' % (name, images, beam))


def test_graph_serving():
    name = 'h_wide'
    cap = _cap(name)
    fc3, att3, sw3 = _inputs(name, 3)
    fc, att, sw = fc3[:1], att3[:1], sw3[:1]
    la, lb = (torch.tensor([x], dtype=torch.int64, device=DEV) for x in ([0, 1], [2, 0]))
    lab9 = SB.rotated_labels(3).to(DEV)
    cap.enable_beam_graphs(False)
    eager = {k: cap.sample_sentiments(fc, att, sw, l, 3, 1, T) for k, l in (('a', la), ('b', lb))}
    eager9 = cap.sample_sentiments(fc3, att3, sw3, lab9, 3, 1, T)
    assert eager['a'][2] != eager['b'][2]
    cap.enable_beam_graphs(True)
    try:
        for _ in range(3):                                       # first sight (eager), capture, replay
            assert cap.sample_sentiments(fc, att, sw, la, 3, 1, T) == eager['a']       # in bits
        entries = [e for e in cap._beam_graphs.values() if isinstance(e, tuple)]
        assert len(entries) == 1 and len(entries[0][0]) == 1       # ONE graph: 6 rows run on the few-row step
        n0 = _n()
        assert cap.sample_sentiments(fc, att, sw, lb, 3, 1, T) == eager['b']           # other labels: inputs of the same graph
        assert _n() == n0                                           # (a replay: nothing was enqueued by the library)
        assert [e for e in cap._beam_graphs.values() if isinstance(e, tuple)] == entries and len(cap._beam_graphs) == 1
        assert cap.sample_sentiments(fc, att, sw, la, 3, 1, T) == eager['a']
        # the general path (27 rows): graphs of four steps
        for _ in range(3):
            out = cap.sample_sentiments(fc3, att3, sw3, lab9, 3, 1, T)
            assert out[2] == eager9[2] and out[0] == eager9[0]
            _close(out[1], eager9[1], PATH_TOL, 'general path, graph vs eager')
        assert len(cap._beam_graphs) == 2 and all(isinstance(e, tuple) for e in cap._beam_graphs.values())
        # the sharing flag is part of the key: the plain search of the same shapes is another entry
        lab1 = torch.tensor([0], dtype=torch.int64, device=DEV)
        ref = cap.sample_batch(fc, att, sw, lab1, 3, 1, T)
        assert cap.sample_batch(fc, att, sw, lab1, 3, 1, T, share_image=True)[2] == ref[2]
        assert len(cap._beam_graphs) == 4
    finally:
        cap.enable_beam_graphs(False)


@pytest.mark.parametrize('beam', [2, 3])
def test_detector_sample_sentiments_equals_sample_per_label(beam):
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
        for words in (derived, None):
            got, detected = det.sample_sentiments(fc, att, words, None, beam_size=beam)
            assert list(got) == cats and detected == det.sample(fc, att, derived, beam)[1]
            for name in cats:
                label = torch.tensor([cats.index(name)], dtype=torch.int64, device=DEV)
                want, _ = det.captioner.sample(fc, att, derived, label, beam, 1, det.max_seq_len)
                assert got[name] == want, (i, name, beam)
            differ += len({tuple(v) for v in got.values()}) > 1
        sub, _ = det.sample_sentiments(fc, att, derived, ['neutral', 'positive'], beam_size=beam)
        assert list(sub) == ['neutral', 'positive'] and all(sub[k] == got[k] for k in sub)
    assert differ                                                # the label reaches the captions
    del det, cd, table
    gc.collect()                                                 # (the detector's private streams go back to the pool)


@pytest.mark.parametrize('name', ['h_wide', 'all_differ'])
def test_grouped_rollout_with_a_label_per_row(name):
    cap = _cap(name)
    _, _, d, _ = Wd.setup(name)
    I, n = 3, 3
    fc, att, cpt, sw = (Wd.cpu(d, k, I).to(DEV) for k in Wd.RL_KEYS[:4])
    labels = SB.rotated_labels(I, n).to(DEV)                     # [I, n]
    u = torch.rand(I * n, T, generator=torch.Generator().manual_seed(7)).to(DEV)

    def rep(x):
        return x.repeat_interleave(n, 0)
    with torch.no_grad():
        r = cap.forward_rl(rep(fc), rep(att), rep(cpt), rep(sw), labels.reshape(-1), T, 0, _uniforms=u)
        for lab in (labels, labels.reshape(-1)):
            g = cap.forward_rl(fc, att, cpt, sw, lab, T, 0, _uniforms=u, captions_per_image=n)
            assert torch.equal(g[0], r[0]) and torch.equal(g[2], r[2])
            _close(g[1].cpu(), r[1].cpu(), LOGP_TOL, '%s grouped roll-out, label per row: log-probs' % name)
        same = cap.forward_rl(fc, att, cpt, sw, labels[:, 0].contiguous(), T, 0, _uniforms=u, captions_per_image=n)
        assert not torch.equal(same[0], g[0])                    # (one label per image is another roll-out)
    shared = cap.sample_captions(fc, att, cpt, sw, labels, n, T, _uniforms=u, share_image=True)
    plain = cap.sample_captions(fc, att, cpt, sw, labels, n, T, _uniforms=u)
    assert shared == plain
    seq_h, len_h = r[0].cpu().tolist(), r[2].sum(1).long().cpu().tolist()
    assert shared[1] == [[seq_h[i * n + j][:len_h[i * n + j]] for j in range(n)] for i in range(I)]


def test_full_size():
    """DEFAULT_SETTINGS, V = 10000, 36 regions: 1 image x 2 labels x beam 3 from its one graph, 4 images x 3 x 3 = 36 rows on
    the general kernels, against the same searches on repeated inputs."""
    V, st = 10000, synth.DEFAULT_SETTINGS
    cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)
    cap.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=2).items()})
    cap.to(DEV).eval()
    d = {k: torch.from_numpy(np.asarray(v)).to(DEV)
         for k, v in synth.make_inputs(4, V, st, regions=36, seq_len=20, seed=5).items()}
    fc, att, sw = d['fc_feats'], d['att_feats'], d['senti_words']

    def repeated(fc, att, sw, labels):
        I, S = labels.shape
        out = cap.sample_batch(fc.repeat_interleave(S, 0), att.repeat_interleave(S, 0), sw.repeat_interleave(S, 0),
                               labels.reshape(-1), 3, 1, 20)
        return tuple([x[i * S:(i + 1) * S] for i in range(I)] for x in out)
    cap.enable_beam_graphs(False)
    l2 = torch.tensor([[1, 0]], dtype=torch.int64, device=DEV)
    l12 = SB.rotated_labels(4).to(DEV)
    ref2, ref12 = repeated(fc[:1], att[:1], sw[:1], l2), repeated(fc, att, sw, l12)
    n0 = _n()
    out12 = cap.sample_sentiments(fc, att, sw, l12, 3, 1, 20)
    torch.cuda.synchronize()
    assert 0 < _n() - n0 <= 20 and cap.last_beam_region_entries == 4       # general kernels, the row-kernel gate scan
    assert out12[2] == ref12[2]
    _close(out12[1], ref12[1], PATH_TOL, 'full size, 36 rows vs repeated inputs')
    cap.enable_beam_graphs(True)
    for _ in range(3):
        out2 = cap.sample_sentiments(fc[:1], att[:1], sw[:1], l2, 3, 1, 20)
        assert out2[2] == ref2[2]
        _close(out2[1], ref2[1], PATH_TOL, 'full size, 1 x 2 x 3 from the graph vs repeated inputs')
    entries = [e for e in cap._beam_graphs.values() if isinstance(e, tuple)]
    assert len(entries) == 1 and len(entries[0][0]) == 1
    assert len({tuple(map(tuple, x)) for x in out2[2][0]}) == 2   # two labels, two results
    cap.enable_beam_graphs(False)
    del cap, entries
    gc.collect()                                                  # (its capture stream goes back to the pool)
