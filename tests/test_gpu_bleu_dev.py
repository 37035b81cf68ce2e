"""BLEU on the device (isc_bleu_dev_score, rewards.DeviceBleu): the kernel against the fixture of the reference's scorer
and against the host library on the same rows - the integer statistics for equality, the scores to 1e-12 RELATIVE
(_bleu_ref.RTOL: BLEU-4 of a short caption is of the order 1e-9 .. 1e-13) -, its edge shapes, the refused shapes, the
orders, a capture into a HIP graph, the device form of the self-critical reward, and `Detector.set_bleu_scorer` in the
eager iterations (host against device scorer), a grouped iteration and a graph-served one.  No test sends an id above
65534 to the device and none provokes a fault: the refusals are host checks."""
import numpy as np
import pytest
import torch

import _bleu_ref as R
from insenticap_model_amd import _lib, ops, rewards, synth

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SOS, EOS = R.SOS, R.EOS
_CACHE = {}


def scorers(order=4):
    if order not in _CACHE:
        host = rewards.Bleu(SOS, EOS, order=order)
        _CACHE[order] = (host, host.to_device(DEV, 65535))
    return _CACHE[order]


def both(hyps, ref_lists, row_div=1):
    """((device scores [N, 4], device stats [N, 10]), (host scores, host stats)); row r against ref_lists[r // row_div]."""
    host, dev = scorers()
    hyps = np.ascontiguousarray(hyps, dtype=np.int64)
    pack = dev.pack_refs(ref_lists)
    stats = torch.full((len(hyps), 10), -7, dtype=torch.int32, device=DEV)
    got = dev.score4(torch.from_numpy(hyps).to(DEV), pack, row_div=row_div, stats=stats)
    torch.cuda.synchronize()
    return (got.cpu().numpy(), stats.cpu().numpy()), (host.score4(hyps, ref_lists, row_div=row_div),
                                                      host.stats(hyps, ref_lists, row_div=row_div))


def check(what, hyps, ref_lists, row_div=1):
    (got, gst), (want, wst) = both(hyps, ref_lists, row_div)
    assert np.array_equal(gst, wst), (what, gst, wst)
    assert np.isfinite(got).all() and (got > 0).all(), what
    assert R.rel_err(got, want) <= R.RTOL, (what, got, want)
    return got, gst


@pytest.mark.parametrize('name', ['small', 'cfg5'])
def test_kernel_matches_the_fixture_and_the_host_library(golden, name):
    hyps, refs, per_row, scores, corpus = R.load_set(golden('bleu'), name)
    assert hyps.shape == {'small': (36, 12), 'cfg5': (1024, 20)}[name]
    (got, gst), (want, wst) = both(hyps, per_row)
    print('BLEUDEV [%s] max relative difference: device - host %.3e, device - fixture %.3e'
          % (name, R.rel_err(got, want), R.rel_err(got, scores)))
    assert np.array_equal(gst, wst)
    assert R.rel_err(got, scores) <= R.RTOL
    assert R.rel_err(got, want) <= R.RTOL
    assert R.rel_err(R.corpus_of(gst), corpus) <= R.RTOL
    # two launches give the same bits (cached references: the second pack comes from the per-image cache)
    host, dev = scorers()
    keys = ['%s/%d' % (name, r % len(refs)) for r in range(len(hyps))]
    d = torch.from_numpy(hyps).to(DEV)
    a, b = dev.score4(d, dev.pack_refs(per_row, keys=keys)), dev.score4(d, dev.pack_refs(per_row, keys=keys))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), got)


def test_edge_rows_against_the_host_library():
    T = 12
    pad = lambda words, Tn=T: list(words) + [0] * (Tn - len(words))
    refs0 = [[SOS, 4, 5, 6, 7, EOS], [SOS, 4, 5, 8, EOS], [SOS, 9, 4, 5, 6, 7, 10, EOS]]
    # <EOS> alone: one word, guess = [1, 0, 0, 0]
    got, st = check('<EOS> alone', [pad([EOS])], [refs0])
    assert st[0].tolist() == [1, 4, 1, 0, 0, 0, 1, 0, 0, 0]
    # T = 1: a word (two words with the appended <EOS>) and <EOS> itself
    got, st = check('T = 1', [[4], [EOS]], [refs0, refs0])
    assert st[:, 0].tolist() == [2, 1] and st[0, 6:].tolist() == [2, 0, 0, 0] and st[0, 2:6].tolist() == [2, 1, 0, 0]
    # a leading <SOS> is dropped
    got, st = check('leading <SOS>', [pad([4, 5, 6, 7, EOS]), pad([SOS, 4, 5, 6, 7, EOS])], [refs0, refs0])
    assert np.array_equal(got[0], got[1]) and st[0].tolist() == [5, 5, 5, 4, 3, 2, 5, 4, 3, 2]
    # T = 63 without <EOS>: 64 words, every lane is live (with and without a leading <SOS>: 63 words then)
    words = [4, 5, 6, 7, 9, 4, 5, 8] * 8
    got, st = check('T = 63, no <EOS>', [words[:63], [SOS] + words[:62]], [refs0, refs0])
    assert st[:, 0].tolist() == [64, 63] and st[0, 2:6].tolist() == [64, 63, 62, 61] and (st[:, 6:9] > 0).all()
    # one repeated word against references that hold it twice and three times: clipped by the max over the references
    refs2 = [[SOS, 7, 7, 5, EOS], [SOS, 7, 7, 7, 6, EOS], [SOS, 5, 6, EOS]]
    got, st = check('one repeated word', [pad([7] * 5 + [EOS]), [7] * T], [refs2, refs2])
    assert st[0].tolist() == [6, 5, 6, 5, 4, 3, 4, 2, 1, 0] and st[1, 6:].tolist() == [4, 2, 1, 0]
    # a closest-length tie (reference lengths testlen - 1 and testlen + 1): the shorter wins; then ratios below 1 (testlen
    # = reflen - 1), just below 1 (testlen = reflen: small > tiny, the penalty is applied) and above 1
    refs3 = [[SOS, 4, 5, 6, EOS], [SOS, 4, 5, 6, 7, 8, EOS]]
    rows = [pad([4, 5, 6, 7, EOS]), pad([4, 5, EOS]), pad([4, 5, 6, EOS]), pad([4, 5, 6, 7, 8, 9, EOS])]
    got, st = check('tie and ratios', rows, [refs3] * 4)
    assert st[:, :2].tolist() == [[5, 4], [3, 4], [4, 4], [7, 6]]
    assert got[1, 0] < 0.75 and 1 - 1e-9 < got[2, 0] < 1.0 and abs(got[0, 0] - 1.0) < 1e-9 and got[3, 0] < 0.9
    # an image with one reference
    check('one reference', [pad([11, 12, 13, EOS]), pad([11, 12, EOS])], [[[SOS, 11, 12, 13, EOS]]] * 2)
    # images whose references cook to more than 64 and more than 128 entries: the second and third hand-round batch; the
    # rows match n-grams of the LAST entries
    rng = np.random.default_rng(17)
    long_a = [int(x) for x in rng.integers(4, 30, size=22)]
    long_b = [int(x) for x in rng.integers(4, 30, size=40)]
    host, _ = scorers()
    assert 64 < len(host.cook_refs([[SOS] + long_a + [EOS]])[0]) <= 128 < len(host.cook_refs([[SOS] + long_b + [EOS]])[0])
    got, st = check('65+ / 129+ entries', [pad(long_a[-11:] + [EOS]), pad(long_b[-11:] + [EOS]), pad(long_b[:12])],
                    [[[SOS] + long_a + [EOS]], [[SOS] + long_b + [EOS]], [[SOS] + long_b + [EOS]]])
    assert st[0, 6:].tolist() == [12, 11, 10, 9] and st[1, 6:].tolist() == [12, 11, 10, 9] and st[2, 9] == 9
    # ids 0 and 65534
    refs5 = [[SOS, 0, 65534, 0, EOS], [SOS, 65534, 65533, EOS]]
    got, st = check('ids 0 and 65534', [pad([0, 65534, 0, EOS]), pad([65534, 0, 65534, 0]), pad([65533, 65534, EOS])],
                    [refs5] * 3)
    assert st[0, 6:].tolist() == [4, 3, 2, 1] and st[2, 6:].tolist() == [3, 0, 0, 0]       # (65533 is another word)
    # N = 1 and N = 5 (the last workgroup partly empty): rows behind the output stay untouched
    g = [pad([4, 5, 6, 7, EOS]), pad([4, 5, 8, EOS]), pad([9, 4, EOS]), pad([10, EOS]), pad([4, 4, 4, EOS])]
    host, dev = scorers()
    for N in (1, 5):
        rows = np.asarray(g[:N], dtype=np.int64)
        out = torch.full((N + 3, 4), -7.0, dtype=torch.float64, device=DEV)
        stats = torch.full((N + 3, 10), -7, dtype=torch.int32, device=DEV)
        dev.score4(torch.from_numpy(rows).to(DEV), dev.pack_refs([refs0] * N), out=out[:N], stats=stats[:N])
        torch.cuda.synchronize()
        assert bool((out[N:] == -7.0).all()) and bool((stats[N:] == -7).all()), N
        assert R.rel_err(out[:N].cpu().numpy(), host.score4(rows, [refs0] * N)) <= R.RTOL
        assert np.array_equal(stats[:N].cpu().numpy(), host.stats(rows, [refs0] * N))
    # row_div = 5 with N = 10: the rows of one image share its references
    rows = g + [pad([7, 7, 5, EOS]), pad([7] * 6 + [EOS]), pad([5, 6, EOS]), pad([SOS, 7, 7, 7, 6, EOS]), pad([6, 5, 7])]
    got, st = check('row_div = 5', rows, [refs0, refs2], row_div=5)
    assert len(set(np.round(got[:, 0], 9))) >= 6


def test_orders_give_the_columns_of_the_four_score_form(golden):
    hyps, refs, per_row, scores, corpus = R.load_set(golden('bleu'), 'small')
    host, dev = scorers()
    pack = dev.pack_refs(per_row)
    d = torch.from_numpy(hyps).to(DEV)
    four = dev.score4(d, pack)
    assert tuple(four.shape) == (len(hyps), 4) and four.dtype == torch.float64
    for order in (1, 2, 3, 4):
        one = scorers(order)[1].score(d, pack)
        assert tuple(one.shape) == (len(hyps),) and torch.equal(one, four[:, order - 1])
    assert R.rel_err(scorers(4)[1].score(d, pack).cpu().numpy(), scores[:, 3]) <= R.RTOL


def test_refused_shapes_write_nothing():
    host, dev = scorers()
    refs = [[SOS, 4, 5, 6, EOS]]
    pack = dev.pack_refs([refs, refs])
    out = torch.full((2, 4), -7.0, dtype=torch.float64, device=DEV)
    stats = torch.full((2, 10), -7, dtype=torch.int32, device=DEV)
    hyp = torch.full((2, 64), 5, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.HipLibraryError, match='ISC_E_SHAPE'):
        dev.score4(hyp, pack, out=out, stats=stats)                                   # T = 64
    with pytest.raises(_lib.HipLibraryError, match='ISC_E_SHAPE'):
        dev.score(hyp, pack, out=out[:, 0].contiguous())
    lib = _lib.load()
    ok = hyp[:, :8].contiguous()

    def call(N=2, T=8, row_div=1, n_img=2, order=0):
        return lib.isc_bleu_dev_score(ok.data_ptr(), N, T, row_div, pack.ent_off.data_ptr(), pack.keys.data_ptr(),
                                      pack.counts.data_ptr(), pack.img_cap_off.data_ptr(), pack.lens.data_ptr(), n_img,
                                      order, SOS, EOS, out.data_ptr(), stats.data_ptr(), None)
    for kw in (dict(N=0), dict(T=0), dict(T=64), dict(row_div=0), dict(order=-1), dict(order=5), dict(n_img=1),
               dict(n_img=0)):
        assert call(**kw) == -2, kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((stats == -7).all())
    assert call() == 0 and call(row_div=2, n_img=1) == 0
    torch.cuda.synchronize()
    assert bool((out > 0).all())
    with pytest.raises(ValueError):
        dev.score(ok, pack, row_div=2)                                                # 2 rows are not 2 images x 2
    with pytest.raises(RuntimeError):
        dev.pack_refs([refs, []])                                                     # an image without references
    with pytest.raises(ValueError):
        host.to_device(DEV, 65536)


def test_score_is_capturable(golden):
    """One capture of DeviceBleu.score4 into a HIP graph, replayed on new tokens, gives the eager bits."""
    hyps, refs, per_row, scores, corpus = R.load_set(golden('bleu'), 'small')
    host, dev = scorers()
    n = len(refs)
    pack = dev.pack_refs(refs)
    first, second = torch.from_numpy(hyps[:n]).to(DEV), torch.from_numpy(hyps[n:2 * n]).to(DEV)
    eager_a, eager_b = dev.score4(first, pack).clone(), dev.score4(second, pack).clone()
    rows = first.clone()
    out = torch.zeros(n, 4, dtype=torch.float64, device=DEV)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        dev.score4(rows, pack, out=out)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            dev.score4(rows, pack, out=out)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_a)
    rows.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_b) and not torch.equal(eager_a, eager_b)


def test_self_critical_reward_on_the_device(golden):
    hyps, refs, per_row, scores, corpus = R.load_set(golden('bleu'), 'cfg5')
    host, dev = scorers()
    I = len(refs)
    fns = ['f%d' % i for i in range(I)]
    gt = dict(zip(fns, refs))
    sample, greedy = hyps[:I], hyps[I:]
    want = rewards.get_self_critical_reward(sample, greedy, fns, gt, SOS, EOS, host).astype('float32')
    pack = dev.pack_refs(refs, keys=fns)
    got = rewards.get_self_critical_reward_device(torch.from_numpy(sample).to(DEV), torch.from_numpy(greedy).to(DEV),
                                                  pack, dev)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == sample.shape and got.is_contiguous()
    got = got.cpu().numpy()
    assert (got == got[:, :1]).all()                                  # repeated over T
    # the host form followed by .astype('float32'): the fp64 differences agree to 1e-12 of the larger score, far inside
    # the float32 rounding - at most the last float32 bit can differ
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    assert np.abs(want).max() > 0.3


# ------------------------------------------------------------------------------------------------ Detector
def _give_back(det):
    """Hand the detector's private streams back now: its training graphs' four and the captioner's roll-out stream.  They
    would go with the objects, but a captioner that has trained can outlive its detector by many tests (autograd keeps it
    alive), and the pool the package draws private streams from has 32 per device for the whole suite."""
    torch.cuda.synchronize()
    if det.__dict__.get('_rl_graph') is not None:
        det._rl_graph.close()
    cap = det.captioner
    st = cap.__dict__.pop('_ro_stream', None)
    if st is not None:
        cap.enable_rollout_graphs(False)
        ops.release_stream_state(DEV.index, st.cuda_stream)


def _run_detector(flag, calls, order=4):
    """A fresh detector at the tiny dimensions of tests/test_detector.py (same weights every time) with set_bleu_scorer,
    device_cider = flag, then the calls in order, each behind the same seed.  With the flag on the host scorer's
    score_arrays raises: it must not be called.  Returns (dicts, the largest BLEU-`order` of any rolled-out row)."""
    from test_gpu_cider_dev import _detector
    V, TN, B = 64, 8, 4
    st = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
    batches, split = synth.make_rl_batches(2, B, V, st, seq_len=TN, seed=70)
    t = torch.from_numpy
    fact = [(b[0], t(b[1]), t(b[2]), (t(b[3][0]), b[3][1]), t(b[4]), t(b[5]), b[6]) for b in batches]
    s = synth.make_inputs(4, V, st, regions=6, seq_len=TN, seed=72)
    scs = [((t(s['captions']), s['lengths']), t(s['cpt_words']), t(s['senti_words']), t(s['senti_labels']))]
    torch.manual_seed(0)
    det = _detector(V, TN, st)
    det.set_bleu_scorer(order)
    assert isinstance(det.ciderd_scorer, rewards.Bleu) and det.ciderd_scorer.order == order
    det.device_cider = flag
    host_score = det.ciderd_scorer.score_arrays
    if flag:
        def never(*a, **k):
            raise AssertionError('the host BLEU scorer was called with device_cider on')
        det.ciderd_scorer.score_arrays = never
    rolled = []
    orig = det.captioner.forward_rl

    def spy(*args, **kw):
        out = orig(*args, **kw)
        rolled.append(out[0].detach().cpu().numpy().copy())
        return out
    det.captioner.forward_rl = spy
    outs = []
    for training, n in calls:
        det.rl_samples_per_image, det.train_graphs = n, False
        torch.manual_seed(1234)
        torch.cuda.manual_seed_all(1234)
        outs.append(det((fact, scs) if training else (fact,), 'fact', training))
        torch.cuda.synchronize()
    assert det._rl_graph is None                                     # every call ran the eager sequence
    if flag:
        assert isinstance(det._cider_dev[2], rewards.DeviceBleu)
    _give_back(det)
    top = 0.0
    for i, toks in enumerate(rolled):                                # (roll-outs alternate over the two batches' images)
        for b in fact:
            if toks.shape[0] % len(b[0]) == 0:
                n = toks.shape[0] // len(b[0])
                top = max(top, float(host_score(toks, [b[6][fn] for fn in b[0] for _ in range(n)]).max()))
    return outs, top


def test_detector_takes_the_bleu_reward_from_the_host_and_the_device_scorer():
    """One 'fact' training iteration and one evaluation call with set_bleu_scorer(), two batches of 4 images each, with
    device_cider off and on.  With S the largest BLEU-4 of any rolled-out row (against either batch's references: an upper
    bound), every row's reward is a float32 of magnitude <= S whose fp64 source differs by 1e-12 relative at most, so the
    two float32 values differ by one ulp <= 2^-23 S at most; each fp32 mean of 4 rows adds 3 additions and a division,
    <= 4 x 2^-24 S per side: |difference of fact_reward| <= 5 x 2^-23 S.  cap_loss within 1e-5 relative, as the CIDEr-D
    test holds it."""
    calls = [(True, 1), (False, 1)]
    (off, top), (on, top_on) = _run_detector(False, calls), _run_detector(True, calls)
    assert top == top_on and 0 < top <= 1.0
    for a, b in zip(off, on):
        assert set(a) == set(b) and 'fact_reward' in b
        print('BLEUDEV detector: S = %.3e' % top, a, b)
        assert abs(a['fact_reward'] - b['fact_reward']) <= 5 * 2.0 ** -23 * top
        assert abs(a['cap_loss'] - b['cap_loss']) <= 1e-5 * abs(a['cap_loss'])


def test_detector_grouped_iteration_with_a_bleu_scorer():
    """A grouped rl_samples_per_image = 3 training iteration (BLEU-2) runs with the host and with the device scorer:
    sample_score is an fp64 mean of scores that agree to 1e-12 relative; the advantages are differences of scores <= 1
    that agree to 1e-12, so their mean (0 up to rounding) agrees to 2e-12 - held to 4e-12."""
    (goff,), _ = _run_detector(False, [(True, 3)], order=2)
    (gon,), _ = _run_detector(True, [(True, 3)], order=2)
    assert set(goff) == set(gon) and 'sample_score' in gon and all(np.isfinite(v) for v in gon.values())
    print('BLEUDEV detector grouped:', goff, gon)
    assert gon['sample_score'] > 0 and abs(goff['sample_score'] - gon['sample_score']) <= 1e-12 * goff['sample_score']
    assert abs(goff['fact_reward'] - gon['fact_reward']) <= 4e-12
    assert abs(goff['cap_loss'] - gon['cap_loss']) <= 1e-5 * abs(goff['cap_loss'])


def test_detector_rebuilds_the_twin_when_the_scorer_is_replaced():
    from insenticap_model_amd.detector import Detector
    st = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
    det = Detector(synth.make_idx2word(64), 8, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-4}, st).to(DEV)
    _, split = synth.make_rl_batches(1, 4, 64, st, seq_len=8, seed=70)
    det.set_ciderd_scorer(split)
    det.device_cider = True
    assert isinstance(det._device_ciderd(DEV, 8), rewards.DeviceCiderD)
    det.set_bleu_scorer()
    twin = det._device_ciderd(DEV, 8)
    assert isinstance(twin, rewards.DeviceBleu) and twin.host is det.ciderd_scorer and det._device_ciderd(DEV, 63) is twin
    with pytest.warns(UserWarning, match='host BLEU'):
        assert det._device_ciderd(DEV, 64) is None
    det.set_ciderd_scorer(split)
    assert isinstance(det._device_ciderd(DEV, 8), rewards.DeviceCiderD)


def test_graph_served_iteration_equals_the_eager_one(monkeypatch):
    """With a `Bleu` set the graph-served 'fact' iteration (train_graph.RLTrainGraph reaches the scorer only through
    self_critical_scores) against the same phases never captured - bit for bit - and against the plain eager iteration -
    within the rounding of another order of the gradient sum -, as tests/test_gpu_rl_graph.py compares them for CIDEr-D:
    forced draws, scheduled sampling off."""
    import test_gpu_rl_graph as G
    from insenticap_model_amd.train_graph import RLTrainGraph
    monkeypatch.setenv('ISC_PAIR_UNROLLS', '0')
    items, scs, split, draws = G.data(1)

    def run(det):
        det.set_bleu_scorer()
        det.xe_ss_prob = det.seq2seq_ss_prob = 0.0
        out = []
        for _ in range(3):
            G.force_draws(det, draws)
            if det.train_graphs and det._rl_graph is None:
                det._rl_graph = RLTrainGraph(det, warmup=det._graph_warmup)
            out.append(det(([items[0]], scs), 'fact', True))
        torch.cuda.synchronize()
        return out
    g, e, p = G.make(graphs=True, warmup=1), G.make(graphs=True, warmup=10 ** 6), G.make(graphs=False)
    og, oe, op_ = run(g), run(e), run(p)
    assert g._rl_graph.captures == 1 and g._rl_graph.replays == 2 and g._rl_graph.eager_steps == 1
    assert e._rl_graph.captures == 0 and e._rl_graph.eager_steps == 3
    G.same_params(g, e)
    for a, b in zip(og, oe):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] == b[k], k
    for a, c in zip(og, op_):
        for k in a:
            np.testing.assert_allclose(a[k], c[k], rtol=2e-4, atol=2e-6, err_msg=k)
    for det in (g, e, p):
        _give_back(det)
