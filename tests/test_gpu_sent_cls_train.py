"""The sentence-sentiment classifier's training on the library's kernels - train.sent_cls_loss_with_grad /
sent_cls_train_step (isc_sent_cls_train_fwd, isc_sent_cls_bwd), sent_cls_evaluate - against the reference's fixture
(tests/golden/sent_cls_train.npz) and the fp64 restatement tests/_sent_cls_train_ref.py.  pytest -m gpu.

Yardstick, per loss and per gradient: |device - fp64| <= 4 max(e, 2^-23 max|fp64|), e = the stock fp32 module's autograd
error on the CPU against the same fp64 reference (computed here: the bound never comes from the code under test).
Every case's input condition is asserted by tests/test_sent_cls_train_ref_host.py and again here."""
import os

import numpy as np
import pytest
import torch

import _sent_cls_train_cases as Cs
import _sent_cls_train_ref as R
from insenticap_model_amd import checkpoint, ops
from insenticap_model_amd.optim import FusedClampAdam
from insenticap_model_amd.train import sent_cls_evaluate, sent_cls_loss_with_grad, sent_cls_train_step

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sent_cls_train.npz')


def _grads(m):
    return {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()}


def _run(m, tokens, lens, labels, masks=None):
    m.zero_grad()
    loss = sent_cls_loss_with_grad(m, tokens, lens, labels, _keep_masks=masks)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu().numpy().copy(), _grads(m)


def _hold(loss, grads, c, tag=''):
    err, bound = R.yardstick(loss, np.asarray(c['loss']), c['e_loss'])
    print('%s loss: err %.3g  fp32-cpu err %.3g  bound %.3g' % (tag, err, c['e_loss'], bound))
    assert err <= bound, (tag, err, bound)
    for n in R.NAMES:
        err, bound = R.yardstick(grads[n], c['grads'][n], c['e_grads'][n])
        print('   %s grad %s: err %.3g  fp32-cpu err %.3g  bound %.3g' % (tag, n, err, c['e_grads'][n], bound))
        assert err <= bound, (tag, n, err, bound)
    assert not grads[R.NAMES[0]][0].any()                      # the <PAD> row, also with <PAD> at a valid position


@pytest.mark.parametrize('fused', [False, True], ids=['adam', 'fused'])
def test_training_step_vs_the_reference(fused):
    """Two iterations (dropout_p = 0, lr 4e-4, clip 0.1) against what the reference's module, CrossEntropyLoss,
    clip_gradient and Adam gave.  Iteration 1 starts from the fixture's weights - the fixture's loss and gradients are the
    fp32 CPU module's, which is asserted; iteration 2 starts from the weights the device's own first step left, so its
    fp64 reference and its e are computed from exactly those.  "Are the fixture's" is held to 1e-6 of the loss and 1e-5 of
    each gradient's largest element, not to equal bits: the fixture comes from the reference's PACKED forward (the vendor
    LSTM over a PackedSequence), the CPU run here is the masked form of the same module - another summation order in
    fp32, the same numbers otherwise; a wrong term would show at 1e-2 and above.  The parameters after step 2 are held to the fixture in the
    median / fraction form of tests/test_gpu_concept.py, scaled to this learning rate."""
    g = np.load(GOLDEN)
    lr, clip = float(g['hyper'][0]), float(g['hyper'][1])
    tokens, lens, labels = g['tokens'], [int(x) for x in g['lens']], g['labels']
    m = Cs.module(32, 32, 64)[0]
    m.load_state_dict({n: torch.from_numpy(g['sd/' + n]) for n in R.NAMES})
    m.to(DEV).train()
    opt, _ = m.get_optim_and_crit(lr, fused=fused)
    assert isinstance(opt, FusedClampAdam) == fused
    td, ld = torch.from_numpy(tokens).to(DEV), torch.from_numpy(labels).to(DEV)
    for it in range(2):
        now = {n: v.cpu().numpy().copy() for n, v in m.state_dict().items()}
        L64, G64, aux = R.forward_backward(now, tokens, lens, labels)
        assert R.relu_margin(aux) >= 1e-5
        cpu = Cs.module(32, 32, 64)[0]
        cpu.load_state_dict({n: torch.from_numpy(v) for n, v in now.items()})
        eL, eG, g32, L32 = Cs.cpu_error(cpu, now, tokens, lens, labels, L64, G64)
        if it == 0:                                            # the fixture's numbers are this module's
            assert abs(L32 - g['loss'][0]) <= 1e-6 * g['loss'][0]
            for n in R.NAMES:
                ref = g['grad1/' + n]
                assert np.abs(g32[n] - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-9, n
        _, grads = _run(m, td, lens, ld)                       # the gradients as the node gives them, before the clamp
        loss = sent_cls_train_step(m, opt, td, lens, ld, clip)
        assert loss.is_cuda and loss.dim() == 0
        _hold(loss.cpu().numpy(), grads, dict(loss=L64, grads=G64, e_loss=eL, e_grads=eG), 'iteration %d' % (it + 1))
        for n, p in m.named_parameters():
            assert np.array_equal(np.clip(grads[n], -clip, clip), p.grad.cpu().numpy()), n
    for n, v in m.state_dict().items():
        d = np.abs(v.cpu().numpy() - g['after2/' + n])
        assert d.max() <= 2 * 2 * lr * 1.01, n
        assert np.median(d) <= lr / 40, (n, float(np.median(d)))
        assert (d > lr / 10).mean() <= 0.1, (n, float((d > lr / 10).mean()))


@pytest.fixture(params=[0, None, 2], ids=['h3_off', 'h3_default', 'h3_forced'])
def h3_mode(request):
    prev = ops.set_h3_mode(request.param) if request.param is not None else None
    yield request.param
    if prev is not None:
        ops.set_h3_mode(prev)


@pytest.mark.parametrize('name', list(Cs.CASES))
def test_shape_cases_vs_fp64(name, h3_mode):
    c = Cs.reference(name)
    assert R.relu_margin(c['aux']) >= 1e-5
    B, L = c['B'], c['L']
    m = Cs.module(c['W'], c['H'], c['V'])[0].to(DEV).train()
    td, ld = torch.from_numpy(c['tokens']).to(DEV), torch.from_numpy(c['labels']).to(DEV)
    before = ops.sent_cls_bwd_launches()
    loss, grads = _run(m, td, c['lens'], ld)
    assert ops.sent_cls_bwd_launches() - before == 2 * L + 13 + (L > 1)          # the header's formula, no out_keep
    _hold(loss, grads, c, name)
    if L == 1:
        assert not grads[R.NAMES[2]].any()                     # no recurrent row: weight_hh's gradient is written as zeros
    # device lengths: the same bits, no host read
    lens_d = torch.tensor(c['lens'], dtype=torch.int64, device=DEV)
    loss_d, grads_d = _run(m, td, lens_d, ld)
    assert np.array_equal(loss, loss_d) and all(np.array_equal(grads[n], grads_d[n]) for n in R.NAMES)
    # what stands behind the lengths changes no bit
    junk = c['tokens'].copy()
    behind = np.arange(L)[None, :] >= np.asarray(c['lens'])[:, None]
    junk[behind] = np.random.default_rng(1).integers(1, c['V'], int(behind.sum()))
    loss_j, grads_j = _run(m, torch.from_numpy(junk).to(DEV), lens_d, ld)
    assert np.array_equal(loss, loss_j) and all(np.array_equal(grads[n], grads_j[n]) for n in R.NAMES)


@pytest.mark.parametrize('name', list(Cs.MASKED))
def test_replayed_keep_masks_and_modes(name):
    c = Cs.reference(name)
    assert R.relu_margin(c['aux']) >= 1e-5
    m = Cs.module(c['W'], c['H'], c['V'], dropout_p=0.5)[0].to(DEV).train()
    td, ld = torch.from_numpy(c['tokens']).to(DEV), torch.from_numpy(c['labels']).to(DEV)
    masks = [torch.from_numpy(a) for a in c['masks']]
    before = ops.sent_cls_bwd_launches()
    loss, grads = _run(m, td, c['lens'], ld, masks)
    assert ops.sent_cls_bwd_launches() - before == 2 * c['L'] + 13 + 1 + 1      # + [L > 1] + [out_keep]
    _hold(loss, grads, c, name)
    # train mode with p > 0 draws masks: another loss than without dropout; eval mode draws none
    torch.manual_seed(3)
    drawn = float(sent_cls_loss_with_grad(m, td, c['lens'], ld).detach())
    m.eval()
    plain = sent_cls_loss_with_grad(m, td, c['lens'], ld)
    assert abs(drawn - float(plain.detach())) > 1e-3
    # ... and its logits are the frozen forward's, bit for bit
    lens_i32 = torch.tensor(c['lens'], dtype=torch.int32, device=DEV)
    params = [p.detach() for p in m.native_params()]
    st = ops.sent_cls_train_fwd(params, td, lens_i32, ld)
    logits, weights, pred, _ = ops.sent_cls_fwd(params, td, lens_i32)
    assert torch.equal(st['logits'], logits) and torch.equal(st['weights'], weights) and torch.equal(st['pred'], pred)
    assert float(st['loss'][0]) == float(plain.detach())


def test_second_backward_through_a_retained_graph_gives_the_same_gradients():
    c = Cs.reference('one_row')
    m = Cs.module(c['W'], c['H'], c['V'])[0].to(DEV).train()
    td, ld = torch.from_numpy(c['tokens']).to(DEV), torch.from_numpy(c['labels']).to(DEV)
    loss = sent_cls_loss_with_grad(m, td, c['lens'], ld)
    loss.backward(retain_graph=True)
    first = _grads(m)
    m.zero_grad()
    loss.backward()
    second = _grads(m)
    assert all(np.array_equal(first[n], second[n]) for n in R.NAMES)


def test_shapes_outside_the_kernels_raise():
    m = Cs.module(48, 32, 64)[0].to(DEV)                       # word_emb_dim % 32 != 0
    with pytest.raises(ValueError, match='multiples of 32'):
        sent_cls_loss_with_grad(m, torch.zeros(2, 3, dtype=torch.int64, device=DEV), [3, 2],
                                torch.zeros(2, dtype=torch.int64, device=DEV))


def test_repeatable_and_capturable():
    c = Cs.reference('unequal_widths')
    m = Cs.module(c['W'], c['H'], c['V'])[0].to(DEV).train()
    td, ld = torch.from_numpy(c['tokens']).to(DEV), torch.from_numpy(c['labels']).to(DEV)
    lens_d = torch.tensor(c['lens'], dtype=torch.int32, device=DEV)
    loss1, g1 = _run(m, td, lens_d, ld)
    loss2, g2 = _run(m, td, lens_d, ld)
    assert np.array_equal(loss1, loss2) and all(np.array_equal(g1[n], g2[n]) for n in R.NAMES)
    # the same work captured once and replayed twice: the eager bits, one chain without branches
    for p in m.parameters():
        p.grad.zero_()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.splitk_ws(DEV)                                     # (the stream's workspace exists before the capture opens)
        with ops.graph_capture(graph, stream=side):
            for p in m.parameters():
                p.grad.zero_()
            loss_c = sent_cls_loss_with_grad(m, td, lens_d, ld)
            loss_c.backward()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(loss_c.detach().cpu().numpy(), loss1)
        gc_ = _grads(m)
        assert all(np.array_equal(g1[n], gc_[n]) for n in R.NAMES)
    _assert_one_chain(graph)


def _assert_one_chain(graph):
    """Every node of the kept graph has at most one dependency and one dependent."""
    import ctypes as C
    hip = C.CDLL('libamdhip64.so')
    raw = C.c_void_p(graph.raw_cuda_graph())
    n = C.c_size_t(0)
    assert hip.hipGraphGetEdges(raw, None, None, C.byref(n)) == 0
    src, dst = (C.c_void_p * max(n.value, 1))(), (C.c_void_p * max(n.value, 1))()
    assert hip.hipGraphGetEdges(raw, src, dst, C.byref(n)) == 0
    nodes = ops.graph_kernel_nodes(graph)
    assert nodes > 10
    outs, ins = {}, {}
    for i in range(n.value):
        outs[src[i]] = outs.get(src[i], 0) + 1
        ins[dst[i]] = ins.get(dst[i], 0) + 1
    assert max(outs.values()) == 1 and max(ins.values()) == 1, 'the captured step has parallel branches'


def test_evaluate_counts_and_checkpoint_round_trip(tmp_path):
    c = Cs.reference('unequal_widths')
    srt = np.sort(c['aux']['logits'], axis=1)
    assert (srt[:, -1] - srt[:, -2]).min() >= 1e-2             # the fp64 predictions are decided
    m = Cs.module(c['W'], c['H'], c['V'])[0].to(DEV)
    B, lens = c['B'], c['lens']
    order = sorted(range(B), key=lambda i: -lens[i])           # a loader hands rows over longest first
    tok, lab, ln = c['tokens'][order], c['labels'][order], [lens[i] for i in order]
    pred = c['aux']['pred'][order]
    cuts = {'positive': slice(0, 20), 'negative': slice(20, 30), 'neutral': slice(30, B)}
    loaders = {}
    for k, s in cuts.items():
        half = (s.start + s.stop) // 2                         # two batches per category
        loaders[k] = [(torch.from_numpy(lab[a:b]), (torch.from_numpy(tok[a:b, :ln[a]]), ln[a:b]))
                      for a, b in ((s.start, half), (half, s.stop))]
    r = sent_cls_evaluate(m, loaders)
    assert not m.training
    for k, s in cuts.items():
        wrong = int((pred[s] != lab[s]).sum())
        total = s.stop - s.start
        assert r['by_category'][k] == {'total_num': total, 'wrong_num': wrong, 'acc_rate': 100 - wrong / total * 100}
    wrong = int((pred != lab).sum())
    assert 0 < wrong < B
    assert r['all'] == {'total_num': B, 'wrong_num': wrong, 'acc_rate': 100 - wrong / B * 100}
    # checkpoint: device module -> file -> a fresh module, equal parameters; the reference-format file loads
    opt, _ = m.get_optim_and_crit(4e-4, fused=True)
    sent_cls_train_step(m.train(), opt, torch.from_numpy(tok).to(DEV), ln, torch.from_numpy(lab).to(DEV), 0.1)
    st = dict(word_emb_dim=c['W'], rnn_hid_dim=c['H'], dropout_p=0.0)
    from insenticap_model_amd import synth
    path = checkpoint.save_sent_cls_checkpoint(str(tmp_path), 0, m, opt, st, synth.make_idx2word(c['V']),
                                               synth.SENTIMENT_CATEGORIES, 'tiny', 'part')
    m2, epoch, _ = checkpoint.load_sent_cls_checkpoint(path, dataset_name='tiny')
    assert epoch == 0 and all(torch.equal(a.cpu(), b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    ref = os.path.join(os.path.dirname(GOLDEN), 'ref_sent_cls_checkpoint_tiny.ckpt')
    m3, _, _ = checkpoint.load_sent_cls_checkpoint(ref)
    g = np.load(GOLDEN)
    loss = sent_cls_loss_with_grad(m3.to(DEV), torch.from_numpy(g['tokens']).to(DEV), [int(x) for x in g['lens']],
                                   torch.from_numpy(g['labels']).to(DEV))
    assert abs(float(loss.detach()) - g['loss'][1]) <= 0.05 * g['loss'][1]     # two small Adam steps past the fixture's second loss
