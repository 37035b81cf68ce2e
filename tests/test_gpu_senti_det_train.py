"""The image-sentiment detector's training on the library's kernels - train.senti_det_loss_with_grad /
senti_det_train_step (isc_senti_det_train_fwd, isc_senti_det_bwd), senti_det_evaluate - against the reference's fixture
(tests/golden/senti_det_train.npz) and the fp64 restatement tests/_senti_det_train_ref.py.  pytest -m gpu.

Yardstick, per loss and per gradient: |device - fp64| <= 4 max(e, 2^-23 max|fp64|), e = the stock fp32 module's autograd
error on the CPU against the same fp64 reference (computed here: the bound never comes from the code under test).
Every case's input condition is asserted by tests/test_senti_det_train_ref_host.py and again here."""
import os

import numpy as np
import pytest
import torch

import _senti_det_train_cases as Cs
import _senti_det_train_ref as R
from insenticap_model_amd import _lib, checkpoint, ops
from insenticap_model_amd.optim import FusedClampAdam
from insenticap_model_amd.train import senti_det_evaluate, senti_det_loss_with_grad, senti_det_train_step

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'senti_det_train.npz')
FIXTURE_CASE = dict(Cs.DEFAULTS, C=64, h=5, w=5, B=6)
E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4          # include/insenticap_hip.h


def _grads(m):
    return {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()}


def _run(m, feats, labels, keep=None, scale=1.0):
    m.zero_grad()
    loss = senti_det_loss_with_grad(m, feats, labels, _keep_mask=keep, _scale=scale)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu().numpy().copy(), _grads(m)


def _hold(loss, grads, c, tag=''):
    err, bound = R.yardstick(loss, np.asarray(c['loss']), c['e_loss'])
    print('%s loss: err %.3g  fp32-cpu err %.3g  bound %.3g' % (tag, err, c['e_loss'], bound))
    assert err <= bound, (tag, err, bound)
    for n in c['names']:
        err, bound = R.yardstick(grads[n], c['grads'][n], c['e_grads'][n])
        print('   %s grad %s: err %.3g  fp32-cpu err %.3g  bound %.3g  max|fp64| %.3g' % (
            tag, n, err, c['e_grads'][n], bound, np.abs(c['grads'][n]).max()))
        assert err <= bound, (tag, n, err, bound)


def _assert_launches(before, after, n_convs):
    """The header's formulas, each on its own: 2 n_convs + 3 forward launches and 4 n_convs + 1 backward launches, each
    plus its slab reduces - at most one per conv forward and one per dX backward ('reduce' counts those of both calls)."""
    fwd, bwd, red = (after[k] - before[k] for k in ('fwd', 'bwd', 'reduce'))
    fwd_red, bwd_red = fwd - (2 * n_convs + 3), bwd - (4 * n_convs + 1)
    assert 0 <= fwd_red <= n_convs and 0 <= bwd_red <= n_convs - 1, (fwd, bwd, red)
    assert fwd_red + bwd_red == red, (fwd, bwd, red)


def _device_case(name):
    c = Cs.reference(name)
    m = Cs.module(c['c'], c['p'], weights=c['w'])[0].to(DEV).train()
    fd, ld = torch.from_numpy(np.array(c['feats'])).to(DEV), torch.from_numpy(np.array(c['labels'])).to(DEV)
    keep = torch.from_numpy(c['keep']).to(DEV) if c['keep'] is not None else None
    return c, m, fd, ld, keep


@pytest.mark.parametrize('fused', [False, True], ids=['adam', 'fused'])
def test_training_step_vs_the_reference(fused):
    """Two iterations (dropout_p = 0, lr 4e-4, clip 0.1) against what the reference's module, CrossEntropyLoss,
    clip_gradient and Adam gave.  Iteration 1 starts from the fixture's weights - the fixture's loss and gradients are the
    fp32 CPU module's, which is asserted (1e-6 of the loss, 1e-5 of each gradient's largest element); iteration 2 starts
    from the weights the device's own first step left, so its fp64 reference and its e are computed from exactly those.
    The parameters after step 2 are held to the fixture in the median / fraction form of tests/test_gpu_sent_cls_train.py,
    scaled to this learning rate."""
    g = np.load(GOLDEN)
    lr, clip = float(g['hyper'][0]), float(g['hyper'][1])
    feats, labels = g['feats'], g['labels']
    names = R.names(2, 2)
    m = Cs.module(FIXTURE_CASE, weights={n: g['sd/' + n] for n in names})[0].to(DEV).train()
    opt, _ = m.get_optim_criterion(lr, fused=fused)
    assert isinstance(opt, FusedClampAdam) == fused
    fd, ld = torch.from_numpy(feats).to(DEV), torch.from_numpy(labels).to(DEV)
    for it in range(2):
        now = {n: v.cpu().numpy().copy() for n, v in m.state_dict().items()}
        L64, G64, aux = R.forward_backward(now, feats, labels)
        assert R.relu_margin(aux) >= 1e-5
        cpu = Cs.module(FIXTURE_CASE, weights=now)[0]
        eL, eG, g32, L32 = Cs.cpu_error(cpu, feats, labels, L64, G64)
        if it == 0:                                            # the fixture's numbers are this module's
            assert abs(L32 - g['loss'][0]) <= 1e-6 * g['loss'][0]
            for n in names:
                ref = g['grad1/' + n]
                assert np.abs(g32[n] - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-9, n
        _, grads = _run(m, fd, ld)                             # the gradients as the node gives them, before the clamp
        loss = senti_det_train_step(m, opt, fd, ld, clip)
        assert loss.is_cuda and loss.dim() == 0
        _hold(loss.cpu().numpy(), grads, dict(loss=L64, grads=G64, e_loss=eL, e_grads=eG, names=names),
              'iteration %d' % (it + 1))
        for n, p in m.named_parameters():
            assert np.array_equal(np.clip(grads[n], -clip, clip), p.grad.cpu().numpy()), n
    for n, v in m.state_dict().items():
        d = np.abs(v.cpu().numpy() - g['after2/' + n])
        assert d.max() <= 2 * 2 * lr * 1.01, n
        assert np.median(d) <= lr / 40, (n, float(np.median(d)))
        assert (d > lr / 10).mean() <= 0.1, (n, float((d > lr / 10).mean()))


@pytest.mark.parametrize('name', list(Cs.CASES))
def test_shape_cases_vs_fp64(name):
    """Loss and all ten gradients of every shape case against fp64 under the yardstick; the forward's and the backward's
    launch counts against the header's two formulas; two calls give equal bits; labels as a host list give the bits of the
    device tensor."""
    c, m, fd, ld, _ = _device_case(name)
    assert R.relu_margin(c['aux']) >= 1e-5
    n_convs = c['c']['n_convs']
    before = ops.senti_det_bwd_launches()
    loss, grads = _run(m, fd, ld)
    after = ops.senti_det_bwd_launches()
    _assert_launches(before, after, n_convs)
    _hold(loss, grads, c, name)
    # two calls give equal bits; labels as a host list give the same bits as the device tensor
    loss2, grads2 = _run(m, fd, ld)
    assert np.array_equal(loss, loss2) and all(np.array_equal(grads[n], grads2[n]) for n in c['names'])
    loss3, grads3 = _run(m, fd, c['labels'].tolist())
    assert np.array_equal(loss, loss3) and all(np.array_equal(grads[n], grads3[n]) for n in c['names'])


@pytest.mark.parametrize('name', list(Cs.MASKED))
def test_replayed_keep_masks_and_modes(name):
    c, m, fd, ld, keep = _device_case(name)
    assert R.relu_margin(c['aux']) >= 1e-5
    before = ops.senti_det_bwd_launches()
    loss, grads = _run(m, fd, ld, keep)
    after = ops.senti_det_bwd_launches()
    _assert_launches(before, after, 2)                         # the mask changes neither count
    _hold(loss, grads, c, name)
    # train mode with p > 0 draws masks: another loss than without dropout; eval mode draws none
    torch.manual_seed(3)
    drawn = float(senti_det_loss_with_grad(m, fd, ld).detach())
    m.eval()
    plain = senti_det_loss_with_grad(m, fd, ld)
    assert abs(drawn - float(plain.detach())) > 1e-3


@pytest.mark.parametrize('name', list(Cs.TINY))
def test_tiny_gradients(name):
    """senti_conv and the FC weights times 2^-10, the loss times 2^-6: every |dx2| and |dx1| element is below 2^-24 in
    fp64 - the same yardstick, relative to each gradient's own magnitude."""
    c, m, fd, ld, _ = _device_case(name)
    assert all(np.abs(d).max() < 2.0 ** -24 for d in c['aux']['dx'])
    loss, grads = _run(m, fd, ld, scale=c['scale'])
    _hold(loss, grads, c, name)
    assert all(np.abs(grads[n]).max() > 0 for n in c['names'])


@pytest.mark.parametrize('name', ['rows_75', 'c128_14x14', 'product'])
def test_training_forward_equals_the_frozen_forward_in_bits(name):
    c, m, fd, ld, _ = _device_case(name)
    params = [p.detach() for p in m.native_params()]
    st = ops.senti_det_train_fwd(params, fd, ld)
    logits, maps, _, _ = m.forward_native(fd)
    assert torch.equal(st['logits'], logits) and torch.equal(st['maps'], maps)
    err, bound = R.yardstick(st['logits'].cpu().numpy(), c['aux']['logits'], 0.0)
    assert err <= 64 * bound                                  # (and they are the detector's logits at all)


def test_an_images_dx_rows_depend_on_that_image_alone():
    """The gradient of conv_0's output (a test-only output), image 1's rows: not one bit changes when the features of
    images 0 and 2 change - although those images' gradients, and with them the common scale, do."""
    c, m, fd, ld, _ = _device_case('rows_75')
    params = [p.detach() for p in m.native_params()]
    hw = c['c']['h'] * c['c']['w']
    dx = ops.senti_det_bwd(ops.senti_det_train_fwd(params, fd, ld), want_dx=True)[-1]
    err, bound = R.yardstick(dx.cpu().numpy(), c['aux']['dx'][0].reshape(dx.shape), 0.0)
    assert err <= 16 * bound, (err, bound)                    # (it is dx1 - the split-f16 engine's few 2^-23)
    other = fd.clone()
    other[0] = other[0].flip(0) * 3.0
    other[2] = other[2].roll(1, 1) * 0.25
    dx2 = ops.senti_det_bwd(ops.senti_det_train_fwd(params, other, ld), want_dx=True)[-1]
    assert torch.equal(dx[hw:2 * hw], dx2[hw:2 * hw])
    assert not torch.equal(dx[:hw], dx2[:hw]) and not torch.equal(dx[2 * hw:], dx2[2 * hw:])


def test_a_row_gather_batch_of_a_device_resident_store_trains():
    """The documented loop: a DeviceFeatureStore behind get_senti_image_dataloader hands senti_det_train_step a
    data.RowGather; the step expands it and gives the bits of the step on the dense batch."""
    from insenticap_model_amd import data
    c, m, fd, ld, _ = _device_case('rows_75')
    fns = ['i%d' % i for i in range(c['c']['B'])]
    store = data.DeviceFeatureStore.from_arrays(fns, c['feats'], DEV)
    loader = data.get_senti_image_dataloader(store, [[fn, int(l)] for fn, l in zip(fns, c['labels'])], batch_size=8,
                                             shuffle=False)
    (_, att, labels), = list(loader)
    assert isinstance(att, data.RowGather) and labels.dtype == torch.int64
    m2 = Cs.module(c['c'], c['p'], weights=c['w'])[0].to(DEV).train()
    opt, opt2 = m.get_optim_criterion(4e-4, fused=True)[0], m2.get_optim_criterion(4e-4, fused=True)[0]
    loss = senti_det_train_step(m, opt, att, labels, 0.1)
    loss2 = senti_det_train_step(m2, opt2, fd, ld, 0.1)
    assert torch.equal(loss, loss2)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    err, bound = R.yardstick(loss.cpu().numpy(), np.asarray(c['loss']), c['e_loss'])
    assert err <= bound


def test_a_label_outside_the_categories_poisons_loss_and_gradients():
    c, m, fd, ld, _ = _device_case('rows_75')
    bad = ld.clone()
    bad[1] = c['c']['k']
    loss, grads = _run(m, fd, bad)
    assert np.isnan(loss) and all(np.isnan(grads[n]).any() for n in c['names'])
    bad[1] = -1
    assert np.isnan(_run(m, fd, bad)[0])


def test_an_in_place_parameter_update_between_forward_and_backward_raises():
    c, m, fd, ld, _ = _device_case('grid_1x5')
    loss = senti_det_loss_with_grad(m, fd, ld)
    with torch.no_grad():
        m.senti_conv.weight.mul_(2.0)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        loss.backward()


def test_float16_features_are_converted_once():
    c, m, fd, ld, _ = _device_case('rows_75')
    half = fd.to(torch.float16)
    loss_h, grads_h = _run(m, half, ld)
    loss_f, grads_f = _run(m, half.float(), ld)
    assert np.array_equal(loss_h, loss_f) and all(np.array_equal(grads_h[n], grads_f[n]) for n in c['names'])


def test_capturable():
    c, m, fd, ld, _ = _device_case('rows_1332')
    loss1, g1 = _run(m, fd, ld)
    for p in m.parameters():
        p.grad.zero_()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with ops.graph_capture(graph, stream=side):
            for p in m.parameters():
                p.grad.zero_()
            loss_c = senti_det_loss_with_grad(m, fd, ld)
            loss_c.backward()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(loss_c.detach().cpu().numpy(), loss1)
        gc_ = _grads(m)
        assert all(np.array_equal(g1[n], gc_[n]) for n in c['names'])


def test_evaluate_counts_and_checkpoint_round_trip(tmp_path):
    g = np.load(GOLDEN)
    names = R.names(2, 2)
    w = {n: g['sd/' + n] for n in names}
    feats, labels = g['feats'], g['labels']
    aux = R.forward_backward(w, feats, labels)[2]
    srt = np.sort(aux['prob'], axis=1)
    assert (srt[:, -1] - srt[:, -2]).min() >= 1e-3             # the fp64 predictions are decided
    pred = aux['prob'].argmax(axis=1)
    m = Cs.module(FIXTURE_CASE, weights=w)[0].to(DEV)
    loader = [(('a', 'b', 'c'), torch.from_numpy(feats[:3]), torch.from_numpy(labels[:3])),
              (('d', 'e', 'f'), torch.from_numpy(feats[3:]).to(torch.float16), torch.from_numpy(labels[3:]))]
    want = int((pred == labels).sum())
    for native in (False, True):
        r = senti_det_evaluate(m.enable_native(native), loader)
        assert not m.training
        assert r == {'corr_num': want, 'all_num': 6, 'corr_rate': want / 6}
    m.enable_native(False)
    with torch.no_grad():                                      # the torch path's count, as train_senti.py:100-108 forms it
        idx = m.sample(torch.from_numpy(feats).to(DEV))[0]
    assert int((idx.cpu() == torch.from_numpy(labels)).sum()) == want
    # checkpoint: device module -> file -> a fresh module, equal parameters; the reference-format file loads
    opt, _ = m.get_optim_criterion(4e-4, fused=True)
    senti_det_train_step(m.train(), opt, torch.from_numpy(feats).to(DEV), torch.from_numpy(labels).to(DEV), 0.1)
    st = {'fc_feat_dim': 64, 'sentiment_convs_num': 2, 'sentiment_fcs_num': 2, 'dropout_p': 0.0}
    path = checkpoint.save_senti_checkpoint(str(tmp_path), 0, m, opt, st, m.sentiment_categories)
    m2, epoch, _ = checkpoint.load_senti_checkpoint(path, settings=st)
    assert epoch == 0 and all(torch.equal(a.cpu(), b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    with pytest.raises(AssertionError, match='settings'):
        checkpoint.load_senti_checkpoint(path, settings=dict(st, dropout_p=0.5))
    ref = os.path.join(os.path.dirname(GOLDEN), 'ref_senti_checkpoint_tiny.ckpt')
    m3, epoch3, _ = checkpoint.load_senti_checkpoint(ref)
    assert epoch3 == 1
    for n, v in m3.state_dict().items():
        assert np.array_equal(v.numpy(), g['after2/' + n]), n


def _problem(c, m, fd, ld):
    st = ops.senti_det_train_fwd([p.detach() for p in m.native_params()], fd, ld)
    return st, st['problem']


def test_refusals_return_their_code_and_write_nothing():
    c, m, fd, ld, _ = _device_case('grid_1x5')
    lib = _lib.load()
    import ctypes as C
    st, p = _problem(c, m, fd, ld)
    torch.cuda.synchronize()
    st['loss'].fill_(-7.0)
    st['logits'].fill_(-7.0)
    grads = ops.senti_det_bwd(st)                               # (fills the gradient pointers and the workspace)
    for t in grads:
        t.fill_(-7.0)
    torch.cuda.synchronize()
    stream = ops.stream()

    def both(expect, what):
        assert lib.isc_senti_det_train_fwd(C.byref(p), stream) == expect, what
        assert lib.isc_senti_det_bwd(C.byref(p), stream) == expect, what

    old = p.C
    p.C = 48
    both(E_SHAPE, 'C % 32')
    p.C = old
    old = p.k
    p.k = 9
    both(E_SHAPE, 'k > 8')
    p.k = old
    old = p.n_convs
    p.n_convs = 5
    both(E_SHAPE, 'n_convs > 4')
    p.n_convs = old
    old = p.labels
    p.labels = None
    both(E_NULL, 'labels')
    p.labels = old
    old = p.conv_w[1]
    p.conv_w[1] = None
    both(E_NULL, 'conv_w[1]')
    p.conv_w[1] = old
    old = p.feats
    p.feats = old + 4
    both(E_ALIGN, 'feats + 4')
    p.feats = old
    old = p.saved_bytes
    p.saved_bytes = old - 1
    both(E_WORKSPACE, 'short saved')
    p.saved_bytes = old
    old = p.workspace_bytes
    p.workspace_bytes = old - 1
    assert lib.isc_senti_det_bwd(C.byref(p), stream) == E_WORKSPACE
    p.workspace_bytes = old
    old = p.d_senti_w
    p.d_senti_w = None
    assert lib.isc_senti_det_bwd(C.byref(p), stream) == E_NULL
    p.d_senti_w = old
    torch.cuda.synchronize()
    assert float(st['loss'][0]) == -7.0 and bool((st['logits'] == -7.0).all())
    assert all(bool((t == -7.0).all()) for t in grads)
    # the Python entry point says what it does not take - no quiet torch fallback
    bad = Cs.module(dict(Cs.DEFAULTS, C=48, h=2, w=2, B=2, n_convs=1))[0].to(DEV)
    with pytest.raises(ValueError, match='multiple of 32'):
        senti_det_loss_with_grad(bad, torch.zeros(2, 2, 2, 48, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV))
