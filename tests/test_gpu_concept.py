"""The concept detector's paths on the device: isc_concept_fwd / ConceptDetector.sample / sample_device at tiny, unequal
and product widths, the training step against the fixture the reference wrote, the HIP-graph capture of sample_device,
and the Detector's device tagging.

Yardstick (tests/test_gpu_sent_cls.py): |native - fp64| <= 4 max(e, 2^-23 max|fp64|), e = the error of the stock fp32
torch module on the CPU against the same fp64 reference (tests/_concept_ref.py), computed here.

Top-k indices must equal the fp64 reference's on EVERY row of every case.  That is only meaningful where fp64 itself
separates the candidates, so each case first asserts, on the CPU, that the smallest fp64 gap among the top num + 1 logits
of any row is >= 1e-2 (the margin tests/test_gpu_sent_cls.py uses) and that the fp32 CPU module already agrees with fp64
on every row.  With 2000 concepts about one random image in three has two of its six best logits closer than that
(their spacing is ~0.1-0.3 at a logit spread of 1.4), so no seed gives 100 such rows in a row: the rows of a case are
drawn in order from np.random.default_rng(SEED) and a drawn row whose fp64 gap is under 1e-2 is skipped for the next
draw - the rule is applied to the inputs, before anything runs on the device, and every row of the case is compared.
Weights: synth.make_module_weights(shapes, 61, gain) - gain 4 at the small widths, 3 at the product widths (the largest
logit stays near 6: the fp32 sigmoid does not saturate, so the CPU module's own sort is well defined)."""
import os

import numpy as np
import pytest
import torch

import _concept_ref as R
from conftest import GOLDEN_DIR
from insenticap_model_amd import FusedClampAdam, data, ops, synth
from insenticap_model_amd.helper_nets import ConceptDetector
from insenticap_model_amd.train import concept_loss_with_grad, concept_train_step

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SEED, WSEED = 8, 61

# name -> (fc, mid, concepts, rows, num, gain)
CASES = {
    'tiny': (64, 32, 20, 6, 5, 4.0),
    'unequal': (96, 64, 68, 37, 5, 4.0),
    'product_b1': (2048, 1024, 2000, 1, 5, 3.0),
    'product_b80': (2048, 1024, 2000, 80, 5, 3.0),
    'product_b100': (2048, 1024, 2000, 100, 5, 3.0),
}
# launches of the three linear layers per case as the existing counters see them: (few-row kernels, large split-f16,
# skinny split-f16, exact-fp32 tiles + split-K reduces) under the default engine; under isc_set_h3_mode(0) no split-f16
# kernel may run at all
ROUTES = {'tiny': (3, 0, 0, 0), 'unequal': (0, 0, 0, 3), 'product_b1': (3, 0, 0, 0), 'product_b80': (0, 0, 0, 6),
          'product_b100': (0, 0, 0, 6)}       # (<= 8 rows: the few-row kernels; 80 / 100 rows: fp32 split-K + its reduce)
_REF = {}


def module(F, H, C, gain):
    m = ConceptDetector(['c%d' % i for i in range(C)], dict(fc_feat_dim=F, concept_mid_him=H, dropout_p=0.5))
    w = synth.make_module_weights({n: tuple(v.shape) for n, v in m.state_dict().items()}, WSEED, gain=gain)
    m.load_state_dict({n: torch.from_numpy(v) for n, v in w.items()})
    return m.eval(), w


def reference(name):
    """Module, inputs (drawn by the rule above), fp64 reference, the fp32 CPU module's outputs and errors - once per case,
    shared, read-only."""
    if name in _REF:
        return _REF[name]
    F, H, C, B, num, gain = CASES[name]
    m, w = module(F, H, C, gain)
    rng = np.random.default_rng(SEED)
    rows, drawn = [], 0
    while len(rows) < B:
        assert drawn <= 4 * B + 16, 'case %s: too many rows under the margin' % name
        block = rng.random((B + 8, F)).astype(np.float32)
        z = R.forward(w, block)['logits']
        for i in range(block.shape[0]):
            if len(rows) < B:
                drawn += 1
                if R.topk_gap(z[i:i + 1], num) >= 1e-2:
                    rows.append(block[i])
    feats = np.stack(rows)
    r = R.forward(w, feats)
    r['idx'] = R.topk(r['logits'], num)
    r['scores'] = np.take_along_axis(r['probs'], r['idx'], axis=1)
    with torch.no_grad():
        cpu_out, cpu_names, cpu_scores = m.sample(torch.from_numpy(feats), num)
        cpu_logits = m.output[:6](torch.from_numpy(feats))
    cpu_idx = np.asarray([[int(n[1:]) for n in row] for row in cpu_names])
    e = dict(probs=np.abs(cpu_out.double().numpy() - r['probs']).max(),
             scores=np.abs(cpu_scores.double().numpy() - r['scores']).max(),
             logits=np.abs(cpu_logits.double().numpy() - r['logits']).max())
    for v in r.values():
        v.setflags(write=False)
    _REF[name] = dict(m=m, w=w, feats=feats, ref=r, e=e, cpu_idx=cpu_idx, num=num, drawn=drawn)
    return _REF[name]


def _counters():
    lib = ops._lib.load()
    return np.asarray([lib.isc_gemv_launches(), lib.isc_h3_launches(), lib.isc_h3s_launches(),
                       sum(lib.isc_f32_launches(k) for k in range(7))])


@pytest.fixture(params=[0, None], ids=['h3_off', 'h3_default'])
def h3_mode(request):
    prev = ops.set_h3_mode(0) if request.param == 0 else None
    yield request.param
    if prev is not None:
        ops.set_h3_mode(prev)


@pytest.mark.parametrize('name', list(CASES))
def test_forward_vs_fp64(name, h3_mode):
    c = reference(name)
    r, num = c['ref'], c['num']
    gap = R.topk_gap(r['logits'], num)
    assert gap >= 1e-2, 'case %s: fp64 gap %.3g among the top %d logits' % (name, gap, num + 1)
    assert np.array_equal(c['cpu_idx'], r['idx'])            # the fp32 CPU module agrees with fp64 on every row
    m = c['m'].to(DEV)
    feats = torch.from_numpy(c['feats']).to(DEV)
    params = [p.detach() for p in m.native_params()]
    table = torch.arange(len(m.idx2concept), dtype=torch.int64, device=DEV) * 2 + 5
    ops.concept_fwd(params, feats, num)                      # (warm: the stream's workspaces)
    n0, k0 = ops.concept_launches(), _counters()
    out = ops.concept_fwd(params, feats, num, concept_word=table, want_logits=True)
    torch.cuda.synchronize()
    assert ops.concept_launches() - n0 == 4
    route = tuple(int(x) for x in _counters() - k0)
    print('%s[%s] rows drawn %d, fp64 gap %.3g, route (gemv, h3, h3s, f32) %r' % (
        name, 'h3=0' if h3_mode == 0 else 'h3 default', c['drawn'], gap, route))
    if h3_mode == 0:
        assert route[1] == route[2] == 0 and route[0] + route[3] >= 3, route
    elif name in ROUTES:
        assert route == ROUTES[name], (name, route)
    assert np.array_equal(out['idx'].cpu().numpy(), r['idx'])               # every row
    assert np.array_equal(out['words'].cpu().numpy(), r['idx'] * 2 + 5)
    for k in ('logits', 'probs', 'scores'):
        err, bound = R.yardstick(out[k].cpu().numpy(), r[k], c['e'][k])
        print('   %s: native err %.3g  torch-fp32-cpu err %.3g  bound %.3g' % (k, err, c['e'][k], bound))
        assert err <= bound, (name, k, err, bound)
    again = ops.concept_fwd(params, feats, num, concept_word=table, want_logits=True)
    for k in out:
        assert torch.equal(out[k], again[k]), k


@pytest.mark.parametrize('name', ['tiny', 'unequal', 'product_b100'])
def test_module_paths_native_torch_and_float16(name):
    c = reference(name)
    r, num = c['ref'], c['num']
    m = c['m'].to(DEV)
    m.set_vocabulary({n: 7 + 3 * i for i, n in enumerate(m.idx2concept)})
    feats = torch.from_numpy(c['feats']).to(DEV)
    with torch.no_grad():
        assert m.native and m.native_active(feats) and not m.native_active(feats.cpu())
    assert not m.native_active(feats)                        # a gradient could be asked for: the torch ops
    n0 = ops.concept_launches()
    out, names, scores = m.sample(feats, num)
    idx, sc2, words = m.sample_device(feats, num)
    with torch.no_grad():
        probs = m(feats)
    assert ops.concept_launches() - n0 == 12
    assert names == [['c%d' % i for i in row] for row in r['idx'].tolist()]
    assert np.array_equal(idx.cpu().numpy(), r['idx']) and np.array_equal(words.cpu().numpy(), 7 + 3 * r['idx'])
    assert torch.equal(sc2, scores) and torch.equal(probs, out)
    # the stock torch ops on the device agree with native under the yardstick, and pick the same concepts
    m.enable_native(False)
    try:
        with torch.no_grad():
            assert not m.native_active(feats)
        n0 = ops.concept_launches()
        t_out, t_names, t_scores = m.sample(feats, num)
        t_idx, _, t_words = m.sample_device(feats, num)
        assert ops.concept_launches() == n0
    finally:
        m.enable_native(True)
    assert t_names == names and torch.equal(t_idx, idx) and torch.equal(t_words, words)
    for k, a, b in (('probs', out, t_out), ('scores', scores, t_scores)):
        for which, x in (('native', a), ('torch', b)):
            err, bound = R.yardstick(x.cpu().numpy(), r[k], c['e'][k])
            print('%s %s %s: err %.3g bound %.3g' % (name, k, which, err, bound))
            assert err <= bound, (name, k, which, err, bound)
    # float16 features: the bits of the call on the up-cast values, natively read or converted once
    h = feats.to(torch.float16)
    c0, f0 = ops.f16_convert_launches(), ops.h3_f16a_launches()
    a = ops.concept_fwd([p.detach() for p in m.native_params()], h, num, want_logits=True)
    converted, native16 = ops.f16_convert_launches() - c0, ops.h3_f16a_launches() - f0
    b = ops.concept_fwd([p.detach() for p in m.native_params()], h.float(), num, want_logits=True)
    assert converted + native16 == 1, (converted, native16)
    print('%s float16 features: %s' % (name, 'read natively' if native16 else 'converted once'))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    with torch.no_grad():
        assert m.native_active(h)
    assert torch.equal(m.sample_device(h, num)[0], a['idx'])
    m.train()                                                # train mode runs the torch ops
    with torch.no_grad():
        assert not m.native_active(feats)
    m.eval()


def test_shapes_the_linear_dispatch_cannot_take_run_the_torch_path():
    m, _ = module(48, 32, 12, 3.0)                            # fc_feat_dim % 32 != 0
    m.to(DEV)
    x = torch.rand(3, 48, device=DEV)
    with torch.no_grad():
        assert not m.native_active(x)
    n0 = ops.concept_launches()
    out, names, scores = m.sample(x, 4)
    assert ops.concept_launches() == n0 and out.shape == (3, 12) and len(names[0]) == 4
    with pytest.raises(ValueError):
        concept_loss_with_grad(m, x, torch.zeros(3, 12, dtype=torch.int64, device=DEV))
    m2, _ = module(64, 32, 12, 3.0)
    m2.to(DEV)
    for bad in (0, 13, 17):
        with pytest.raises(ValueError):
            m2.sample(torch.rand(2, 64, device=DEV), bad)


def test_sample_device_in_a_hip_graph():
    c = reference('unequal')
    m, num = c['m'].to(DEV), c['num']
    m.set_vocabulary({n: 7 + 3 * i for i, n in enumerate(m.idx2concept)})
    rng = np.random.default_rng(77)
    fresh = [torch.from_numpy(rng.random(c['feats'].shape).astype(np.float32)).to(DEV) for _ in range(3)]
    eager = [tuple(t.clone() for t in m.sample_device(x, num)) for x in fresh]
    static = torch.from_numpy(c['feats']).to(DEV).clone()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        m.sample_device(static, num)                         # warm (allocates the stream's workspace outside the capture)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            got = m.sample_device(static, num)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    for x, want in zip(fresh, eager):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)


# ------------------------------------------------------------------ training step
def _fixture_model(g):
    m = ConceptDetector(['cpt%d' % i for i in range(20)], {'fc_feat_dim': 64, 'concept_mid_him': 32, 'dropout_p': 0.0})
    m.load_state_dict({k: torch.from_numpy(g['sd/' + k]) for k in R.NAMES})
    return m


def test_training_step_vs_the_reference(golden):
    """Two iterations with dropout_p = 0 against what the reference's module, criterion, clip_gradient and Adam gave
    (tests/golden/concept.npz).  Loss and gradients of BOTH iterations are held to the yardstick against fp64, with e
    from the fp32 CPU module: iteration 1 starts from the fixture's weights - the fixture's loss and gradients are that
    module's, which is asserted; iteration 2 starts from the weights the device's own first step left (a first Adam step
    moves every element by +-lr whatever its gradient's size, so the two sides' weights differ where a gradient is
    rounding noise), so its fp64 reference and its e are computed from exactly those weights.  The parameters after
    the second step are held to the fixture in the median / fraction form of tests/test_gpu_bench_config.py:283-291,
    scaled to this learning rate (there, at lr 4e-5: max 4 lr, median lr / 40, at most a tenth beyond lr / 10)."""
    from insenticap_model_amd.helper_nets import MultiLabelClsLoss
    g = golden('concept')
    lr, clip = float(g['hyper'][0]), float(g['hyper'][1])
    feats, targets = g['feats'], g['targets']
    m = _fixture_model(g).to(DEV).train()
    opt, _ = m.get_optim_criterion(lr)
    assert isinstance(opt, FusedClampAdam)
    fd, td = torch.from_numpy(feats).to(DEV), torch.from_numpy(targets).to(DEV)
    for it in range(2):
        now = {k: v.cpu().numpy().copy() for k, v in m.state_dict().items()}
        L64, g64 = R.backward(now, feats, targets)
        cpu = _fixture_model(g).train()
        cpu.load_state_dict({k: torch.from_numpy(v) for k, v in now.items()})
        L32 = MultiLabelClsLoss()(cpu(torch.from_numpy(feats)), torch.from_numpy(targets))
        L32.backward()
        if it == 0:                                          # the fixture's numbers are this module's
            assert abs(float(L32.detach()) - g['loss'][0]) <= 1e-6 * g['loss'][0]
            for k, q in cpu.named_parameters():
                ref = g['grad1/' + k]
                assert np.abs(q.grad.numpy() - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-9, k
        # the gradients as the step's own autograd node gives them, read before the step clamps them in place ...
        m.zero_grad()
        concept_loss_with_grad(m, fd, td).backward()
        grads = {k: p.grad.cpu().numpy().copy() for k, p in m.named_parameters()}
        loss = concept_train_step(m, opt, fd, td, clip)      # ... and the step itself (loss, backward, clamp + Adam)
        assert loss.is_cuda and loss.dim() == 0
        e = abs(float(L32.detach()) - L64)
        err, bound = R.yardstick(loss.cpu().numpy(), np.asarray(L64), e)
        print('iteration %d loss: err %.3g  fp32-cpu err %.3g  bound %.3g' % (it + 1, err, e, bound))
        assert err <= bound, (it, err, bound)
        for (k, p), (_, q) in zip(m.named_parameters(), cpu.named_parameters()):
            e = np.abs(q.grad.double().numpy() - g64[k]).max()
            err, bound = R.yardstick(grads[k], g64[k], e)
            print('   grad %s: err %.3g  fp32-cpu err %.3g  bound %.3g' % (k, err, e, bound))
            assert err <= bound, (it, k, err, bound)
            assert np.array_equal(np.clip(grads[k], -clip, clip), p.grad.cpu().numpy()), k      # the step's own, clamped
    for k, v in m.state_dict().items():
        d = np.abs(v.cpu().numpy() - g['after2/' + k])
        assert d.max() <= 2 * 2 * lr * 1.01, k
        assert np.median(d) <= lr / 40, (k, float(np.median(d)))
        assert (d > lr / 10).mean() <= 0.1, (k, float((d > lr / 10).mean()))


def test_training_step_with_a_keep_mask_vs_fp64(golden):
    g = golden('concept')
    feats, targets = g['feats'], g['targets']
    sd = {k: g['sd/' + k] for k in R.NAMES}
    keep = (np.random.default_rng(4).random((feats.shape[0], 32)) < 0.5).astype(np.uint8)
    keep[0, :] = 1
    L64, g64 = R.backward(sd, feats, targets, keep_mask=keep, dropout_p=0.5)
    cpu = _fixture_model(g)
    cpu.output[4].p = 0.5
    x = torch.from_numpy(feats)
    h2 = cpu.output[:4](x) * torch.from_numpy(keep).float() * 2.0          # the fp32 CPU module with the same mask
    from insenticap_model_amd.helper_nets import MultiLabelClsLoss
    L32 = MultiLabelClsLoss()(cpu.output[5:](h2), torch.from_numpy(targets))
    L32.backward()
    m = _fixture_model(g).to(DEV).train()
    m.output[4].p = 0.5
    for targets_dev in (torch.from_numpy(targets).to(DEV), torch.from_numpy(targets.astype(np.uint8)).to(DEV)):
        m.zero_grad()
        loss = concept_loss_with_grad(m, torch.from_numpy(feats).to(DEV), targets_dev, _keep_mask=torch.from_numpy(keep))
        loss.backward()
        err, bound = R.yardstick(loss.detach().cpu().numpy(), np.asarray(L64), abs(float(L32.detach()) - L64))
        assert err <= bound, (err, bound)
        for (k, p), (_, q) in zip(m.named_parameters(), cpu.named_parameters()):
            e = np.abs(q.grad.double().numpy() - g64[k]).max()
            err, bound = R.yardstick(p.grad.cpu().numpy(), g64[k], e)
            print('keep-mask grad %s: err %.3g  fp32-cpu err %.3g  bound %.3g' % (k, err, e, bound))
            assert err <= bound, (k, err, bound)
    # a drawn mask: train mode with p > 0 draws one (the loss differs from the p = 0 loss), eval mode draws none
    torch.manual_seed(1)
    a = concept_loss_with_grad(m, torch.from_numpy(feats).to(DEV), torch.from_numpy(targets).to(DEV))
    m.eval()
    b = concept_loss_with_grad(m, torch.from_numpy(feats).to(DEV), torch.from_numpy(targets).to(DEV))
    assert abs(float(b.detach()) - g['loss'][0]) <= 1e-5 and abs(float(a.detach()) - float(b.detach())) > 1e-4


@pytest.mark.parametrize('B,on_h3', [(64, 2), (128, 3)])
def test_training_gradients_on_the_split_f16_dw_route_vs_fp64(B, on_h3):
    """A batch that is a multiple of 32: at the product widths the dW contractions of 2.5e8 FLOP and more go to the
    split-f16 engine - at 64 rows those of the first and the last layer (2.7e8, 2.6e8; the middle one has 1.3e8), at 128
    rows all three (asserted with isc_h3_launches).  dz is ~1 / (B C) = 2^-17 and below; the step
    carries it through the sweep times a power of two, so the gradients stay inside the yardstick against fp64, with e
    from the fp32 CPU module on the same weights and inputs."""
    from insenticap_model_amd.helper_nets import MultiLabelClsLoss
    F, H, C = 2048, 1024, 2000
    m, w = module(F, H, C, 3.0)
    rng = np.random.default_rng(90 + B)
    feats = rng.random((B, F)).astype(np.float32)
    targets = (rng.random((B, C)) < 0.01).astype(np.int64)
    L64, g64 = R.backward(w, feats, targets)
    cpu, _ = module(F, H, C, 3.0)
    L32 = MultiLabelClsLoss()(cpu(torch.from_numpy(feats)), torch.from_numpy(targets))      # (eval mode: no dropout)
    L32.backward()
    m.to(DEV)
    lib = ops._lib.load()
    h0 = lib.isc_h3_launches()
    loss = concept_loss_with_grad(m, torch.from_numpy(feats).to(DEV), torch.from_numpy(targets).to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    took = lib.isc_h3_launches() - h0
    print('B = %d: split-f16 launches %d' % (B, took))
    assert took == on_h3, took
    err, bound = R.yardstick(loss.detach().cpu().numpy(), np.asarray(L64), abs(float(L32.detach()) - L64))
    assert err <= bound, (err, bound)
    worst = []
    for (k, p), (_, q) in zip(m.named_parameters(), cpu.named_parameters()):
        e = np.abs(q.grad.double().numpy() - g64[k]).max()
        err, bound = R.yardstick(p.grad.cpu().numpy(), g64[k], e)
        print('   B = %d grad %s: err %.3g  fp32-cpu err %.3g  bound %.3g  max|fp64| %.3g' % (
            B, k, err, e, bound, np.abs(g64[k]).max()))
        worst.append((k, err, bound))
    for k, err, bound in worst:
        assert err <= bound, (B, k, err, bound)


def test_large_batch_takes_the_split_f16_kernels_and_reads_float16_rows_natively():
    """4096 rows at the product widths: under the default engine the linear launches go to the large split-f16 kernels
    (isc_h3_launches), float16 features are handed to the first one as they are (isc_h3_f16a_launches, no conversion)
    and give the bits of the call on the up-cast values; the first 256 rows are held to fp64 under the yardstick (rows
    are independent; e from the fp32 CPU module on those rows)."""
    F, H, C, B, num = 2048, 1024, 2000, 4096, 5
    m, w = module(F, H, C, 3.0)
    feats = np.random.default_rng(12).random((B, F)).astype(np.float32)
    r = R.forward(w, feats[:256])
    with torch.no_grad():
        cpu_probs = m(torch.from_numpy(feats[:256]))
        cpu_logits = m.output[:6](torch.from_numpy(feats[:256]))
    m.to(DEV)
    params = [p.detach() for p in m.native_params()]
    x = torch.from_numpy(feats).to(DEV)
    lib = ops._lib.load()
    ops.concept_fwd(params, x, num)
    h0 = lib.isc_h3_launches()
    out = ops.concept_fwd(params, x, num, want_logits=True)
    torch.cuda.synchronize()
    took = lib.isc_h3_launches() - h0
    print('B = 4096: split-f16 launches %d' % took)
    assert took >= 3, took
    for k, cpu_v in (('logits', cpu_logits), ('probs', cpu_probs)):
        e = np.abs(cpu_v.double().numpy() - r[k]).max()
        err, bound = R.yardstick(out[k][:256].cpu().numpy(), r[k], e)
        print('   %s: native err %.3g  torch-fp32-cpu err %.3g  bound %.3g' % (k, err, e, bound))
        assert err <= bound, (k, err, bound)
    # (undrawn random rows: the indices are compared on the rows whose own fp64 gap is >= 1e-2 - most of them)
    clear = np.asarray([R.topk_gap(r['logits'][i:i + 1], num) >= 1e-2 for i in range(256)])
    assert clear.sum() >= 128
    assert np.array_equal(out['idx'][:256].cpu().numpy()[clear], R.topk(r['logits'], num)[clear])
    h = x.to(torch.float16)
    c0, f0 = ops.f16_convert_launches(), ops.h3_f16a_launches()
    a = ops.concept_fwd(params, h, num, want_logits=True)
    assert ops.f16_convert_launches() - c0 == 0 and ops.h3_f16a_launches() - f0 == 1
    b = ops.concept_fwd(params, h.float(), num, want_logits=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_reference_checkpoint_on_the_device(golden):
    from insenticap_model_amd import checkpoint
    g = golden('concept')
    m, _, _ = checkpoint.load_concept_checkpoint(os.path.join(GOLDEN_DIR, 'ref_concept_checkpoint_tiny.ckpt'))
    m.to(DEV)
    store = {str(fn): g['feats'][i] for i, fn in enumerate(g['collate_fns'])}
    tags = data.tag_concepts(m, store, 5, batch=4)
    assert list(tags) == list(store) and all(len(v) == 5 for v in tags.values())
    m.enable_native(False)                                   # the stock torch ops on the same weights name the same concepts
    assert data.tag_concepts(m, store, 5, batch=4) == tags


# ------------------------------------------------------------------ Detector
V, TN, B = 64, 8, 4
ST = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)


def _detector():
    from insenticap_model_amd.detector import Detector
    idx2word = synth.make_idx2word(V)
    d = Detector(idx2word, TN, synth.SENTIMENT_CATEGORIES, {'cap_lr': 4e-5}, ST)
    d.captioner.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, ST, seed=1).items()})
    for mod, seed in ((d.senti_detector, 51), (d.sent_senti_cls, 52)):
        shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
        mod.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_module_weights(shapes, seed).items()})
        mod.eval()
    d.to(DEV)
    word2idx = {w: i for i, w in enumerate(idx2word)}
    idx2concept = ['w%d' % (10 + i) for i in range(20)]
    cd = ConceptDetector(idx2concept, dict(fc_feat_dim=ST['fc_feat_dim'], concept_mid_him=32, dropout_p=0.5))
    w = synth.make_module_weights({n: tuple(v.shape) for n, v in cd.state_dict().items()}, WSEED, gain=4.0)
    cd.load_state_dict({n: torch.from_numpy(v) for n, v in w.items()})
    cd.set_vocabulary(word2idx).to(DEV)
    rng = np.random.default_rng(21)
    sd = {c: [['w%d' % int(rng.integers(30, 64)), float(rng.random())] for _ in range(int(rng.integers(0, 7)))]
          for c in idx2concept[:16]}
    table = data.SentimentWordTable(sd, word2idx, idx2concept)
    return d, cd, table, word2idx


def test_detector_tags_on_the_device():
    det, cd, table, word2idx = _detector()
    batches, split = synth.make_rl_batches(2, B, V, ST, seq_len=TN)
    det.set_ciderd_scorer(split)
    with pytest.raises(ValueError):
        det.tag(torch.from_numpy(batches[0][1]).to(DEV))
    det.set_concept_detector(cd, table, num_concepts=5, num_sentiments=10)
    assert not any('concept' in k for k in det.state_dict())
    t = torch.from_numpy
    host = []
    for b in batches:                                        # the host pipeline: names, then ids, then the table's lookup
        fc = t(b[1]).to(DEV)
        _, names, _ = cd.sample(fc, 5)
        cpts = torch.tensor([[word2idx[n] for n in row] for row in names], dtype=torch.int64)
        sentis = table.lookup_tensor(names, 10, det.pad_id)
        d_cpts, d_sentis = det.tag(fc)
        assert torch.equal(d_cpts.cpu(), cpts) and torch.equal(d_sentis.cpu(), sentis)
        host.append((cpts, sentis))
    assert any((s != det.pad_id).any() for _, s in host)
    # Detector.sample: the words derived on the device give the captions of the same call handed the host lookup's tensor
    for i in range(B):
        fc, att = t(batches[0][1][i]).to(DEV), t(batches[0][2][i]).to(DEV)
        want = det.sample(fc, att, host[0][1][i].to(DEV), beam_size=3, decoding_constraint=1)
        got = det.sample(fc, att, None, beam_size=3, decoding_constraint=1)
        assert got == want and len(got[0]) >= 1
    # Detector.forward: a batch with None tensors gives the loss and statistics of the batch that carries the host-tagged ones
    def run(with_none):
        items = []
        for b, (cpts, sentis) in zip(batches, host):
            items.append((b[0], t(b[1]), t(b[2]), (t(b[3][0]), b[3][1]), None if with_none else cpts,
                          None if with_none else sentis, b[6]))
        torch.manual_seed(5)
        # (no_grad: an evaluation forward with gradients enabled leaves the captioner's prologue attributes holding an
        # autograd graph whose nodes refer back to the captioner - the detector would keep its two private streams)
        with torch.no_grad():
            return det((items,), 'fact', False)
    a, b_ = run(False), run(True)
    assert set(a) == set(b_) == {'da_loss', 'fact_reward', 'cls_reward', 'all_rewards', 'cap_loss', 'xe_loss'}
    for k in a:
        assert a[k] == b_[k], (k, a[k], b_[k])
    det.set_concept_detector(cd, None)
    with pytest.raises(ValueError):
        det.sample(t(batches[0][1][0]).to(DEV), t(batches[0][2][0]).to(DEV))
