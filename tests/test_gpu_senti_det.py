"""isc_senti_det_fwd / SentimentDetector.forward_native - the frozen image-sentiment detector's forward on the library's
implicit-GEMM convolution - alone, against the fp64 restatement tests/_senti_det_ref.py.  pytest -m gpu.

Yardstick of the values (post-ReLU conv output, logits, sentiment maps, scores), per case and output:
    |native - fp64| <= 4 * max(e, 2^-23 * max|fp64 value|)
with e = the largest error of the stock fp32 torch module, run on the CPU, against the same fp64 reference - computed in
_senti_det_ref.reference, never from the code under test.  Labels must equal the fp64 labels on every row: each case's
smallest fp64 top-2 probability margin and smallest |score - threshold| are asserted >= 5e-3 first.  The lattice case
(integer features, weights and biases multiples of 1/2; the guarantee is asserted from the operands) must give the conv
output's BITS, on both routes and every grid.  Cases, seeds and the comparison: tests/_senti_det_ref.py."""
import numpy as np
import pytest
import torch

import _senti_det_ref as R
from insenticap_model_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
_PARAMS = {}
ROUTES = {'baseline': 3, 'c128_14x14': 5, 'product': 7}       # case -> forced split of the route tests


def dev_params(key, m):
    """The module's tensors on the device + their packed conv weights, once per case."""
    if key not in _PARAMS:
        params = [p.detach().to(DEV).contiguous() for p in m.native_params()]
        n_convs = sum(1 for p in params if p.dim() == 4 and p.shape[-1] == 3)
        _PARAMS[key] = (params, ops.senti_det_pack(params[0:2 * n_convs:2]))
    return _PARAMS[key]


def run_native(name, feats=None, ksplit=0, c=None, key=None, threshold=None):
    c = c or R.reference(name)
    params, packed = dev_params(key or name, c['m'])
    f = torch.tensor(c['feats']).to(DEV) if feats is None else feats
    thr = c['c']['threshold'] if threshold is None else threshold
    out = ops.senti_det_fwd(params, f, thr, c['neu_idx'], packed=packed, ksplit=ksplit, want_conv_out=True)
    torch.cuda.synchronize()
    return dict(zip(('logits', 'maps', 'labels', 'scores', 'conv_out'), out))


def as_numpy(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_margins(name, c):
    r = c['ref']
    top2, tm = R.top2_margin(r['probs']), R.threshold_margin(r['scores'], c['c']['threshold'])
    assert top2 >= R.MARGIN and tm >= R.MARGIN, 'case %s: margins %.3g / %.3g - change the seed' % (name, top2, tm)


def kinds_delta(before):
    now = ops.senti_det_launches()
    return {k: now[k] - before[k] for k in now}


@pytest.mark.parametrize('name', list(R.CASES))
def test_native_forward_vs_fp64(name):
    c = R.reference(name)
    assert_margins(name, c)
    got = as_numpy(run_native(name))
    R.compare(got, c['ref'], c['e'], name)
    assert got['labels'].dtype == np.int64
    if name == 'thr_2':
        assert (got['labels'] == c['neu_idx']).all()
    ops.check_numerics(name)


@pytest.mark.parametrize('name', list(ROUTES))
def test_both_routes_vs_fp64_and_their_launch_kinds(name):
    c = R.reference(name)
    assert_margins(name, c)
    n = c['c']['n_convs']
    before = ops.senti_det_launches()
    direct = as_numpy(run_native(name, ksplit=1))
    assert kinds_delta(before) == dict(direct=n, split=0, reduce=0, tail=1, pack=0, f16=0)
    before = ops.senti_det_launches()
    split = as_numpy(run_native(name, ksplit=ROUTES[name]))
    assert kinds_delta(before) == dict(direct=0, split=n, reduce=n, tail=1, pack=0, f16=0)
    R.compare(direct, c['ref'], c['e'], name + ' ksplit=1')
    R.compare(split, c['ref'], c['e'], name + ' ksplit=%d' % ROUTES[name])
    # the two routes agree within the bound (both lie within it of the same reference; held directly as well)
    for k in R.VALUE_KEYS:
        assert np.abs(direct[k].astype(np.float64) - split[k]).max() <= R.bound(c['e'][k], c['ref'][k]), k
    assert np.array_equal(direct['labels'], split['labels'])


def test_auto_route_splits_the_contraction_for_one_product_width_image():
    c = R.reference('product')
    one = torch.tensor(c['feats'][:1]).to(DEV)
    before = ops.senti_det_launches()
    got = as_numpy(run_native('product', feats=one))
    d = kinds_delta(before)
    assert d['split'] == 2 and d['reduce'] == 2 and d['direct'] == 0 and d['tail'] == 1
    ref = {k: v[:36] if k == 'conv_out' else v[:1] for k, v in c['ref'].items()}
    R.compare(got, ref, c['e'], 'product[0] auto')
    # and 230 images of the narrow detector (M = 8280: 130 row tiles, at and above half the chip's CUs) run one workgroup
    # per tile, in both layers
    b = R.reference('baseline')
    many = torch.tensor(b['feats']).to(DEV).repeat(7, 1, 1, 1)[:230].contiguous()
    before = ops.senti_det_launches()
    got = run_native('baseline', feats=many)
    d = kinds_delta(before)
    assert d['direct'] == 2 and d['split'] == 0 and d['reduce'] == 0
    R.compare({k: v[:37 * 36] if k == 'conv_out' else v[:37] for k, v in as_numpy(got).items()}, b['ref'], b['e'], 'baseline x 230')


LATTICE_CASES = ('baseline', 'grid_2x3', 'grid_1x1', 'grid_1x5', 'grid_5x1', 'c256_3x3', 'c128_14x14', 'one_image', 'product')


@pytest.mark.parametrize('name', LATTICE_CASES)
def test_lattice_conv_output_in_bits_on_both_routes(name):
    cc = R.case(name)
    w, feats = R.lattice_operands(cc)
    expect = R.lattice_expect(w, feats)                 # (asserts the exactness guarantee from the operands)
    m, _ = R.module(cc, weights=w)
    c = dict(c=cc, m=m, feats=feats, neu_idx=m.neu_idx)
    nchunks_last = 9 * ((cc['C'] >> 1) // 32)
    for ksplit in (1, 2, min(4, nchunks_last), 0):
        before = ops.senti_det_launches()
        got = run_native(name, ksplit=ksplit, c=c, key='lattice/' + name)['conv_out'].cpu().numpy()
        d = kinds_delta(before)
        assert (d['direct'] == 2) if ksplit == 1 else (d['split'] == 2) if ksplit > 1 else (d['direct'] + d['split'] == 2)
        assert got.shape == expect.shape
        bad = np.flatnonzero(got.view(np.uint32) != expect.view(np.uint32))
        assert bad.size == 0, '%s ksplit=%d: %d of %d values differ, first at flat index %d: %r != %r' % (
            name, ksplit, bad.size, got.size, bad[0], got.flat[bad[0]], expect.flat[bad[0]])


@pytest.mark.parametrize('ksplit', [1, 3])
def test_an_image_depends_on_its_own_pixels_alone(ksplit):
    """Every other image replaced by NaN and +-6e4 values: the untouched images' four outputs (and conv rows) keep their
    bits - an out-of-grid tap contributes exact zeros, whatever lies in the neighbouring rows of memory."""
    c = R.reference('baseline')
    clean = run_native('baseline', ksplit=ksplit)
    feats = c['feats'].copy()
    rng = np.random.default_rng(5)
    junk = rng.choice(np.array([np.nan, 6e4, -6e4], np.float32), size=feats[1::2].shape)
    feats[1::2] = junk
    dirty = run_native('baseline', feats=torch.from_numpy(feats).to(DEV), ksplit=ksplit)
    assert ops.device_status(reset=True) & ops.STATUS_NONFINITE_STATS      # the NaN images raise the flag ...
    assert bool((dirty['labels'][1::2] == c['neu_idx']).all())             # ... and read neutral
    for k in ('logits', 'maps', 'labels', 'scores'):
        assert torch.equal(clean[k][0::2], dirty[k][0::2]), k
    hw = 36
    a, b = clean['conv_out'].view(-1, hw, 16)[0::2], dirty['conv_out'].view(-1, hw, 16)[0::2]
    assert torch.equal(a, b)


@pytest.mark.parametrize('name', ['baseline', 'grid_1x5', 'c128_14x14'])
@pytest.mark.parametrize('ksplit', [1, 2])
def test_f16_features_give_the_bits_of_their_up_cast_and_are_read_natively(name, ksplit):
    c = R.reference(name)
    f16 = torch.tensor(c['feats']).to(DEV).half()
    up = run_native(name, feats=f16.float(), ksplit=ksplit)
    before = ops.senti_det_launches()
    nat = run_native(name, feats=f16, ksplit=ksplit)
    assert kinds_delta(before)['f16'] == 1              # the first conv layer read the halfs; nothing was up-cast
    for k in up:
        assert torch.equal(up[k], nat[k]), k


@pytest.mark.parametrize('name', ['baseline', 'product'])
def test_two_runs_give_the_same_bits(name):
    for ksplit in (0, 1, ROUTES[name]):
        a, b = run_native(name, ksplit=ksplit), run_native(name, ksplit=ksplit)
        for k in a:
            assert torch.equal(a[k], b[k]), (k, ksplit)


def test_golden_file_itself():
    import os
    from test_senti_det_ref_host import golden_setup
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'detector.npz'))
    cc, m, w, feats = golden_setup()
    for i, f in enumerate(feats):
        c = dict(c=cc, m=m, feats=f, neu_idx=m.neu_idx)
        got = as_numpy(run_native('golden', c=c, key='golden'))
        assert np.array_equal(got['labels'], g['senti_det/labels%d' % i])
        np.testing.assert_allclose(got['scores'], g['senti_det/scores%d' % i], atol=1e-5)
        np.testing.assert_allclose(got['maps'], g['senti_det/maps%d' % i], atol=1e-4)
        np.testing.assert_allclose(got['logits'], g['senti_det/logits%d' % i], atol=1e-4)


def fresh_module(name='baseline'):
    c = R.reference(name)
    m, _ = R.module(c['c'], weights=c['w'])
    return c, m.to(DEV)


def test_module_follows_an_in_place_change_of_its_weights():
    c, m = fresh_module()
    m.enable_native()
    f = torch.tensor(c['feats']).to(DEV)
    with torch.no_grad():
        assert m.native_active(f)
        before = ops.senti_det_launches()
        a = m.forward_native(f, 0.7)
        b = m.forward_native(f, 0.7)
        assert kinds_delta(before)['pack'] == 2         # packed once for two calls
        conv1 = m.convs.conv_1.weight
        conv1.mul_(-1.0)
        w2 = dict(c['w'])
        w2['convs.conv_1.weight'] = -c['w']['convs.conv_1.weight']
        before = ops.senti_det_launches()
        d = m.forward_native(f, 0.7)
        assert kinds_delta(before)['pack'] == 2         # ... and again for the new version
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    ref2 = R.forward(w2, c['feats'], 0.7, c['neu_idx'])
    got = dict(zip(('logits', 'maps', 'labels', 'scores'), [t.cpu().numpy() for t in d]))
    R.compare(got, ref2, c['e'], 'conv_1 negated', keys=('logits', 'maps'), labels=False)
    assert np.abs(ref2['logits'] - c['ref']['logits']).max() > 1e-2        # (the change is visible at all)


def test_module_contract():
    c, m = fresh_module()
    f = torch.tensor(c['feats']).to(DEV)
    with torch.no_grad():
        assert not m.native_active(f)                   # the default is off
        l0, mp0 = m(f)
        lab0, mp0b, names0, sc0 = m.sample(f, 0.7)
        m.enable_native()
        assert m.native_active(f) and m.native_active(f.half())
        before = ops.senti_det_launches()
        l1, mp1 = m(f)
        lab1, mp1b, names1, sc1 = m.sample(f, 0.7)
        assert kinds_delta(before)['tail'] == 2
        assert not m.train().native_active(f)
        m.eval()
        with ops.exact_fp32_engine():
            assert not m.native_active(f)
            lab2, _, names2, _ = m.sample(f.half(), 0.7)        # the torch code, on its own up-cast
        assert not m.native_active(f.cpu())
    with torch.enable_grad():
        assert not m.native_active(f)                   # grad mode on, parameters require grad
    assert_margins('baseline', c)
    assert lab1.dtype == torch.int64 and torch.equal(lab0, lab1) and names0 == names1
    assert names1 == [m.sentiment_categories[i] for i in c['ref']['labels']]
    assert l1.shape == l0.shape and mp1.shape == mp0.shape == mp1b.shape and sc1.shape == sc0.shape
    got = dict(logits=l1.cpu().numpy(), maps=mp1b.cpu().numpy(), scores=sc1.cpu().numpy(), labels=lab1.cpu().numpy())
    R.compare(got, c['ref'], c['e'], 'module', keys=('logits', 'maps', 'scores'))
    # float16 features that are the fp32 ones rounded decide every row the same way here or not at all: only the form
    assert lab2.shape == lab1.shape and len(names2) == len(names1)


@pytest.mark.parametrize('what', ['k9', 'Cin48', 'hw_over_limit'])
def test_unsupported_shapes_are_refused_before_any_launch(what):
    B, h, w, C, k = 2, 2, 3, 64, 3
    if what == 'k9':
        k = 9
    elif what == 'Cin48':
        C = 96                                          # conv_1 reads 48 channels
    else:
        h, w = 33, 32                                   # 1056 > ISC_SENTI_DET_MAX_HW = 1024
        assert h * w > _lib.SENTI_DET_MAX_HW
    g = torch.Generator().manual_seed(1)
    shapes = [(C // 2, C, 3, 3), (C // 2,), (C // 4, C // 2, 3, 3), (C // 4,), (k, C // 4, 1, 1), (k,), (k, k), (k,), (k, k), (k,)]
    params = [torch.randn(s, generator=g).to(DEV) for s in shapes]
    feats = torch.randn(B, h, w, C, generator=g).to(DEV)
    out = (torch.full((B, k), 7.0, device=DEV), torch.full((B, h, w), 7.0, device=DEV),
           torch.full((B,), 7, dtype=torch.int64, device=DEV), torch.full((B,), 7.0, device=DEV))
    packed = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    before = ops.senti_det_launches()
    with pytest.raises(_lib.HipLibraryError, match='ISC_E_SHAPE'):
        ops.senti_det_fwd(params, feats, 0.7, 2, packed=packed, out=out)
    torch.cuda.synchronize()
    assert ops.senti_det_launches() == before
    assert all(bool((t == 7).all()) for t in out)
