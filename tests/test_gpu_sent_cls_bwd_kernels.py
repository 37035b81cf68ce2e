"""isc_sent_cls_pool_bwd and isc_sent_cls_head_loss alone, against the fp64 restatement tests/_sent_cls_train_ref.py.
pytest -m gpu.  Values: |device - fp64| <= 4 max(e, 2^-23 max|fp64|) with e the error of the same formula evaluated in fp32
numpy on the CPU; counts, predictions and zeros are exact."""
import numpy as np
import pytest
import torch

import _sent_cls_train_ref as R
from insenticap_model_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _dev(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)


def _held(got, ref64, ref32, what):
    e = float(np.abs(np.asarray(ref32, dtype=np.float64) - ref64).max())
    err, bound = R.yardstick(got.double().cpu().numpy(), ref64, e)
    print('%s: err %.3g  fp32-numpy err %.3g  bound %.3g' % (what, err, e, bound))
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize('B,L,H', [(5, 1, 32), (37, 8, 32), (3, 20, 64), (2, 3, 512)])
@pytest.mark.parametrize('how', ['drawn', 'full', 'one'])
def test_pool_bwd(B, L, H, how):
    rng = np.random.default_rng(100 * B + L)
    dfeats, e2 = rng.standard_normal((B, H)).astype(np.float32), (3 * rng.standard_normal((L, B, H))).astype(np.float32)
    o, weights = rng.standard_normal((L, B, H)).astype(np.float32), rng.random((B, L + 3)).astype(np.float32)
    lens = rng.integers(1, L + 1, B)
    lens[0] = L
    if how != 'drawn':
        lens[:] = L if how == 'full' else 1
    r64 = R.pool_bwd(dfeats, e2, o, weights, lens)
    r32 = R.pool_bwd(dfeats, e2, o, weights, lens, dtype=np.float32)
    args = (_dev(dfeats), _dev(e2), _dev(o), _dev(weights), _dev(lens, torch.int32))
    nan = lambda: torch.full((L, B, H), float('nan'), device=DEV)
    de2, d_o, dw = ops.sent_cls_pool_bwd(*args, de2=nan(), d_o=nan())
    again = ops.sent_cls_pool_bwd(*args, de2=nan(), d_o=nan())
    for name, got, a64, a32, rep in zip(('de2', 'd_o', 'dw'), (de2, d_o, dw), r64, r32, again):
        _held(got, a64, a32, name)
        assert torch.equal(got, rep), name                                    # two calls, the same bits
    for b in range(B):                                                        # exact zeros at and past every length
        assert not de2[lens[b]:, b].any() and not d_o[lens[b]:, b].any() and not dw[b, lens[b]:].any()
        assert torch.isfinite(de2[:, b]).all() and torch.isfinite(d_o[:, b]).all()


def test_pool_bwd_refuses_before_launching():
    from insenticap_model_amd._lib import HipLibraryError
    B, L, H = 2, 3, 30                                                        # H % 4 != 0
    z = torch.zeros(L, B, H, device=DEV)
    out = torch.full((L, B, H), 7.0, device=DEV)
    with pytest.raises(HipLibraryError, match='ISC_E_SHAPE'):
        ops.sent_cls_pool_bwd(torch.zeros(B, H, device=DEV), z, z, torch.zeros(B, L, device=DEV),
                              torch.ones(B, dtype=torch.int32, device=DEV), de2=out, d_o=out.clone())
    assert (out == 7.0).all()


@pytest.mark.parametrize('k', [1, 2, 3, 8])
@pytest.mark.parametrize('B', [1, 5, 37])
def test_head_loss(k, B):
    H, g = 64, 8.0
    rng = np.random.default_rng(10 * k + B)
    hid = np.maximum(rng.standard_normal((B, H)), 0).astype(np.float32)
    w3, b3 = rng.standard_normal((k, H)).astype(np.float32), rng.standard_normal(k).astype(np.float32)
    labels = rng.integers(0, k, B)
    r64, r32 = R.head_loss(hid, w3, b3, labels, g), R.head_loss(hid, w3, b3, labels, g, dtype=np.float32)
    srt = np.sort(r64['logits'], axis=1)
    assert k == 1 or (srt[:, -1] - srt[:, -2]).min() >= 1e-3                  # predictions are decided
    o = ops.sent_cls_head_loss(_dev(hid), _dev(w3), _dev(b3), _dev(labels, torch.int64), g)
    o2 = ops.sent_cls_head_loss(_dev(hid), _dev(w3), _dev(b3), _dev(labels, torch.int64), g)
    for n in ('logits', 'loss_rows', 'dhid', 'dw3', 'db3'):
        _held(o[n], r64[n], r32[n], n)
    _held(o['dz'][:, :k], r64['dz'], r32['dz'], 'dz')
    _held(o['loss'], np.asarray([r64['loss']]), np.asarray([r32['loss']]), 'loss')
    assert not o['dz'][:, k:].any()                                           # the columns k..7 are zero
    assert np.array_equal(o['pred'].cpu().numpy(), r64['pred']) and int(o['wrong']) == r64['wrong']
    assert all(torch.equal(o[n], o2[n]) for n in o)


def test_head_loss_saturated_logits_and_ties():
    H, k = 32, 3
    hid = np.zeros((4, H), dtype=np.float32)
    hid[:, 0] = 1.0
    w3 = np.zeros((k, H), dtype=np.float32)
    w3[:, 0] = [80.0, -80.0, 0.0]
    b3 = np.zeros(k, dtype=np.float32)
    labels = np.array([0, 1, 2, 1])
    r64, r32 = R.head_loss(hid, w3, b3, labels), R.head_loss(hid, w3, b3, labels, dtype=np.float32)
    o = ops.sent_cls_head_loss(_dev(hid), _dev(w3), _dev(b3), _dev(labels, torch.int64))
    assert torch.isfinite(o['loss_rows']).all() and torch.isfinite(o['loss']).all() and torch.isfinite(o['dz']).all()
    _held(o['loss_rows'], r64['loss_rows'], r32['loss_rows'], 'loss_rows at +-80')
    _held(o['dz'][:, :k], r64['dz'], r32['dz'], 'dz at +-80')
    # a tie: the lowest index
    w3[:, 0] = [1.0, 2.0, 2.0]
    o = ops.sent_cls_head_loss(_dev(hid), _dev(w3), _dev(b3), _dev(labels, torch.int64))
    assert o['pred'].tolist() == [1, 1, 1, 1] and int(o['wrong']) == 2
    w3[:, 0] = 0.0
    o = ops.sent_cls_head_loss(_dev(hid), _dev(w3), _dev(b3), _dev(labels, torch.int64))
    assert o['pred'].tolist() == [0, 0, 0, 0] and int(o['wrong']) == 3
