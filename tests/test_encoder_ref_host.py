"""tests/_encoder_ref.py - the encoder restated from the operator definitions - held to the stock torch operators on the
CPU: F.conv2d, F.batch_norm, F.max_pool2d(ceil_mode=True), F.adaptive_avg_pool2d.  Odd and even sizes, a clipped pool
window (image 32x45 -> 16x23 stem output -> 8x11 pool output with overhanging last windows) and the sizes the stock pool
refuses.  fp64 against fp64: 1e-12 relative."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _encoder_ref as R

F64 = torch.float64


def close(a, b, rel=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float(b.abs().max()) > 0
    assert float((a - b).abs().max()) <= rel * float(b.abs().max())


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


@pytest.mark.parametrize('H,W', [(3, 3), (32, 45), (45, 61), (8, 8)])
def test_stem_convolution_7x7_stride_2_pad_3(H, W):
    x, w = rnd(1, 2, 3, H, W), rnd(2, 8, 3, 7, 7)
    got = R.conv2d(x, w, 2, 3)
    close(got, F.conv2d(x, w, stride=2, padding=3))
    assert got.shape[2:] == ((H - 1) // 2 + 1, (W - 1) // 2 + 1)


@pytest.mark.parametrize('h,w', [(1, 1), (5, 7), (6, 8)])
def test_convolutions_of_the_bottleneck(h, w):
    x = rnd(3, 2, 6, h, w)
    close(R.conv2d(x, rnd(4, 5, 6, 3, 3), 1, 1), F.conv2d(x, rnd(4, 5, 6, 3, 3), padding=1))
    close(R.conv2d(x, rnd(5, 5, 6, 1, 1), 1, 0), F.conv2d(x, rnd(5, 5, 6, 1, 1)))
    s2 = R.conv2d(x, rnd(6, 5, 6, 1, 1), 2, 0)
    close(s2, F.conv2d(x, rnd(6, 5, 6, 1, 1), stride=2))
    assert s2.shape[2:] == ((h - 1) // 2 + 1, (w - 1) // 2 + 1)


def bn_params(seed, n):
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: (torch.rand(n, generator=g, dtype=F64) * (hi - lo) + lo)
    return u(0.5, 1.5), u(-0.2, 0.2), u(-0.2, 0.2), u(0.5, 1.5)          # weight, bias, mean, var


def test_batch_norm_and_its_fold():
    x, w = rnd(7, 2, 6, 5, 7), rnd(8, 10, 6, 3, 3)
    g, b, m, v = bn_params(9, 10)
    y = R.conv2d(x, w, 1, 1)
    want = F.batch_norm(y, m, v, g, b, training=False, eps=1e-5)
    close(R.batch_norm(y, g, b, m, v), want)
    wf, bf = R.fold(w, g, b, m, v)
    close(R.conv2d(x, wf, 1, 1) + bf.view(1, -1, 1, 1), want)            # the fold equals conv-then-BN to 1e-12 relative
    wf32, bf32 = R.fold(w.float(), g.float(), b.float(), m.float(), v.float())
    assert wf32.dtype == F64 and bf32.dtype == F64                       # (fp32 parameters are folded in double)


@pytest.mark.parametrize('h,w', [(2, 2), (3, 3), (4, 5), (16, 23), (23, 31), (8, 11)])
def test_max_pool_ceil_mode_with_clipped_windows(h, w):
    x = rnd(10, 2, 4, h, w)
    got = R.max_pool_ceil(x)
    assert torch.equal(got, F.max_pool2d(x, 3, 2, 0, ceil_mode=True))
    assert got.shape[2:] == (R.pool_out(h), R.pool_out(w)) == ((h - 2) // 2 + 1, (w - 2) // 2 + 1)


def test_the_clipped_window_of_a_32x45_image():
    x = rnd(11, 1, 3, 32, 45)
    stem = R.conv2d(x, rnd(12, 4, 3, 7, 7), 2, 3)
    assert stem.shape[2:] == (16, 23)
    pooled = R.max_pool_ceil(stem)
    assert pooled.shape[2:] == (8, 11)
    # the last row of windows starts at 14 and holds rows 14, 15 only; the last column starts at 20 and holds 20 .. 22
    assert torch.equal(pooled[:, :, 7, 3], stem[:, :, 14:16, 6:9].amax(dim=(2, 3)))
    assert torch.equal(pooled, F.max_pool2d(stem, 3, 2, 0, ceil_mode=True))


@pytest.mark.parametrize('h,w', [(1, 1), (1, 4), (5, 1)])
def test_sizes_the_stock_pool_refuses(h, w):
    x = rnd(13, 1, 2, h, w)
    with pytest.raises(RuntimeError):
        F.max_pool2d(x, 3, 2, 0, ceil_mode=True)
    with pytest.raises(ValueError):
        R.max_pool_ceil(x)


@pytest.mark.parametrize('h,w', [(1, 1), (2, 3), (14, 14), (20, 15), (3, 3)])
@pytest.mark.parametrize('a', [1, 6, 14])
def test_tail(h, w, a):
    x = rnd(14, 2, 5, h, w)
    fc, att = R.tail(x, a)
    close(fc, x.mean(3).mean(2))
    close(att, F.adaptive_avg_pool2d(x, [a, a]).permute(0, 2, 3, 1))
    assert att.shape == (2, a, a, 5)


def test_preprocess_and_im2col():
    u8 = R.make_image(5, 7, 3)
    x = torch.from_numpy(u8.astype('float32') / 255.0).permute(2, 0, 1)
    want = (x - torch.tensor(R.MEAN).view(3, 1, 1)) / torch.tensor(R.STD).view(3, 1, 1)
    assert torch.equal(R.preprocess(u8), want)
    t = rnd(15, 2, 5, 7, 4)                                              # [B, h, w, C]
    w = rnd(16, 6, 4, 3, 3)
    rows = R.im2col(t, 3) @ w.permute(0, 2, 3, 1).reshape(6, 36).t()      # k = tap C + ci
    close(rows.view(2, 5, 7, 6).permute(0, 3, 1, 2), F.conv2d(t.permute(0, 3, 1, 2), w, padding=1))
    rows = R.im2col(t, 1, 2) @ w[:, :, 0, 0].t()
    close(rows.view(2, 3, 4, 6).permute(0, 3, 1, 2), F.conv2d(t.permute(0, 3, 1, 2), w[:, :, :1, :1], stride=2))
