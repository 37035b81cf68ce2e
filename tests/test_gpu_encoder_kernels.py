"""The encoder's kernels (csrc/encoder.hip), each alone, at the smallest shapes where it can still go wrong.  pytest -m gpu.

Convolution (isc_conv_fwd): lattice operands (tests/_lattice.py: the exactness guarantee is asserted from the operands)
must give the output's BITS - on both routes, with every residual / ReLU combination, ksplit 1, 2 and 3 (3 does not
divide the chunk counts 27, 2 and 1 is capped), the kernel form and the route asserted by counter, two runs equal, and an
image independent of its neighbour's pixels.  Stem and tail: the project's yardstick against the fp64 restatement
(tests/_encoder_ref.py), e = the stock fp32 torch operator's error on the CPU.  Max-pool: bit-equal."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _encoder_ref as R
import _lattice as L
from insenticap_model_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

# name -> (R, stride, B, h, w, Cin, N)
CONV_CASES = {
    'r3_1x1': (3, 1, 1, 1, 1, 32, 32),          # all eight neighbours off-grid
    'r3_5x7': (3, 1, 2, 5, 7, 96, 80),          # M = 70: a 64-row tile and an image border; N % 128 != 0; 27 chunks
    'r1_c32': (1, 1, 2, 5, 7, 32, 48),          # one chunk: the prologue only
    'r1_c64': (1, 1, 2, 5, 7, 64, 144),         # two column tiles
    'r1_s2_5x7': (1, 2, 2, 5, 7, 64, 32),       # -> 3 x 4
    'r1_s2_6x8': (1, 2, 2, 6, 8, 64, 32),       # -> 3 x 4
}


def kinds_delta(before):
    now = ops.encoder_launches()
    return {k: now[k] - before[k] for k in now}


def conv_operands(name):
    Rk, stride, B, h, w, Cin, N = CONV_CASES[name]
    K = Rk * Rk * Cin
    hmax, density = L.params_for(K)
    g = L.gen(sum(map(ord, name)))
    x, xh, xl = L.operand(g, B * h * w, Cin, hmax, density)
    wt, wh, wl = L.operand(g, N, K, hmax, density)          # [N, K], k = tap Cin + ci
    ho, wo = ((h - 1) // 2 + 1, (w - 1) // 2 + 1) if stride == 2 else (h, w)
    bias, res = L.addend(g, N), L.addend(g, B * ho * wo, N)
    col = lambda t: R.im2col(t.view(B, h, w, Cin), Rk, stride)
    segs = [((col(xh), col(xl)), (wh, wl))]
    w4 = wt.view(N, Rk * Rk, Cin).permute(0, 2, 1).reshape(N, Cin, Rk, Rk).contiguous()
    return dict(x=x.view(B, h, w, Cin), w4=w4, bias=bias, res=res, segs=segs, ho=ho, wo=wo)


@pytest.mark.parametrize('name', list(CONV_CASES))
def test_convolution_lattice_bits_on_both_routes(name):
    Rk, stride, B, h, w, Cin, N = CONV_CASES[name]
    o = conv_operands(name)
    x, bias, res = o['x'].to(DEV), o['bias'].to(DEV), o['res'].to(DEV).contiguous()
    before = ops.encoder_launches()
    planes, _ = ops.conv_pack(o['w4'].to(DEV))
    assert kinds_delta(before)['pack'] == 1
    nchunks = Rk * Rk * Cin // 32
    for with_res in (False, True):
        z = L.expect(o['segs'], [o['bias']] + ([o['res']] if with_res else []))       # (asserts the guarantee)
        for relu in (False, True):
            want = (z.clamp_min(0) if relu else z).float().numpy().reshape(B, o['ho'], o['wo'], N)
            for ksplit in (1, 2, 3):
                s = min(ksplit, nchunks)
                before = ops.encoder_launches()
                got = ops.conv_fwd(x, planes, bias, N, Rk, stride, res if with_res else None, relu, ksplit)
                again = ops.conv_fwd(x, planes, bias, N, Rk, stride, res if with_res else None, relu, ksplit)
                d = kinds_delta(before)
                assert d == dict(stem=0, pool=0, direct=2 * (s == 1), split=2 * (s > 1), reduce=2 * (s > 1), tail=0,
                                 pack=0, r1=2 * (Rk == 1), r3=2 * (Rk == 3)), (ksplit, d)
                assert torch.equal(got, again)
                got = got.cpu().numpy()
                bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
                assert bad.size == 0, '%s res=%d relu=%d ksplit=%d: %d of %d values differ, first at %d: %r != %r' % (
                    name, with_res, relu, ksplit, bad.size, got.size, bad[0], got.flat[bad[0]], want.flat[bad[0]])
    if relu:
        assert (want == 0).any() and (want > 0).any()


def test_convolution_auto_route_by_the_cost_rule():
    # 27 chunks over 2 tiles: the rule splits (13 shares of >= 2 chunks); one chunk: direct
    for name, split in (('r3_5x7', True), ('r1_c32', False)):
        Rk, stride, B, h, w, Cin, N = CONV_CASES[name]
        o = conv_operands(name)
        planes, _ = ops.conv_pack(o['w4'].to(DEV))
        before = ops.encoder_launches()
        got = ops.conv_fwd(o['x'].to(DEV), planes, o['bias'].to(DEV), N, Rk, stride)
        d = kinds_delta(before)
        assert (d['split'], d['reduce'], d['direct']) == ((1, 1, 0) if split else (0, 0, 1))
        want = L.expect(o['segs'], [o['bias']]).float().view(B, o['ho'], o['wo'], N)
        assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize('name', [n for n, c in CONV_CASES.items() if c[2] >= 2])      # (every case with a neighbour)
@pytest.mark.parametrize('ksplit', [1, 3])
def test_an_image_depends_on_its_own_pixels_alone(name, ksplit):
    Rk, stride, B, h, w, Cin, N = CONV_CASES[name]
    o = conv_operands(name)
    planes, _ = ops.conv_pack(o['w4'].to(DEV))
    bias = o['bias'].to(DEV)
    clean = ops.conv_fwd(o['x'].to(DEV), planes, bias, N, Rk, stride, ksplit=ksplit)
    x = o['x'].clone()
    junk = np.random.default_rng(5).choice(np.array([np.nan, 6e4, -6e4], np.float32), size=tuple(x[1].shape))
    x[1] = torch.from_numpy(junk)
    dirty = ops.conv_fwd(x.to(DEV), planes, bias, N, Rk, stride, ksplit=ksplit)
    assert torch.equal(clean[0], dirty[0]) and not torch.equal(clean[1], dirty[1])
    x = o['x'].clone()
    x[0] = torch.from_numpy(junk)
    dirty = ops.conv_fwd(x.to(DEV), planes, bias, N, Rk, stride, ksplit=ksplit)
    assert torch.equal(clean[1], dirty[1])


def test_convolution_pack_folds_the_batch_norm_in_double():
    g = torch.Generator().manual_seed(4)
    w = torch.randn(48, 64, 3, 3, generator=g)
    bn = [torch.rand(48, generator=g) + 0.5, torch.rand(48, generator=g) * 0.4 - 0.2,
          torch.rand(48, generator=g) * 0.4 - 0.2, torch.rand(48, generator=g) + 0.5]
    planes, bias = ops.conv_pack(w.to(DEV), [t.to(DEV) for t in bn])
    wf, bf = R.fold(w, *bn)
    assert torch.equal(bias.cpu(), bf.float())
    # planes [N, 2 K]: per 32-deep k-block 32 hi then 32 lo halfs; hi + lo 2^-11 restores w' to the split's precision
    pl = planes.view(torch.float16)[:48 * 2 * 576].view(48, 18, 2, 32).cpu().double()
    back = (pl[:, :, 0] + pl[:, :, 1] * 2.0 ** -11).reshape(48, 9, 64).permute(0, 2, 1).reshape(48, 64, 3, 3)
    want = wf.float().double()
    assert float((back - want).abs().max()) <= 2.0 ** -21 * float(want.abs().max())
    hi = wf.float().half()
    assert torch.equal(pl[:, :, 0].reshape(48, 9, 64).permute(0, 2, 1).reshape(48, 64, 3, 3), hi.double())


# ------------------------------------------------------------------ stem
def stem_case(H, W, C0=32, B=2):
    g = torch.Generator().manual_seed(H * 100 + W)
    u8 = R.make_image(H, W, H + W, B=B)
    w = (torch.rand(C0, 3, 7, 7, generator=g) * 2 - 1) / 147 ** 0.5
    bn = [torch.rand(C0, generator=g) + 0.5, torch.rand(C0, generator=g) * 0.4 - 0.2,
          torch.rand(C0, generator=g) * 0.4 - 0.2, torch.rand(C0, generator=g) + 0.5]      # weight, bias, mean, var
    x = torch.stack([R.preprocess(i) for i in u8])                                          # [B, 3, H, W] fp32
    ref = R.batch_norm(R.conv2d(x.double(), w.double(), 2, 3), *[t.double() for t in bn]).clamp_min(0)
    stock = F.relu(F.batch_norm(F.conv2d(x, w, stride=2, padding=3), bn[2], bn[3], bn[0], bn[1], False, 0.0, 1e-5))
    ref = ref.permute(0, 2, 3, 1).numpy()
    e = float(np.abs(stock.permute(0, 2, 3, 1).double().numpy() - ref).max())
    return u8, x, w, bn, ref, e


@pytest.mark.parametrize('H,W', [(3, 3), (32, 45), (45, 61)])
@pytest.mark.parametrize('C0', [32, 64])
def test_stem_uint8_and_fp32_inputs(H, W, C0):
    u8, x, w, bn, ref, e = stem_case(H, W, C0)
    before = ops.encoder_launches()
    wk, bias = ops.encoder_stem_pack(w.to(DEV), [t.to(DEV) for t in bn])
    from_u8 = ops.encoder_stem(torch.from_numpy(u8).to(DEV), wk, bias)
    from_f32 = ops.encoder_stem(x.permute(0, 2, 3, 1).contiguous().to(DEV), wk, bias)
    d = kinds_delta(before)
    assert d['stem'] == 2 and d['pack'] == 1
    b = R.bound(e, ref)
    for what, got in (('uint8', from_u8), ('fp32', from_f32)):
        got = got.cpu().numpy()
        assert got.shape == ref.shape == (2, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C0)
        err = float(np.abs(got - ref).max())
        print('stem %dx%d C0=%d %s: err %.3g, stock fp32 e %.3g, bound %.3g' % (H, W, C0, what, err, e, b))
        assert err <= b
    # the fused normalisation is Encoder.preprocess: the two inputs give the same values within the yardstick
    diff = float((from_u8 - from_f32).abs().max())
    print('stem %dx%d C0=%d: |uint8 path - fp32 path| = %.3g' % (H, W, C0, diff))
    assert diff <= b
    assert (ref == 0).any() and (ref > 0).any()


# ------------------------------------------------------------------ max-pool
@pytest.mark.parametrize('h,w', [(2, 2), (16, 23), (23, 31)])
def test_max_pool_bit_equal(h, w):
    x = torch.randn(2, 32, h, w, generator=torch.Generator().manual_seed(h))
    want = R.max_pool_ceil(x).permute(0, 2, 3, 1).contiguous()
    before = ops.encoder_launches()
    got = ops.encoder_maxpool(x.permute(0, 2, 3, 1).contiguous().to(DEV))
    assert kinds_delta(before)['pool'] == 1
    assert torch.equal(got.cpu(), want)


# ------------------------------------------------------------------ tail
@pytest.mark.parametrize('h,w', [(1, 1), (2, 3), (14, 14), (20, 15)])
@pytest.mark.parametrize('a', [1, 6, 14])
def test_tail(h, w, a):
    x = torch.randn(2, 96, h, w, generator=torch.Generator().manual_seed(h * 31 + a)).clamp_min(0)    # post-ReLU features
    fc64, att64 = R.tail(x.double(), a)
    efc = float((x.mean(3).mean(2).double() - fc64).abs().max())
    eatt = float((F.adaptive_avg_pool2d(x, [a, a]).permute(0, 2, 3, 1).double() - att64).abs().max())
    before = ops.encoder_launches()
    fc, att, fc16, att16 = ops.encoder_tail(x.permute(0, 2, 3, 1).contiguous().to(DEV), a, want_f16=True)
    again = ops.encoder_tail(x.permute(0, 2, 3, 1).contiguous().to(DEV), a)
    assert kinds_delta(before)['tail'] == 2
    assert att.shape == (2, a, a, 96) and fc.shape == (2, 96)
    for what, got, ref, e in (('fc', fc, fc64, efc), ('att', att, att64, eatt)):
        err, b = float((got.cpu().double() - ref).abs().max()), R.bound(e, ref.numpy())
        print('tail %dx%d a=%d %s: err %.3g, stock fp32 e %.3g, bound %.3g' % (h, w, a, what, err, e, b))
        assert err <= b
    assert torch.equal(fc16, fc.half()) and torch.equal(att16, att.half())
    assert torch.equal(again[0], fc) and torch.equal(again[1], att)


# ------------------------------------------------------------------ refusals: the code, and the outputs untouched
def test_refused_shapes_return_their_code_with_the_outputs_untouched():
    lib = _lib.load()
    sentinel = 12345.0

    def refused(fn, code, out):
        with pytest.raises(_lib.HipLibraryError) as ei:
            fn()
        assert code in str(ei.value), str(ei.value)
        torch.cuda.synchronize()
        assert bool((out == sentinel).all())

    # Cin % 32 != 0
    out = torch.full((1, 2, 2, 32), sentinel, device=DEV)
    x = torch.zeros(1, 2, 2, 48, device=DEV)
    planes, bias = torch.zeros(4 * 32 * 64, dtype=torch.uint8, device=DEV), torch.zeros(32, device=DEV)
    refused(lambda: ops.conv_fwd(x, planes, bias, 32, 1, out=out), 'ISC_E_SHAPE', out)
    x = torch.zeros(1, 2, 2, 64, device=DEV)
    refused(lambda: ops.conv_fwd(x, planes, bias, 24, 1, out=out), 'ISC_E_SHAPE', out)             # N % 16 != 0
    refused(lambda: ops.conv_fwd(x, planes, bias, 32, 3, stride=2, out=out), 'ISC_E_SHAPE', out)   # 3x3 is stride 1
    # a short workspace (the split route needs slabs) and a misaligned pointer
    short = torch.zeros(256, dtype=torch.uint8, device=DEV)
    refused(lambda: ops.conv_fwd(x, planes, bias, 32, 1, ksplit=2, out=out, workspace=short), 'ISC_E_WORKSPACE', out)
    off = torch.zeros(1 * 2 * 2 * 64 + 1, device=DEV)[1:].view(1, 2, 2, 64)
    refused(lambda: ops.conv_fwd(off, planes, bias, 32, 1, out=out), 'ISC_E_ALIGN', out)
    # an image under 3 px: the stem's 1x1 grid has no pooled output
    pool_out = torch.full((1, 1, 1, 32), sentinel, device=DEV)
    refused(lambda: ops.encoder_maxpool(torch.zeros(1, 1, 4, 32, device=DEV), out=pool_out), 'ISC_E_SHAPE', pool_out)
    enc = R.encoder('n1111')
    import copy
    dev_enc = copy.deepcopy(enc).to(DEV)
    packed = dev_enc.packed()
    before = ops.encoder_launches()
    for H, W in ((2, 5), (5, 2)):
        with pytest.raises(_lib.HipLibraryError) as ei:
            ops.encoder_fwd(packed, torch.zeros(1, H, W, 3, dtype=torch.uint8, device=DEV), (1, 1, 1, 1), 32)
        assert 'ISC_E_SHAPE' in str(ei.value)
    with pytest.raises(_lib.HipLibraryError) as ei:
        ops.encoder_fwd(packed, torch.zeros(1, 33, 33, 3, dtype=torch.uint8, device=DEV), (1, 1, 1, 1), 32,
                        workspace=torch.zeros(1024, dtype=torch.uint8, device=DEV))
    assert 'ISC_E_WORKSPACE' in str(ei.value)
    with pytest.raises(_lib.HipLibraryError) as ei:
        ops.encoder_fwd(packed[:4096], torch.zeros(1, 33, 33, 3, dtype=torch.uint8, device=DEV), (1, 1, 1, 1), 32)
    assert 'ISC_E_WORKSPACE' in str(ei.value)
    assert kinds_delta(before) == {k: 0 for k in _lib.ENCODER_KINDS}
    assert lib.isc_conv_workspace_bytes(1, 2, 2, 48, 32, 1, 1, 0) == 0
