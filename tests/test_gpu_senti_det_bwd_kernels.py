"""The kernels of the image-sentiment detector's reverse sweep (csrc/senti_det.hip), each on its own at its edge shapes:
the implicit-TN weight-gradient kernel (isc_senti_det_dw) on lattice operands - equal bits - and on random operands under
the yardstick, the flipped-transposed weight pack against the host formula in bits, and the tail backward for k = 1, 3, 8
and h w = 1, 25, 196 - through the sweep of a one-conv detector (everything behind x2) and by what its two launches leave
in the workspace.  pytest -m gpu."""
import numpy as np
import pytest
import torch

import _lattice as L
import _senti_det_train_cases as Cs
import _senti_det_train_ref as R
from insenticap_model_amd import ops
from insenticap_model_amd.train import senti_det_loss_with_grad

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

# (Cin, Cout, h, w, B, ld of dy): one pixel (eight taps out of grid); 75 rows (a partial chunk pair, image borders inside
# a chunk); 1332 rows (many chunks, odd h w against the row pairs); Cin % 128 == 0 (the tap-fastest tile order);
# 9 Cin and Cout no multiples of the tile (partial tiles on both sides); padded dy rows
DW_SHAPES = [(32, 16, 1, 1, 3, 16), (32, 16, 5, 5, 3, 32), (64, 32, 6, 6, 37, 32), (128, 64, 3, 3, 2, 64),
             (160, 80, 2, 3, 2, 96), (32, 16, 1, 5, 2, 16), (32, 16, 5, 1, 2, 16), (256, 144, 3, 3, 1, 160)]


def _shift(t, B, h, w, ky, kx):
    """rows m = (b, y, x) of t [B h w, C] -> the rows of pixel (y + ky - 1, x + kx - 1), zeros outside the grid."""
    C = t.shape[1]
    pad = torch.zeros(B, h + 2, w + 2, C, dtype=t.dtype)
    pad[:, 1:h + 1, 1:w + 1] = t.reshape(B, h, w, C)
    return pad[:, ky:ky + h, kx:kx + w].reshape(B * h * w, C)


@pytest.mark.parametrize('shape', DW_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_dw_kernel_on_lattice_operands_in_bits(shape):
    Cin, Cout, h, w, B, ld = shape
    M = B * h * w
    g = L.gen(11)
    hmax, density = L.params_for(max(M, 32))
    dy, dy_hi, dy_lo = L.operand(g, M, Cout, hmax, density)
    x, x_hi, x_lo = L.operand(g, M, Cin, hmax, density)
    want = torch.empty(Cout, Cin, 3, 3, dtype=L.F64)
    for ky in range(3):
        for kx in range(3):
            seg = ((dy_hi, dy_lo), (_shift(x_hi, B, h, w, ky, kx), _shift(x_lo, B, h, w, ky, kx)))
            want[:, :, ky, kx] = L.expect([seg], transposed=True)
    dy_ld = torch.full((M, ld), 7.0)                          # (what stands in the padding columns is never read)
    dy_ld[:, :Cout] = dy
    got = ops.senti_det_dw(dy_ld.to(DEV), x.reshape(B, h, w, Cin).to(DEV), Cout)
    assert torch.equal(got.cpu().double(), want)
    # ratio and unscale: exact powers of two per image and for the whole sum
    ratio = torch.tensor([2.0 ** -(b % 3) for b in range(B)])
    got2 = ops.senti_det_dw((dy_ld / ratio.repeat_interleave(h * w)[:, None]).to(DEV), x.reshape(B, h, w, Cin).to(DEV),
                            Cout, ratio=ratio.to(DEV), unscale=torch.tensor([0.25], device=DEV))
    assert torch.equal(got2.cpu().double(), want * 0.25)


@pytest.mark.parametrize('shape', [(32, 16, 5, 5, 3, 16), (64, 32, 6, 6, 37, 32), (128, 64, 14, 14, 2, 64)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_dw_kernel_on_random_operands_vs_fp64(shape):
    Cin, Cout, h, w, B, ld = shape
    rng = np.random.default_rng(5)
    dy = rng.standard_normal((B, h, w, Cout)).astype(np.float32)
    x = rng.standard_normal((B, h, w, Cin)).astype(np.float32)
    ref = R.conv_dw(dy.astype(np.float64), x.astype(np.float64))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    wt = torch.zeros(Cout, Cin, 3, 3, requires_grad=True)
    (torch.nn.functional.conv2d(xt, wt, padding=1) * torch.from_numpy(dy).permute(0, 3, 1, 2)).sum().backward()
    e = float(np.abs(wt.grad.double().numpy() - ref).max())
    got = ops.senti_det_dw(torch.from_numpy(dy).reshape(-1, Cout).to(DEV), torch.from_numpy(x).to(DEV), Cout)
    err, bound = R.yardstick(got.cpu().numpy(), ref, e)
    print('dw %s: err %.3g  fp32-cpu err %.3g  bound %.3g' % (shape, err, e, bound))
    assert err <= bound


def _planes_host(mat):
    """fp32 [rows, K] -> the float16 planes [rows, 2 K] of csrc/common.h: per 32-deep k-block 32 hi then 32 lo."""
    hi = mat.astype(np.float16)
    lo = ((mat - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    rows, K = mat.shape
    out = np.empty((rows, K // 32, 2, 32), np.float16)
    out[:, :, 0] = hi.reshape(rows, K // 32, 32)
    out[:, :, 1] = lo.reshape(rows, K // 32, 32)
    return out.reshape(rows, 2 * K)


@pytest.mark.parametrize('shape', [(16, 32), (32, 64), (80, 160), (512, 1024)], ids=lambda s: '%dx%d' % s)
def test_flipped_transposed_pack_in_bits(shape):
    Cout, Cin = shape
    w = np.random.default_rng(6).standard_normal((Cout, Cin, 3, 3)).astype(np.float32) * np.float32(0.05)
    Cp = (Cout + 31) // 32 * 32
    mat = np.zeros((Cin, 9, Cp), np.float32)                    # [ci, tap', co]: tap' = (2 - ky) 3 + (2 - kx)
    mat[:, :, :Cout] = R.flipped(w).reshape(Cin, Cout, 9).transpose(0, 2, 1)
    got = ops.senti_det_pack_flipped(torch.from_numpy(w).to(DEV)).cpu().numpy()
    assert np.array_equal(got.view(np.uint16), _planes_host(mat.reshape(Cin, 9 * Cp)).view(np.uint16))


@pytest.mark.parametrize('k', [1, 3, 8])
@pytest.mark.parametrize('hw', [(1, 1), (5, 5), (14, 14)], ids=['hw1', 'hw25', 'hw196'])
def test_tail_backward_alone(k, hw):
    """A one-conv detector at C = 32: behind x2 the sweep is the tail backward alone - the FC gradients, d senti_conv,
    and dx2 read through conv_0's bias gradient (its column sums) and weight gradient.  k = 1: the loss and every
    gradient are zero, exactly."""
    c = dict(C=32, h=hw[0], w=hw[1], B=5, n_convs=1, n_fcs=2, k=k)
    m, w = Cs.module(c)
    seed = R.find_seed(lambda s: R.forward_backward(w, *Cs.inputs(c, s))[2])
    feats, labels = Cs.inputs(c, seed)
    L64, G64, _ = R.forward_backward(w, feats, labels)
    eL, eG, _, _ = Cs.cpu_error(m, feats, labels, L64, G64)
    m = m.to(DEV)
    m.zero_grad()
    loss = senti_det_loss_with_grad(m, torch.from_numpy(feats).to(DEV), torch.from_numpy(labels).to(DEV))
    loss.backward()
    err, bound = R.yardstick(loss.detach().cpu().numpy(), np.asarray(L64), eL)
    assert err <= bound
    for n, p in m.named_parameters():
        err, bound = R.yardstick(p.grad.cpu().numpy(), G64[n], eG[n])
        print('k %d hw %s %s: err %.3g  fp32-cpu err %.3g  bound %.3g' % (k, hw, n, err, eG[n], bound))
        assert err <= bound, n
        if k == 1:
            assert not p.grad.any()


@pytest.mark.parametrize('k', [1, 3, 8])
@pytest.mark.parametrize('hw', [(1, 1), (5, 5), (14, 14)], ids=['hw1', 'hw25', 'hw196'])
def test_tail_backward_kernels_outputs(k, hw):
    """What the two tail-backward launches leave in the workspace, each against fp64 to 2^-16 of its largest element: they
    are fp32 sums of at most 196 + 8 terms over inputs that carry the forward's few 2^-23, so the worst case of a
    sequential sum, 212 x 2^-24 < 2^-16, bounds them, and a wrong or missing term shows at 2^-8 and above.  The
    gradient of every FC output, dpool, sum_p r, dr; and the scales - e_b the power of two that brings max_c |dr[b,c]|
    into [1, 2) (computed here from the device's own dr, exactly), E / e_b with E = min_b e_b."""
    import _senti_det_ref as S
    from insenticap_model_amd import ops
    c = dict(C=32, h=hw[0], w=hw[1], B=5, n_convs=1, n_fcs=2, k=k)
    m, w = Cs.module(c)
    seed = R.find_seed(lambda s: R.forward_backward(w, *Cs.inputs(c, s))[2])
    feats, labels = Cs.inputs(c, seed)
    _, _, aux = R.forward_backward(w, feats, labels)
    convs, (Ws, bs), fcs = S.split_weights(w)
    B, npix = 5, hw[0] * hw[1]
    g = aux['prob'].copy()
    g[np.arange(B), labels] -= 1.0
    g /= B
    want_g = [None, None]
    for l in (1, 0):
        want_g[l] = g
        g = g @ fcs[l][0]
    want = dict(dpool=g, rsum=aux['r'].sum(axis=(1, 2)), dr=(g / npix) @ Ws)
    m = m.to(DEV)
    st = ops.senti_det_train_fwd([p.detach() for p in m.native_params()], torch.from_numpy(feats).to(DEV),
                                 torch.from_numpy(labels).to(DEV))
    ops.senti_det_bwd(st)
    torch.cuda.synchronize()
    got = {n: v.cpu().numpy().astype(np.float64) for n, v in ops.senti_det_bwd_tail(st).items()}

    def close(a, b, what):
        assert np.abs(a - b).max() <= 2.0 ** -16 * np.abs(b).max(), what

    for l in (0, 1):
        close(got['g'][l][:, :k], want_g[l], 'g%d' % l)
    close(got['dpool'][:, :k], want['dpool'], 'dpool')
    close(got['rsum'], want['rsum'], 'rsum')
    close(got['dr'], want['dr'], 'dr')
    mx = np.abs(got['dr']).max(axis=1)
    eb = np.where(mx > 0, 2.0 ** -np.floor(np.log2(np.where(mx > 0, mx, 1.0))), 2.0 ** 126)
    assert np.array_equal(got['eb'], eb)
    assert np.array_equal(got['ratio'], eb.min() / eb)
    if k > 1:
        assert ((mx * eb >= 1.0) & (mx * eb < 2.0)).all()
