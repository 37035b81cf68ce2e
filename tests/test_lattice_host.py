"""tests/_lattice.py on the CPU, at every (hmax, density, K) tests/test_gpu_h3_kernels.py uses: the operands really are
their planes, the expected result really is an fp32 number, the guarantee assertion really fires, and a kernel that lost
one cross term of one 32-deep chunk really would be caught on most outputs."""
import pytest
import torch

import _lattice as L
from _split_f16 import planes

M, N = 70, 130


def split(K):
    """A two-segment split of K (one block first: the shape the skinny cases use), or K alone at one block."""
    return (K,) if K == 32 else (32, K - 32)


def build(K, seed=0, scale_b=1.0):
    g = L.gen(1000 * seed + K)
    hmax, density = L.params_for(K)
    xs, segs = [], []
    for Ks in split(K):
        a, b = L.operand(g, M, Ks, hmax, density), L.operand(g, N, Ks, hmax, density, scale_b)
        xs += [a, b]
        segs.append((a[1:], b[1:]))
    return xs, segs, [L.addend(g, N) for _ in range(3)] + [L.addend(g, M, N)]


def test_the_parameter_rule_covers_both_lattices_and_the_sparse_one():
    got = {L.params_for(K) for K in L.GPU_K_TOTALS}
    assert (2, 1.0) in got and (1, 1.0) in got and any(d < 1.0 for _, d in got)
    assert L.params_for(480) == (2, 1.0) and L.params_for(512)[0] == 1 and L.params_for(1900) == (1, 1.0)


@pytest.mark.parametrize('K', L.GPU_K_TOTALS)
def test_planes_reproduce_the_lattice(K):
    """tests/_split_f16.planes(x) - the library's number format - gives back exactly the (hi, lo) x was built from, at
    scale 1 and at the scales the LSTM / vocabulary cases give their weights."""
    for scale in (1.0, 0.25, 0.125):
        xs, _, _ = build(K, scale_b=scale)
        for x, hi, lo in xs:
            rows, Ks = x.shape
            p = planes(x).view(rows, Ks // 32, 2, 32)
            assert torch.equal(p[:, :, 0].reshape(rows, Ks).double(), hi)
            assert torch.equal(p[:, :, 1].reshape(rows, Ks).double(), lo)
            assert bool(torch.isfinite(x).all()) and torch.equal(x.double(), hi + lo * L.PLANE_SCALE)


@pytest.mark.parametrize('K', L.GPU_K_TOTALS)
def test_expect_is_an_fp32_number_and_every_partial_sum_too(K):
    _, segs, addends = build(K)
    z = L.expect(segs, addends)
    assert torch.equal(z.float().double(), z)
    q = L.quantum(segs)
    assert torch.equal(z / q, (z / q).round())
    # a worst-order partial sum: all positive terms first.  Bounded by the sum of magnitudes, so still on the lattice.
    (ha, la), (hb, lb) = segs[0]
    terms = ha[:, None, :] * hb[None, :, :]                     # [M, N, K0] hi hi products of segment 0
    pos = terms.clamp(min=0).sum(2)
    assert float(pos.max()) < 2.0 ** 24 * q and torch.equal(pos.float().double(), pos)
    # the TN reading of the same data
    zt = L.expect([((ha.t(), la.t()), (hb.t(), lb.t())) for (ha, la), (hb, lb) in segs], addends, transposed=True)
    assert torch.equal(zt, z)


def test_expect_is_the_three_term_formula_not_the_full_product():
    xs, segs, _ = build(416)
    z = L.expect(segs)
    full = sum(xs[2 * s][0].double() @ xs[2 * s + 1][0].double().t() for s in range(len(segs)))
    lolo = L.PLANE_SCALE ** 2 * sum(la @ lb.t() for (_, la), (_, lb) in segs)
    assert torch.equal(full - lolo, z) and float((full - z).abs().max()) > 0


def test_guarantee_fires():
    g = L.gen(5)
    a, b = L.operand(g, 8, 1024, 2), L.operand(g, 8, 1024, 2)            # sum |hi_a||hi_b| ~ 2.25 * 1024 > 2^11
    with pytest.raises(AssertionError, match='exactness guarantee'):
        L.expect([(a[1:], b[1:])])
    ok = [(L.operand(g, 8, 64, 2)[1:], L.operand(g, 8, 64, 2)[1:])]
    L.expect(ok, [L.addend(g, 8)])
    with pytest.raises(AssertionError, match='off the lattice'):
        L.expect(ok, [torch.full((8,), 2.0 ** -15)])
    with pytest.raises(AssertionError, match='exactness guarantee'):
        L.expect(ok, [torch.full((8,), 2048.0)])
    with pytest.raises(AssertionError):                                   # an operand off its lattice
        L.expect([((ok[0][0][0] + 0.3, ok[0][0][1]), ok[0][1])])


@pytest.mark.parametrize('K', L.GPU_K_TOTALS)
def test_one_lost_cross_term_changes_most_outputs(K):
    """The sensitivity the GPU file is for: expect() without lo_a hi_b of ONE 32-deep chunk differs from expect() on more
    than half of the outputs (and wherever it differs, by at least one quantum: 2^-13 = 1.2e-4 at scale 1)."""
    _, segs, addends = build(K, seed=1)
    z = L.expect(segs, addends)
    for s, chunk in {(0, 0), (len(segs) - 1, segs[-1][0][0].shape[1] // 32 - 1)}:
        d = L.drop_cross(segs, s, chunk)
        frac = float((d != 0).double().mean())
        assert frac > 0.5, (K, s, chunk, frac)
        assert float(d[d != 0].abs().min()) >= L.quantum(segs)
        assert not torch.equal((z + d).float(), z.float())
