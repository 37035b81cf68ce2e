"""Lattice operands for the split-f16 GEMM kernels: inputs on which the kernels' result is determined bit for bit.

The engine computes  sum hi_a hi_b + 2^-11 sum (hi_a lo_b + lo_a hi_b)  over the f16 planes x = hi + lo 2^-11 of its
operands.  operand() builds x directly from planes hi in s {0, +-1 .. +-hmax} and lo in s {0, +-1/4} (s a power of two):
every product is then exact in fp32, every partial sum of every term is a multiple of the quantum q = 2^-13 s_a s_b, and
a multiple of q below 2^24 q is an fp32 number - so while the sum of the ABSOLUTE values of all terms of an output (and
of whatever the epilogue adds to it) stays below 2^24 q, no partial sum in any order, over any number of waves, slabs,
K chunks or accumulating launches, ever rounds.  expect() evaluates the three-term formula in fp64 and asserts that
bound from the operands, never from a result.  What it returns differs from the true product x_a . x_b by the lo lo
term the engine drops (about 2^-24 per unit of K): a test that holds a kernel to expect() in bits also holds it to the
three-term definition."""
import torch

F64 = torch.float64
LO_STEP = 0.25
PLANE_SCALE = 2.0 ** -11
CHUNK = 32                      # the kernels' k-block


def gen(seed):
    return torch.Generator().manual_seed(seed)


def operand(g, rows, K, hmax, density=1.0, scale=1.0):
    """(x fp32 [rows, K], hi fp64, lo fp64) with x = hi + lo 2^-11 exactly: hi uniform in scale {+-1 .. +-hmax}, lo
    uniform in scale {0, +-1/4}; an entry is zero (both planes) with probability 1 - density.  scale: a power of two."""
    assert hmax in (1, 2) and scale > 0 and float(torch.tensor(scale).log2()) % 1 == 0
    mag = torch.randint(1, hmax + 1, (rows, K), generator=g).to(F64)
    sign = torch.randint(0, 2, (rows, K), generator=g).to(F64) * 2 - 1
    lo = (torch.randint(0, 3, (rows, K), generator=g).to(F64) - 1) * LO_STEP
    hi = mag * sign
    if density < 1.0:
        live = (torch.rand(rows, K, generator=g) < density).to(F64)
        hi, lo = hi * live, lo * live
    hi, lo = hi * scale, lo * scale
    x64 = hi + lo * PLANE_SCALE
    x = x64.float()
    assert torch.equal(x.double(), x64)
    return x, hi, lo


def addend(g, *shape):
    """Small multiples of 2^-13 (|v| <= 2): biases, prior outputs, pre, tab, c_prev."""
    return (torch.randint(-(1 << 14), (1 << 14) + 1, shape, generator=g).to(F64) * 2.0 ** -13).float()


def _unit(t):
    nz = t[t != 0].abs()
    return float(nz.min()) if nz.numel() else 1.0


def quantum(segs):
    """The common quantum q of every term of sum_s (three-term product of segment s); segs = [((hi_a, lo_a), (hi_b,
    lo_b)), ...].  Asserts that the planes are on their lattice: hi / u and 4 lo / u integers, u the smallest |hi|."""
    q = None
    for (ha, la), (hb, lb) in segs:
        ua, ub = _unit(ha), _unit(hb)
        for h, l, u in ((ha, la, ua), (hb, lb, ub)):
            assert torch.equal(h / u, (h / u).round()) and torch.equal(l / (u * LO_STEP), (l / (u * LO_STEP)).round())
        qs = ua * ub * LO_STEP * PLANE_SCALE
        q = qs if q is None else min(q, qs)
    return q


def contract(segs, transposed=False):
    """sum_s hi_a hi_b^T + 2^-11 (hi_a lo_b^T + lo_a hi_b^T) in fp64 (exact there: < 2^53 quanta).  a [M, K], b [N, K];
    transposed: a [K, M], b [K, N] (the TN layout)."""
    z = 0
    for (ha, la), (hb, lb) in segs:
        if transposed:
            ha, la, hb, lb = ha.t(), la.t(), hb.t(), lb.t()
        z = z + ha @ (hb + PLANE_SCALE * lb).t() + PLANE_SCALE * (la @ hb.t())
    return z


def magnitude(segs, transposed=False):
    """An upper bound, per output, of sum_k |hi_a||hi_b| + 2^-11 sum_k (|hi_a||lo_b| + |lo_a||hi_b|) (it adds the
    2^-22 |lo_a||lo_b| term: one product instead of three)."""
    m = 0
    for (ha, la), (hb, lb) in segs:
        if transposed:
            ha, la, hb, lb = ha.t(), la.t(), hb.t(), lb.t()
        m = m + (ha.abs() + PLANE_SCALE * la.abs()) @ (hb.abs() + PLANE_SCALE * lb.abs()).t()
    return m


def expect(segs, addends=(), transposed=False):
    """The kernels' exact result before any non-linear epilogue: the three-term sum of all K-segments plus the addends
    (each broadcastable to [M, N]), in fp64.  Asserts the exactness guarantee from the operands: every addend is a
    multiple of the quantum q, and per output  sum |terms| + sum |addends| < 2^24 q  - which bounds every partial sum in
    any order (q = 2^-13 at scale 1: the bound is 2^11)."""
    q = quantum(segs)
    z, m = contract(segs, transposed), magnitude(segs, transposed)
    for a in addends:
        a = a.to(F64)
        assert torch.equal(a / q, (a / q).round()), 'an addend is off the lattice of quantum %g' % q
        z, m = z + a, m + a.abs()
    worst = float(m.max())
    assert worst < q * 2.0 ** 24, 'exactness guarantee violated: sum of magnitudes %g >= 2^24 q = %g' % (worst, q * 2.0 ** 24)
    return z


def drop_cross(segs, s, chunk, transposed=False):
    """What a kernel that loses lo_a hi_b of segment s for one 32-deep chunk would add to expect(): minus that term."""
    (ha, la), (hb, lb) = segs[s]
    if transposed:
        la, hb = la.t(), hb.t()
    k = slice(chunk * CHUNK, (chunk + 1) * CHUNK)
    return -PLANE_SCALE * (la[:, k] @ hb[:, k].t())


# Every contraction length the GPU file (test_gpu_h3_kernels.py) uses; test_lattice_host.py checks each on the CPU.
GPU_K_TOTALS = (32, 64, 96, 128, 160, 192, 224, 288, 544, 1024, 1088, 2048, 2080, 4128)


def params_for(K):
    """(hmax, density) of both operands for a contraction over K in all, from the guarantee at scale 1 with up to six
    addends (|v| <= 2 each): hmax = 2 needs 4 K + K / 2^10 + 12 < 2^11, i.e. K <= 480; hmax = 1 needs K + ... < 2^11: K <=
    1900 leaves room; beyond that both operands are thinned to density d, the sum of magnitudes is binomial with mean
    d^2 K = ~1100 and a standard deviation below 32 - thirty of them under the bound."""
    if K <= 480:
        return 2, 1.0
    if K <= 1900:
        return 1, 1.0
    return 1, int((1100.0 / K) ** 0.5 * 20) / 20.0
