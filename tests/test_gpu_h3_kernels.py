"""The split-f16 GEMM kernels of csrc/gemm_f32.hip, one by one: every case names the instantiation it means to run,
proves with the launch counters (ops.h3_kernel_launches and the older ones) that this instantiation and no other ran,
and holds the result to exact bits.

Operands are lattice operands (tests/_lattice.py): built from their planes so that every product and every partial sum
of  sum hi_a hi_b + 2^-11 sum (hi_a lo_b + lo_a hi_b)  is an fp32 number - the kernel's output is then determined bit for
bit whatever its summation order, and the reference is the fp64 evaluation of that formula (L.expect, which asserts the
guarantee from the operands).  The comparison is torch.equal.  A kernel that loses one cross term of one 32-deep chunk
(a stale ring buffer, a wrong f32_bufs bit at a segment switch, a wave whose K range starts one block off) changes more
than half of a case's outputs by at least 2^-13 (tests/test_lattice_host.py).

Routes ("The split-f16 engine: which route reaches which kernel").  route_nt asks gemv_plan, h3s_plan,
plan_splitk, h3_plan in this order.  Mode 2 switches the first two off and lets h3_plan take any tile count; modes 3 / 4
force the skinny 32 x 32 / 64 x 64 tile without a weights scope.  plan_splitk stands down for N % 4 != 0, for fewer than
8 chunks, for 384 or more 32-row blocks, or for a workspace below 2 sum(M N) floats: every case hands the launch a private
workspace just large enough for its weight planes (and slabs), followed by sentinel floats that must survive, and
no_f32_split() asserts on the host that one of those reasons holds.

Outputs sit in sentinel-filled buffers with ldc > N (ldc == N with a keep-mask) and one extra row."""
import copy
import functools

import numpy as np
import pytest
import torch

import _lattice as L
from _split_f16 import planes as _planes
from insenticap_model_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = 7.25
ISENT = 123456789
F32, F64 = torch.float32, torch.float64
NAMES = tuple(range(17)) + ('h3', 'h3x', 'h3s', 'f16a') + tuple('f32_%d' % k for k in range(7)) + ('gemv',)
TILE_KIND = {128: 0, 256: 3, 64: 6}               # + 0 planes / + 1 fp32 rows
S32, S32_W8, S64, SV, SV_W8, V_PLANES, V_F32, SPLIT = 9, 10, 11, 12, 13, 14, 15, 16


@pytest.fixture(autouse=True)
def _restore_routing():
    lib = _lib.load()
    mode, rows = ops.h3_mode(), ops.set_gemv_rows(8)
    ops.set_gemv_rows(rows)
    h3v = ops.set_h3v(1)
    ops.set_h3v(h3v)
    ksplit = lib.isc_set_h3_ksplit(1)
    lib.isc_set_h3_ksplit(ksplit)
    yield
    ops.set_tile_override(-1)
    ops.set_h3_mode(mode)
    ops.set_gemv_rows(rows)
    ops.set_h3v(h3v)
    lib.isc_set_h3_ksplit(ksplit)


# ------------------------------------------------------------------------------------------------ helpers
def counters():
    lib = _lib.load()
    return (tuple(ops.h3_kernel_launches(k) for k in range(17)) +
            (lib.isc_h3_launches(), lib.isc_h3x_launches(), lib.isc_h3s_launches(), lib.isc_h3_f16a_launches()) +
            tuple(ops.f32_launches(k) for k in range(7)) + (lib.isc_gemv_launches(),))


class ran:
    """`with ran({name: n, ...}):` - exactly these counters went up, by exactly n: the 17 kinds of ops.h3_kernel_launches
    (int keys), isc_h3 / h3x / h3s / h3_f16a_launches, the seven ops.f32_launches kinds ('f32_6' = the reduce behind a K
    split) and isc_gemv_launches."""

    def __init__(self, want):
        self.want = want

    def __enter__(self):
        self.before = counters()
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            delta = {n: a - b for n, a, b in zip(NAMES, counters(), self.before) if a != b}
            assert delta == self.want, 'launch counters moved by %r, expected %r' % (delta, self.want)
        return False


def private_ws(floats):
    """(whole buffer, the declared workspace): `floats` floats followed by 64 sentinels."""
    buf = torch.full((floats + 64,), SENT, device=DEV)
    assert buf.data_ptr() % 256 == 0
    return buf, buf[:floats]


def ws_intact(buf, floats):
    assert bool((buf[floats:] == SENT).all()), 'the launch wrote past its declared workspace'


def set_ws(problem, ws):
    problem.splitk_ws, problem.splitk_ws_floats = ws.data_ptr(), ws.numel()


def no_f32_split(shapes, ws_floats):
    """plan_splitk declines [(M, N, (K_s ...)), ...] with this workspace - asserted from its code, not from a run."""
    blocks = sum((M + 31) // 32 * ((N + 127) // 128) for M, N, _ in shapes)
    chunks = min(sum(K // 32 for K in Ks) for _, _, Ks in shapes)
    assert (any(N % 4 for _, N, _ in shapes) or blocks >= 384 or min(768 // blocks, 16, chunks // 4) < 2 or
            ws_floats < 2 * sum(M * N for M, N, _ in shapes)), 'plan_splitk would take this launch first'


def planes_need(shapes):
    return sum(N * sum(Ks) + 1024 for _, N, Ks in shapes)


def exact32(z):
    """fp64 lattice values as the fp32 tensor the kernel must produce; the guarantee makes the conversion exact."""
    v = z.float()
    assert torch.equal(v.double(), z)
    return v


def outbuf(M, N, ldc, prior=None):
    buf = torch.full((M + 1, ldc), SENT, device=DEV)
    if prior is not None:
        buf[:M, :N] = prior.to(DEV)
    return buf, buf[:M, :N]


def hold(buf, want, what):
    """buf [M + 1, ld] equals want [M, N] in bits; the extra row and the columns past N keep the sentinel."""
    got = buf.detach().cpu()
    sent = ISENT if got.dtype == torch.int32 else SENT
    M, N = want.shape
    assert bool((got[M:] == sent).all()), '%s: the row past M lost its sentinel' % what
    assert bool((got[:M, N:] == sent).all()), '%s: a column past N lost its sentinel' % what
    if not torch.equal(got[:M, :N], want):
        bad = got[:M, :N] != want
        r, c = [int(v[0]) for v in bad.nonzero(as_tuple=True)]
        raise AssertionError('%s: %d of %d outputs differ in bits, first at (%d, %d): got %r, want %r, max |d| %.3e' % (
            what, int(bad.sum()), bad.numel(), r, c, float(got[r, c]), float(want[r, c]),
            float((got[:M, :N].double() - want.double()).abs().nan_to_num(nan=float('inf')).max())))


class Opd:
    """A lattice operand [rows, K] of a contraction over Ktot in all: host planes, the device tensor (wide: a column slice
    of a NaN-filled wider one, ld = K + 16) and, on demand, its device plane buffer."""

    def __init__(self, g, rows, K, Ktot, scale=1.0, wide=False, tie_rows=False):
        assert Ktot in L.GPU_K_TOTALS, Ktot
        hmax, density = L.params_for(Ktot)
        self.x, hi, lo = L.operand(g, rows, K, hmax, density, scale)
        if tie_rows:                                      # rows 64 .. 95 of every 128 repeat rows 0 .. 31: tied logits
            for t0 in range(0, rows, 128):
                n = min(32, rows - (t0 + 64))
                if n > 0:
                    for t in (self.x, hi, lo):
                        t[t0 + 64:t0 + 64 + n] = t[t0:t0 + n]
        self.pl = (hi, lo)
        if wide:
            whole = torch.full((rows, K + 16), float('nan'))
            whole[:, 8:8 + K] = self.x
            self.whole = whole.to(DEV)
            self.d = self.whole[:, 8:8 + K]
        else:
            self.d = self.x.to(DEV)
        self._planes = None

    @property
    def planes(self):
        if self._planes is None:
            self._planes = _planes(self.d.contiguous())
        return self._planes


def seg_tuple(a, w, form):
    return (a.d, w.d, a.planes) if form == 'p' else (a.d, w.d)


# ------------------------------------------------------------------------------------------------ 1. linear epilogue
class Linear:
    """One linear problem on lattice operands: forms[s] = 'p' (segment s comes with planes) or 'r' (fp32 rows)."""

    def __init__(self, seed, M, N, Ks, forms, ldc=None, nbias=0, acc=False, relu=False, mask=False, wide=False, A=None):
        g = L.gen(seed)
        assert len(Ks) == len(forms)
        self.M, self.N, self.Ks, self.forms, self.Kt = M, N, tuple(Ks), forms, sum(Ks)
        self.ldc = N if mask else (ldc or (N + 3) // 4 * 4 + 4)          # the keep-mask is read with ld = N
        self.A = A or [Opd(g, M, K, self.Kt, wide=wide) for K in Ks]
        self.W = [Opd(g, N, K, self.Kt, wide=wide) for K in Ks]
        self.biases = [L.addend(g, N) for _ in range(nbias)]
        self.dbiases = [b.to(DEV) for b in self.biases] + [None] * (3 - nbias)
        self.prior = L.addend(g, M, N) if acc else None
        self.relu = relu
        self.keep = (torch.rand(M, N, generator=g) > 0.5).to(torch.uint8) if mask else None
        self.dkeep = None if self.keep is None else self.keep.to(DEV)
        self.pl = [(a.pl, w.pl) for a, w in zip(self.A, self.W)]
        z = L.expect(self.pl, self.biases + ([self.prior] if acc else []))
        pre = torch.relu(z) if relu else z
        self.want_pre = exact32(pre)
        self.want = exact32(pre * self.keep.double() * 2.0) if mask else self.want_pre
        self.shape = (M, N, self.Ks)
        self.all_planes = set(forms) == {'p'}

    def problem(self):
        buf, out = outbuf(self.M, self.N, self.ldc, self.prior)
        pbuf = pre = None
        if self.keep is not None:
            pbuf, pre = outbuf(self.M, self.N, self.ldc)
        segs = [seg_tuple(a, w, f) for a, w, f in zip(self.A, self.W, self.forms)]
        p = ops.linear_problem(segs, out, *self.dbiases, relu=self.relu, keep_mask=self.dkeep,
                               mask_scale=2.0 if self.keep is not None else 1.0, out_pre=pre,
                               accumulate=self.prior is not None)
        return p, buf, pbuf

    def check(self, buf, pbuf, what):
        hold(buf, self.want, what)
        if pbuf is not None:
            hold(pbuf, self.want_pre, what + ' out_pre')


def launch_linear(cases, want, what, ws_floats=None, f32_split_ok=False):
    """One isc_linear_fwd launch of `cases` with a private workspace; counters, sentinels and bits.  f32_split_ok: the
    skinny modes, where h3s_plan takes the launch before plan_splitk is asked."""
    shapes = [c.shape for c in cases]
    floats = ws_floats or planes_need(shapes)
    if not f32_split_ok:
        no_f32_split(shapes, floats)
    ws_buf, ws = private_ws(floats)
    probs = [c.problem() for c in cases]
    set_ws(probs[0][0], ws)
    with ran(want):
        ops.linear_fwd([p[0] for p in probs])
        torch.cuda.synchronize()
    ws_intact(ws_buf, floats)
    for j, (c, (_, buf, pbuf)) in enumerate(zip(cases, probs)):
        c.check(buf, pbuf, '%s p%d' % (what, j))


def feat(i):
    return dict(nbias=(0, 1, 3)[i % 3], acc=i % 4 == 1, relu=i % 2 == 0, mask=i % 5 == 3, wide=i % 3 == 1)


def large_want(rows, all_planes):
    want = {TILE_KIND[rows] + (0 if all_planes else 1): 1, SPLIT: 1, 'h3': 1}
    if rows == 256:
        want['h3x'] = 1
    return want


def name(Ks, forms):
    return '+'.join('%d%s' % kf for kf in zip(Ks, forms))


def test_first_plain_case_one_chunk_64_row_tile_is_exact():
    """The supposition everything else rests on: v_mfma_f32_16x16x32_f16 accumulates small multiples of 1/4 without
    loss.  One chunk, planes, no epilogue feature, gemm_h3m_kernel<false> (kind 6)."""
    ops.set_h3_mode(2)
    x = Linear(1, 70, 130, (32,), 'p')
    launch_linear([x], large_want(64, True), 'h3m one chunk')


# 64-row tile, ring of 4: chunk counts 1 .. NBUF + 2, then two-, three- and four-segment splits of 6 (and 3) chunks with
# the switch at every ring position, planes and fp32 rows in both orders
K64 = (((32,), 'p'), ((64,), 'r'), ((96,), 'p'), ((128,), 'r'), ((160,), 'p'), ((192,), 'r'),
       ((32, 160), 'pr'), ((64, 128), 'rp'), ((96, 96), 'pr'), ((128, 64), 'rp'), ((160, 32), 'pp'), ((32, 160), 'rr'),
       ((32, 32, 128), 'prp'), ((64, 64, 64), 'rpr'), ((32, 64, 96), 'rrp'), ((96, 64, 32), 'ppr'),
       ((32, 32, 32, 32), 'prpr'), ((32, 64), 'rp'))
M64 = (1, 65, 70)
N64 = (130, 17, 127, 200)       # one past the tile / one past a 16-column block / one short / inside the second wave column


@pytest.mark.parametrize('i', range(len(K64)))
def test_h3m_64_row_tile(i):
    """gemm_h3m_kernel<false> (kind 6: every segment on planes) / <true> (kind 7: an fp32-row segment), mode 2: any launch
    of at most 256 64-row tiles."""
    ops.set_h3_mode(2)
    (Ks, forms), M, N = K64[i], M64[i % 3], N64[i % 4]
    x = Linear(100 + i, M, N, Ks, forms, **feat(i))
    launch_linear([x], large_want(64, x.all_planes), 'h3m [%d %dx%d %s]' % (i, M, N, name(Ks, forms)))


def test_the_64_row_table_covers_its_edges():
    cases = [(K64[i], M64[i % 3], N64[i % 4], feat(i)) for i in range(len(K64))]
    assert {sum(k[0]) // 32 for k, _, _, _ in cases if len(k[0]) == 1} == {1, 2, 3, 4, 5, 6}       # 1 .. NBUF + 2
    assert {k[0][0] // 32 for k, _, _, _ in cases if len(k[0]) == 2 and sum(k[0]) == 192} == {1, 2, 3, 4, 5}
    assert {k[1] for k, _, _, _ in cases} >= {'pr', 'rp', 'pp', 'rr', 'prp', 'rpr'}
    assert {(m, n) for _, m, n, _ in cases} >= {(1, 130), (65, 17), (70, 127), (70, 200)}
    for f in ('acc', 'relu', 'mask', 'wide'):
        assert sum(c[3][f] for c in cases) >= 3
    assert sum(c[3]['nbias'] == 3 for c in cases) >= 3


# 128-row tile, ring of 2, linear: 129 <= tiles < 256 with more than 256 64-row tiles.  M = 65: N = 16 390 (129 column tiles).
K128 = (((32,), 'p'), ((64,), 'r'), ((96,), 'p'), ((128,), 'r'), ((32, 64), 'pr'), ((64, 32), 'rp'), ((32, 32, 32), 'rpr'),
        ((32, 96), 'pp'))
N128 = (16390, 16384 + 17, 16384 + 127)      # 129 column tiles each: 6 live columns / one past a 16-column block / one short
M128 = (65, 65, 65, 65, 65, 65, 65, 129)


def large_case(i, Ms, Ns):
    return Ms[i], Ns[i % 3]


@pytest.mark.parametrize('i', range(len(K128)))
def test_h3_128_row_tile_linear(i):
    """gemm_h3_kernel<LINEAR, false / true> (kinds 0 / 1), mode 2.  M = 65 x N = 16 390 is 129 tiles of 128 x 128 and 258
    of 64 x 128: half_tile is false and 130 256-row tiles are fewer than 224.  N walks 16 384 + 6 / + 17 (one past a
    16-column block) / + 127 (one short of the tile): 129 column tiles each, so the route does not move.  Case 7 runs M =
    129 (one past a tile): 258 tiles, 129 of 256 rows."""
    ops.set_h3_mode(2)
    Ks, forms = K128[i]
    M, N = large_case(i, M128, N128)
    f = feat(i)
    x = Linear(200 + i, M, N, Ks, forms, nbias=f['nbias'], acc=f['acc'], relu=f['relu'], mask=i == 3)
    launch_linear([x], large_want(128, x.all_planes), 'h3 128 [%d %dx%d %s]' % (i, M, N, name(Ks, forms)))


@pytest.mark.parametrize('forms', ('pr', 'pp'))
def test_h3_128_row_tile_grouped_three_problems_sharing_a(forms):
    """Three problems of one A (65 rows) and 43 column tiles each: 129 tiles, 258 of 64 rows - one launch of the 128-row
    tile; tile_start / map_tile past problem 0."""
    ops.set_h3_mode(2)
    Ks = (64, 32)
    first = Linear(300, 65, 5462, Ks, forms, nbias=1, relu=True)
    cases = [first, Linear(301, 65, 5500, Ks, forms, nbias=3, acc=True, A=first.A),
             Linear(302, 65, 5380, Ks, forms, mask=True, A=first.A)]
    launch_linear(cases, large_want(128, forms == 'pp'), 'h3 128 grouped %s' % forms)


# 256-row tile, ring of 3: >= 224 tiles of 256 x 128.  M = 257 (one past a tile) x N = 14 338 = 2 x 113 tiles.
K256 = (((32,), 'r'), ((64,), 'p'), ((96,), 'p'), ((128,), 'r'), ((160,), 'r'), ((32, 64, 64), 'prp'), ((64, 32), 'rp'),
        ((96, 64), 'pr'))
N256 = (14338, 14336 + 17, 14336 + 127)      # 113 column tiles each: 2 live columns / one past a 16-column block / one short
M256 = (257, 257, 257, 257, 257, 257, 257, 1)
N256_M1 = 32768 + 127                        # 257 column tiles


def test_the_large_tile_tables_cover_their_column_edges():
    """Both large-tile tables run N one past a 16-column block and N one short of the tile (and a few live columns) in at
    least two cases each, on planes and on fp32 rows, without leaving their route: 129 / 113 / 257 column tiles."""
    for Ks, Ms, Ns, tiles_n in ((K128, M128, N128, 129), (K256, M256, N256, 113)):
        cases = [(large_case(i, Ms, Ns), Ks[i][1]) for i in range(len(Ks))]
        assert all((n + 127) // 128 == tiles_n for (_, n), _ in cases)
        for rem in (17, 127):
            hit = [forms for (m, n), forms in cases if n % 128 == rem and m > 1]
            assert len(hit) >= 2, (tiles_n, rem)
            assert any(set(f) == {'p'} for f in hit) and any('r' in f for f in hit), (tiles_n, rem)
        assert sum(n % 128 < 16 for (_, n), _ in cases) >= 2
    assert (N256_M1 + 127) // 128 == 257 and N256_M1 % 128 == 127
    assert {sum(k) // 32 for k, _ in K128 if len(k) == 1} == {1, 2, 3, 4}            # 1 .. NBUF + 2, ring of 2
    assert {sum(k) // 32 for k, _ in K256 if len(k) == 1} == {1, 2, 3, 4, 5}         # ring of 3


@pytest.mark.parametrize('i', range(len(K256)))
def test_h3x_256_row_tile_linear(i):
    """gemm_h3x_kernel<LINEAR, false / true> (kinds 3 / 4; isc_h3x_launches), mode 2.  Chunk counts 1 .. NBUF + 2 = 5, a
    segment switch at every ring position, both orders of planes and fp32 rows.  N walks 14 336 + 2 / + 17 (one past a
    16-column block) / + 127 (one short of the tile): 113 column tiles each.  Case 7 runs M = 1 x N = 32 768 + 127: 257
    tiles of one live row each (with fewer than 256 the half_tile rule would hand the launch to the 64-row tile)."""
    ops.set_h3_mode(2)
    Ks, forms = K256[i]
    M, N = large_case(i, M256, N256)
    if M == 1:
        N = N256_M1
    f = feat(i)
    x = Linear(400 + i, M, N, Ks, forms, nbias=f['nbias'], acc=f['acc'], relu=f['relu'], mask=i == 2)
    launch_linear([x], large_want(256, x.all_planes), 'h3x 256 [%d %dx%d %s]' % (i, M, N, name(Ks, forms)))


@functools.lru_cache(maxsize=None)
def ksliced():
    return Linear(500, 4160, 512, (800, 1280), 'pr', nbias=3, acc=True, relu=True, mask=True)


@pytest.mark.parametrize('forms', ('pr', 'pp'))
def test_h3_128_row_tile_k_sliced_and_reduce(forms):
    """isc_set_h3_ksplit(2): gemm_h3_kernel<LINEAR> writes raw partial tiles of S = 2 slices of K to slabs behind the
    planes and splitk_linear_kernel (f32 kind 6) finishes them.  4160 x 512 is 132 tiles (260 of 64 rows, 68 of 256), K =
    2080 = 65 blocks in segments of 25 + 40: S = min(512 / 132, 8) = 3 leaves 21 < 24 blocks per slice, so S = 2 with 32 /
    33 blocks - not divisible; the slice border (block 32) falls inside segment 1, the segment border inside slice 0."""
    _lib.load().isc_set_h3_ksplit(2)
    ops.set_h3_mode(2)
    x = copy.copy(ksliced())              # (one set of operands and one reference for both forms)
    x.forms, x.all_planes = forms, forms == 'pp'
    need = planes_need([x.shape])
    floats = ((need + 255) & ~255) + 2 * x.M * x.N
    launch_linear([x], {TILE_KIND[128] + (0 if forms == 'pp' else 1): 1, SPLIT: 1, 'h3': 1, 'f32_6': 1},
                  'h3 128 K-sliced %s' % forms, ws_floats=floats)


# ------------------------------------------------------------------------------------------------ 2. skinny, linear
KSK = (((32,), 'p'), ((64,), 'r'), ((96,), 'p'), ((160,), 'r'), ((288,), 'p'), ((544,), 'r'), ((32, 256), 'rp'),
       ((32, 512), 'pr'), ((32, 64), 'pr'), ((1024,), 'r'), ((32, 1056), 'pr'), ((1024,), 'p'))
MSK = (1, 33, 70)
NSK = (36, 100)


def skinny_kind(mode, Kt, forms, S=1):
    if mode == 4:
        return S64
    return S32_W8 if Kt // S >= 1024 and 'r' in forms else S32


@pytest.mark.parametrize('mode', (3, 4))
@pytest.mark.parametrize('i', range(len(KSK)))
def test_h3s_skinny_linear(i, mode):
    """gemm_h3s_kernel<LINEAR, 1, 4> (kind 9), <1, 8> (kind 10: mode 3, K >= 1024 and an fp32-row segment), <2, 4> (kind
    11: mode 4).  1, 2, 3, 5, 9, 17, 32, 34 k-blocks - fewer blocks than waves leaves waves without work, 17 wrap every
    ring; a first segment of one block, so that waves start inside the second; M = 70 x N = 100 is 3 x 4 (2 x 2) tiles:
    the grouped tile order with a column tile count that 8 does not divide."""
    ops.set_h3_mode(mode)
    (Ks, forms), M, N = KSK[i], MSK[i % 3], NSK[i % 2]
    if i in (9, 10):
        M, N = 70, 100
    x = Linear(600 + i, M, N, Ks, forms, **feat(i))
    launch_linear([x], {skinny_kind(mode, x.Kt, forms): 1, SPLIT: 1, 'h3s': 1},
                  'h3s mode %d [%d %dx%d %s]' % (mode, i, M, N, name(Ks, forms)), f32_split_ok=True)


def test_the_skinny_table_covers_its_edges():
    assert {sum(k) // 32 for k, _ in KSK} >= {1, 2, 3, 5, 9, 17}
    assert sum(k[0] == 32 and len(k) == 2 for k, _ in KSK) >= 3
    assert {skinny_kind(3, sum(k), f) for k, f in KSK} == {S32, S32_W8}
    assert {(MSK[i % 3], NSK[i % 2]) for i in range(len(KSK))} >= {(1, 36), (33, 100), (70, 36), (70, 100)}


@pytest.mark.parametrize('mode,S', [(3, 8), (3, 3), (4, 5)])
def test_h3s_skinny_k_split_over_workgroups_and_reduce(mode, S):
    """K = 4128 = 129 k-blocks (sparse lattice), 33 x 36: h3s_pick_ksplit takes the largest S <= 8 the workspace has slabs
    for - 8, 3, 5 here, of which 8 and 5 do not divide 129 - and splitk_linear_kernel (f32 kind 6) sums the slabs.  S = 3
    leaves 1376 >= 1024 per workgroup: eight waves."""
    ops.set_h3_mode(mode)
    M, N, Ks, forms = 33, 36, (32, 4096), 'pr'
    x = Linear(700 + S, M, N, Ks, forms, nbias=3, acc=True, relu=True, mask=True)
    floats = N * x.Kt + 256 + 64 + S * M * N + 8
    launch_linear([x], {skinny_kind(mode, x.Kt, forms, S): 1, SPLIT: 1, 'h3s': 1, 'f32_6': 1},
                  'h3s mode %d K-split S%d' % (mode, S), ws_floats=floats, f32_split_ok=True)


def test_h3_split_kernel_runs_once_per_weights_scope():
    """Without a scope every launch splits its weights (asserted by every case above: kind 16 + 1).  Inside
    ops.h3_weights_scope the first launch splits them into the scope's buffer and the second re-uses the planes; a
    refresh re-splits them in one launch.  The results stay exact."""
    ops.set_h3_mode(3)
    x = Linear(800, 33, 100, (32, 64), 'pr', nbias=1)
    with ops.h3_weights_scope(torch.device(DEV)):
        launch_linear([x], {S32: 1, SPLIT: 1, 'h3s': 1}, 'scope, first use', f32_split_ok=True)
        launch_linear([x], {S32: 1, 'h3s': 1}, 'scope, re-use', f32_split_ok=True)
        with ran({SPLIT: 1}):
            assert _lib.load().isc_h3_weights_refresh(ops.stream()) == 0
            torch.cuda.synchronize()
        launch_linear([x], {S32: 1, 'h3s': 1}, 'scope, after a refresh', f32_split_ok=True)


# ------------------------------------------------------------------------------------------------ 3. LSTM epilogue
W_SCALE = 0.125          # the weights' lattice scale of the LSTM cases: pre-activations of a few units, gates unsaturated


def cell64(z, c0, H):
    i, f, gg, o = z.split(H, dim=1)
    c = torch.sigmoid(f) * c0 + torch.sigmoid(i) * torch.tanh(gg)
    h = torch.sigmoid(o) * torch.tanh(c)
    return h, c, torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)], 1)


class Lstm:
    """variant: 'bias' (b_ih + b_hh only), 'pre', 'prediv' (one pre row per pre_div = 2 rows), 'tab', 'full' (pre + tab +
    keep-mask + gates_out)."""

    def __init__(self, seed, M, H, Ks, forms, variant):
        g = L.gen(seed)
        self.M, self.H, self.Ks, self.forms, self.Kt = M, H, tuple(Ks), forms, sum(Ks)
        self.A = [Opd(g, M, K, self.Kt) for K in Ks]
        self.W = [Opd(g, 4 * H, K, self.Kt, scale=W_SCALE) for K in Ks]
        self.b_ih, self.b_hh, self.c0 = L.addend(g, 4 * H), L.addend(g, 4 * H), L.addend(g, M, H)
        self.pre_div = 2 if variant == 'prediv' else 1
        assert M % self.pre_div == 0
        self.pre = L.addend(g, M // self.pre_div, 4 * H) if variant in ('pre', 'prediv', 'full') else None
        self.tab = L.addend(g, 50, 4 * H) if variant in ('tab', 'full') else None
        self.ids = torch.randint(0, 50, (M,), generator=g) if self.tab is not None else None
        self.full = variant == 'full'
        self.keep = (torch.rand(M, H, generator=g) > 0.5).to(torch.uint8) if self.full else None
        addends = [self.b_ih, self.b_hh]
        if self.pre is not None:
            addends.append(self.pre.repeat_interleave(self.pre_div, dim=0))
        if self.tab is not None:
            addends.append(self.tab[self.ids])
        self.z = L.expect([(a.pl, w.pl) for a, w in zip(self.A, self.W)], addends)
        exact32(self.z)
        self.ref = cell64(self.z, self.c0.double(), H)
        self.dev = [None if v is None else v.to(DEV) for v in (self.b_ih, self.b_hh, self.c0, self.pre, self.tab, self.ids,
                                                                self.keep)]
        self.shape = (M, 4 * H, self.Ks)
        self.all_planes = set(forms) == {'p'}

    def run(self, ws, want, what):
        """One launch; h, c (and gates) against the fp64 cell on the exact pre-activations at 2e-5, sentinels, hdrop and
        planes exact.  Returns (h, c, gates or None) on the host."""
        M, H = self.M, self.H
        hb, cb = torch.full((M + 1, H), SENT, device=DEV), torch.full((M + 1, H), SENT, device=DEV)
        gb = torch.full((M + 1, 4 * H), SENT, device=DEV) if self.full else None
        db = torch.full((M + 1, H), SENT, device=DEV) if self.full else None
        hp = torch.full((2, M, H), float('nan'), dtype=torch.float16, device=DEV)
        b_ih, b_hh, c0, pre, tab, ids, keep = self.dev
        segs = [seg_tuple(a, w, f) for a, w, f in zip(self.A, self.W, self.forms)]
        with ran(want):
            ops.lstm_fwd(segs, b_ih, b_hh, c0, hb[:M], cb[:M], gates_out=None if gb is None else gb[:M], h_keep_mask=keep,
                         mask_scale=2.0, hdrop_out=None if db is None else db[:M], pre=pre, tab=tab, tab_ids=ids,
                         h_planes=hp, pre_div=self.pre_div, ws=ws)
            torch.cuda.synchronize()
        outs = []
        for buf, ref, nm in ((hb, self.ref[0], 'h'), (cb, self.ref[1], 'c'), (gb, self.ref[2], 'gates')):
            if buf is None:
                outs.append(None)
                continue
            got = buf.cpu()
            assert bool((got[M:] == SENT).all()), '%s %s: the row past M lost its sentinel' % (what, nm)
            assert bool(torch.isfinite(got[:M]).all()), (what, nm)
            np.testing.assert_allclose(got[:M].numpy(), ref.float().numpy(), atol=2e-5, rtol=0, err_msg='%s %s' % (what, nm))
            outs.append(got[:M])
        if self.full:
            assert torch.equal(db[:M], hb[:M] * keep.float() * 2.0) and bool((db[M:] == SENT).all()), what
        assert bool(torch.isfinite(hp.float()).all()), what + ': an h_planes element was not written'
        assert torch.equal(hp, _planes(hb[:M])), what + ': planes != a re-split of h'
        return outs

    def run_mode0(self, what):
        """The same launch on the exact-fp32 engine: mode 0, tile override 0, a 1-float workspace - gemm_kernel on the
        128-row tile (f32 kind 0), which test_gpu_gemm_f32_kernels.py holds to fp64."""
        mode = ops.set_h3_mode(0)
        ops.set_tile_override(0)
        off_buf, off = private_ws(1)
        try:
            return self.run(off, {'f32_0': 1}, what + ' mode 0')
        finally:
            ws_intact(off_buf, 1)
            ops.set_tile_override(-1)
            ops.set_h3_mode(mode)


def ulps(a, b):
    """The largest distance of two fp32 tensors in units in the last place (0 = equal in bits up to the sign of zero)."""
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return int((key(a) - key(b)).abs().max())


SMALL_Z = 2.0 ** -5


def lstm_both(x, mode, want, what, ulp_bar=0):
    """The launch in `mode` and in mode 0, compared in ulps (printed before it is asserted): h, c and the gates agree in
    bits (ulp_bar = 0) wherever the exact-fp32 engine's pre-activation is the lattice value too - see
    test_h3x_256_row_tile_lstm for where it is not.  ulp_bar > 0 applies ONLY to outputs with an expected
    pre-activation below SMALL_Z (a gate value: its own; h and c: any of the unit's four gates); everything else in the
    launch is still held to bit equality."""
    ops.set_h3_mode(mode)
    floats = planes_need([x.shape])
    if mode == 2:                         # (modes 3 / 4: h3s_plan takes the launch before plan_splitk is asked)
        no_f32_split([x.shape], floats)
    ws_buf, ws = private_ws(floats)
    got = x.run(ws, want, what)
    ws_intact(ws_buf, floats)
    base = x.run_mode0(what)
    dist = {nm: ulps(a, b) for a, b, nm in zip(got, base, ('h', 'c', 'gates')) if a is not None}
    print('H3 vs mode 0 %-50s ulps %r  differing %r' % (what, dist, {
        nm: int((a != b).sum()) for a, b, nm in zip(got, base, ('h', 'c', 'gates')) if a is not None}))
    assert max(dist.values()) <= ulp_bar, '%s: differs from the exact-fp32 engine by %r ulps, bar %d' % (what, dist, ulp_bar)
    if ulp_bar:
        big = x.z.abs() >= SMALL_Z                                          # [M, 4H]: this gate's residue cannot survive
        unit_big = big.view(x.M, 4, x.H).all(1)                             # [M, H]: none of the unit's gates is small
        for a, b, nm in zip(got, base, ('h', 'c', 'gates')):
            if a is not None:
                keep = big if nm == 'gates' else unit_big
                bad = (a != b) & keep
                assert not bool(bad.any()), '%s: %d %s values differ in bits where every pre-activation is >= 2^-5' % (
                    what, int(bad.sum()), nm)
        print('H3 vs mode 0 %-50s outputs under the ulp bar: %d of %d' % (what, int((~unit_big).sum()), unit_big.numel()))


LSTM_LARGE = [(130, 64, (64, 32), 'pr', 'bias'), (130, 64, (32, 64, 32), 'rpr', 'pre'), (130, 64, (96,), 'p', 'prediv'),
              (130, 64, (32, 32), 'pp', 'tab'), (129, 32, (64, 64, 32), 'prp', 'full'), (1, 64, (32,), 'r', 'full'),
              (130, 64, (32, 96), 'rp', 'full')]


@pytest.mark.parametrize('M,H,Ks,forms,variant', LSTM_LARGE)
def test_h3_128_row_tile_lstm(M, H, Ks, forms, variant):
    """gemm_h3_kernel<LSTM, false / true> (kinds 0 / 1), mode 2: 1-4 chunks on the ring of 2, segment switches, bias-only,
    pre, pre_div = 2, tab, and everything with keep-mask and gates_out; M = 1, one past a tile, two past."""
    x = Lstm(900 + M + H + len(Ks), M, H, Ks, forms, variant)
    lstm_both(x, 2, large_want(128, x.all_planes), 'h3 128 lstm [%dx%d %s %s]' % (M, H, name(Ks, forms), variant))


@pytest.mark.parametrize('forms,variant,ulp_bar', [('pr', 'bias', 30), ('pp', 'full', 0), ('rp', 'prediv', 0)])
def test_h3x_256_row_tile_lstm(forms, variant, ulp_bar):
    """gemm_h3x_kernel<LSTM, false / true> (kinds 3 / 4), mode 2: M = 3330 x H = 512 is 14 x 16 = 224 tiles of 256 x 128.

    Against mode 0, measured on an MI355X: every LSTM case of this file agrees with the exact-fp32 engine in bits, except
    the bias-only one here, where 3 of 1 704 960 h values and 8 c values differ, by at most 14 and 15 ulps (bar: 2 x 15,
    and only for units with a gate pre-activation below 2^-5; every other output of the launch is held to bit equality).
    The cause is not the cell and not the split-f16 kernel: its pre-activation IS the lattice value (h, c and the gates
    are held to the fp64 cell on it).  The exact-fp32 engine contracts x_a x_b whole, including the lo_a lo_b 2^-22 term
    the split-f16 definition drops (here up to 2^-29 per k); while a gate's running sum AND its sum with the bias stay
    below about 2^-5 that residue is more than half an ulp and survives, so mode 0's pre-activation is off the lattice
    by ~1e-8.  All 9 gate values that differ (7 of gate g, 2 of gate f) sit at |pre-activation| <= 0.025; there
    isc_tanh's 1 - 2 / (1 + exp(2 x)) turns a last-bit change of exp(2 x) into a step of 2^-23 = 1.2e-7 absolute - 20 ulps
    of a tanh of 0.006 - and both engines' values lie within 6e-8 of the fp64 cell.  With `pre` or `tab` the chain of
    sums would have to stay below 2^-5 at every link, which no element of the other cases does."""
    M, H, Ks = 3330, 512, (32, 64)
    x = Lstm(950, M, H, Ks, forms, variant)
    lstm_both(x, 2, large_want(256, x.all_planes), 'h3x 256 lstm [%dx%d %s %s]' % (M, H, name(Ks, forms), variant), ulp_bar)


LSTM_SKINNY = [(33, 32, (32,), 'p', 'bias'), (70, 64, (32, 64), 'pr', 'full'), (34, 32, (96,), 'r', 'prediv'),
               (1, 64, (32, 32, 32), 'rpr', 'tab'), (70, 32, (160,), 'p', 'pre'), (33, 64, (1024,), 'r', 'full'),
               (70, 64, (32, 512), 'pr', 'full')]


@pytest.mark.parametrize('mode', (3, 4))
@pytest.mark.parametrize('M,H,Ks,forms,variant', LSTM_SKINNY)
def test_h3s_skinny_lstm(M, H, Ks, forms, variant, mode):
    """gemm_h3s_kernel<LSTM, 1, 4> (kind 9), <1, 8> (kind 10: K = 1024 on fp32 rows), <2, 4> (kind 11), modes 3 / 4; 1 ...
    32 k-blocks, a first segment of one block, M = 70 in 3 (2) row tiles."""
    x = Lstm(1000 + M + H + sum(Ks), M, H, Ks, forms, variant)
    lstm_both(x, mode, {skinny_kind(mode, x.Kt, forms): 1, SPLIT: 1, 'h3s': 1},
              'h3s mode %d lstm [%dx%d %s %s]' % (mode, M, H, name(Ks, forms), variant))


# ------------------------------------------------------------------------------------------------ 4. vocabulary epilogue
class Vocab:
    """h [M, K] x W [V, K] + bias on lattice operands; W rows (and bias) 64 .. 95 of every 128-column tile repeat rows 0 ..
    31, so tile maxima are tied in many (row, tile) pairs: part_idx must be the lowest column among them."""

    def __init__(self, seed, M, V, K):
        g = L.gen(seed)
        self.M, self.V, self.K, self.nt = M, V, K, (V + 127) // 128
        self.h = Opd(g, M, K, K)
        self.W = Opd(g, V, K, K, scale=0.25, tie_rows=True)
        self.bias = L.addend(g, V)
        for t0 in range(0, V, 128):
            n = min(32, V - (t0 + 64))
            if n > 0:
                self.bias[t0 + 64:t0 + 64 + n] = self.bias[t0:t0 + n]
        self.dbias = self.bias.to(DEV)
        z = L.expect([(self.h.pl, self.W.pl)], [self.bias])
        self.logits = exact32(z)
        tiles = torch.nn.functional.pad(z, (0, self.nt * 128 - V), value=float('-inf')).view(M, self.nt, 128)
        self.pmax64 = tiles.max(2).values
        is_max = tiles == self.pmax64[:, :, None]
        col = torch.arange(self.nt * 128).view(1, self.nt, 128).expand(M, -1, -1)
        self.pidx = torch.where(is_max, col, torch.full_like(col, 1 << 30)).min(2).values.to(torch.int32)
        self.tied = int((is_max.sum(2) > 1).sum())
        assert self.tied >= 1, 'no (row, tile) pair with tied maxima: the lowest-column rule would go untested'
        self.lse = torch.logsumexp(z, 1)
        self.shape = (M, V, (K,))

    def run(self, want, what, planes, logits_pad=None):
        M, V, nt = self.M, self.V, self.nt
        floats = planes_need([self.shape])
        no_f32_split([self.shape], floats)
        ws_buf, ws = private_ws(floats)
        pm, ps = torch.full((M + 1, nt), SENT, device=DEV), torch.full((M + 1, nt), SENT, device=DEV)
        pi = torch.full((M + 1, nt), ISENT, device=DEV, dtype=torch.int32)
        lb = lg = None
        if logits_pad is not None:
            lb, lg = outbuf(M, V, V + logits_pad)
        with ran(want):
            ops.vocab_fwd(self.h.d, self.W.d, self.dbias, pm[:M], ps[:M], pi[:M], lg,
                          h_planes=self.h.planes if planes else None, ws=ws)
            torch.cuda.synchronize()
        ws_intact(ws_buf, floats)
        if lb is not None:
            hold(lb, self.logits, what + ' logits')
        hold(pm, exact32(self.pmax64), what + ' part_max')
        hold(pi, self.pidx, what + ' part_idx')
        sums = ps.cpu()
        assert bool((sums[M:] == SENT).all()) and bool(torch.isfinite(sums[:M]).all()), what
        lse = self.pmax64.max(1).values + torch.log((sums[:M].double() * torch.exp(self.pmax64 - self.pmax64.max(1).values[:, None])).sum(1))
        np.testing.assert_allclose(lse.float().numpy(), self.lse.float().numpy(), atol=3e-5, rtol=1e-5, err_msg=what)
        tile_lse = torch.log(sums[:M].double()) + self.pmax64
        z = torch.nn.functional.pad(self.logits.double(), (0, nt * 128 - V), value=float('-inf')).view(M, nt, 128)
        np.testing.assert_allclose(tile_lse.float().numpy(), torch.logsumexp(z, 2).float().numpy(), atol=3e-5, rtol=1e-5,
                                   err_msg=what + ' per tile')


def vocab_all(x, want, what, planes):
    x.run(want, what, planes, logits_pad=0)
    x.run(want, what + ' ld+6', planes, logits_pad=6)
    x.run(want, what + ' no logits', planes)


@pytest.mark.parametrize('M,V,K,planes', [(70, 130, 64, True), (70, 1000, 64, False), (129, 130, 96, False),
                                          (1, 1000, 128, True)])
def test_h3_128_row_tile_vocab(M, V, K, planes):
    """gemm_h3_kernel<VOCAB, false / true> (kinds 0 / 1), mode 2 (the vocabulary projection never takes the 256-row tile),
    with logits (ld = V, V + 6) and without."""
    ops.set_h3_mode(2)
    x = Vocab(1100 + M + V, M, V, K)
    vocab_all(x, large_want(128, planes), 'h3 128 vocab [%dx%dx%d]' % (M, V, K), planes)


@pytest.mark.parametrize('M,V,K,planes,kind', [(33, 130, 64, True, SV_W8), (33, 130, 160, False, SV_W8),
                                               (33, 130, 224, True, SV_W8),
                                               (300, 4100, 64, False, SV), (300, 4100, 64, True, SV),
                                               (300, 4100, 160, True, SV), (300, 4100, 224, False, SV)])
def test_h3s_skinny_vocab_ring_form(M, V, K, planes, kind):
    """gemm_h3s_kernel<VOCAB, 1, 8> (kind 13: up to 256 workgroups; waves w and w + 4 halve K) and <VOCAB, 1, 4> (kind
    12: 10 x 33 = 330 workgroups), mode 3 with ops.set_h3v(0).  Both forms stage through rings of 2: K = 64 fills the
    four-wave ring once, K = 160 / 224 (5 / 7 k-blocks) re-issue its slots; the eight-wave halves see 1, 2-3, 3-4 blocks."""
    ops.set_h3_mode(3)
    ops.set_h3v(0)
    x = Vocab(1200 + M + V + K, M, V, K)
    vocab_all(x, {kind: 1, SPLIT: 1, 'h3s': 1}, 'h3s vocab [%dx%dx%d]' % (M, V, K), planes)


@pytest.mark.parametrize('planes', (True, False))
@pytest.mark.parametrize('K', (32, 64, 96, 128, 224))
def test_h3v_vocab_shared_stages(K, planes):
    """gemm_h3v_kernel<false> (kind 14: h_planes given) / <true> (kind 15), mode 3: 1, 2, 3, 4, 7 k-blocks on 3 stages."""
    ops.set_h3_mode(3)
    M, V = (33, 130) if K != 128 else (70, 1000)
    x = Vocab(1300 + K, M, V, K)
    vocab_all(x, {V_PLANES if planes else V_F32: 1, SPLIT: 1, 'h3s': 1}, 'h3v [%dx%dx%d]' % (M, V, K), planes)


# ------------------------------------------------------------------------------------------------ 5. backward NN / TN
class Bwd:
    """One backward problem on lattice operands.  NN: A_s [M, K_s], W_s stored [K_s, N] as a column slice of a wider
    matrix; TN: A_s stored [K_s, M], W_s stored [K_s, N], both column slices; out a column slice."""

    def __init__(self, seed, layout, M, N, Ks, acc=False, bias=False, A=None, W=None):
        g = L.gen(seed)
        self.layout, self.M, self.N, self.Ks, self.Kt = layout, M, N, tuple(Ks), sum(Ks)
        self.A = A or [Opd(g, M, K, self.Kt) for K in Ks]
        self.W = W or [Opd(g, N, K, self.Kt) for K in Ks]
        self.keepalive, self.dsegs = [], []
        for a, w in zip(self.A, self.W):
            wt = torch.full((w.x.shape[1], N + 8), float('nan'))
            wt[:, 4:4 + N] = w.x.t()
            dwt = wt.to(DEV)
            if layout == ops.NN:
                da = a.d
            else:
                if not hasattr(a, 'dt'):
                    at = torch.full((a.x.shape[1], M + 8), float('nan'))
                    at[:, 4:4 + M] = a.x.t()
                    a.dt_whole = at.to(DEV)
                    a.dt = a.dt_whole[:, 4:4 + M]
                da = a.dt
            self.keepalive.append(dwt)
            self.dsegs.append((da, dwt[:, 4:4 + N]))
        self.prior = L.addend(g, M, N) if acc else None
        self.bias = L.addend(g, N) if bias else None
        self.dbias = None if self.bias is None else self.bias.to(DEV)
        addends = ([self.bias] if bias else []) + ([self.prior] if acc else [])
        self.want = exact32(L.expect([(a.pl, w.pl) for a, w in zip(self.A, self.W)], addends))
        self.shape = (M, N, self.Ks)

    def problem(self):
        buf = torch.full((self.M + 1, self.N + 12), SENT, device=DEV)
        out = buf[:self.M, 4:4 + self.N]
        if self.prior is not None:
            out.copy_(self.prior)
        return ops.gemm_problem(self.dsegs, out, self.layout, accumulate=self.prior is not None, bias0=self.dbias), buf

    def check(self, buf, what):
        got = buf.cpu()
        assert bool((got[:, :4] == SENT).all()), what + ': a column before the slice lost its sentinel'
        hold(buf[:, 4:], self.want, what)


def launch_bwd(cases, layout, want, what, floats):
    ws_buf, ws = private_ws(floats)
    probs = [c.problem() for c in cases]
    set_ws(probs[0][0], ws)
    with ran(want):
        ops.gemm_bwd([p[0] for p in probs], layout)
        torch.cuda.synchronize()
    ws_intact(ws_buf, floats)
    for j, (c, (_, buf)) in enumerate(zip(cases, probs)):
        c.check(buf, '%s p%d' % (what, j))


NN_CASES = [(3, 1, 36, (32,)), (3, 33, 100, (64, 32)), (3, 70, 100, (32, 256)), (3, 70, 36, (1024,)),
            (4, 33, 36, (96,)), (4, 70, 100, (32, 512)), (4, 1, 100, (160,)),
            (2, 70, 132, (32,)), (2, 65, 260, (64, 128)), (2, 1, 132, (32, 64, 32)), (2, 70, 20, (192,))]


@pytest.mark.parametrize('mode,M,N,Ks', NN_CASES)
def test_nn_layout_on_the_skinny_and_the_64_row_kernels(mode, M, N, Ks):
    """ops.gemm_bwd(..., NN): dX = dY W over planes of W^T from the TRANSPOSING h3_split_kernel (kind 16), dY read as
    fp32 rows.  Modes 3 / 4: gemm_h3s_kernel 32 x 32 (kind 9; kind 10 at K = 1024) / 64 x 64 (kind 11); mode 2:
    gemm_h3m_kernel<true> (kind 7).  Accumulate, bias0, W and out column slices."""
    ops.set_h3_mode(mode)
    x = Bwd(1400 + M + N + sum(Ks), ops.NN, M, N, Ks, acc=M != 33, bias=N != 36)
    want = ({skinny_kind(mode, x.Kt, 'r'): 1, SPLIT: 1, 'h3s': 1} if mode != 2 else large_want(64, False))
    launch_bwd([x], ops.NN, want, 'NN mode %d [%dx%d K%s]' % (mode, M, N, '+'.join(map(str, Ks))), planes_need([x.shape]))


def test_nn_layout_k_sliced_on_the_128_row_tile():
    """The NN layout slices K on its own (isc_set_h3_ksplit left at 1): dX [4160, 512] over K = 800 + 1280 in mode 2 is
    the launch of test_h3_128_row_tile_k_sliced_and_reduce read k-major - gemm_h3_kernel<LINEAR, true> (kind 1) writes S =
    2 slabs over planes of W^T from the transposing split, splitk_linear_kernel adds bias0 and the prior once."""
    ops.set_h3_mode(2)
    lin = ksliced()
    x = Bwd(1450, ops.NN, lin.M, lin.N, lin.Ks, acc=True, bias=True, A=lin.A, W=lin.W)
    need = planes_need([x.shape])
    launch_bwd([x], ops.NN, {TILE_KIND[128] + 1: 1, SPLIT: 1, 'h3': 1, 'f32_6': 1}, 'NN K-sliced',
               ((need + 255) & ~255) + 2 * x.M * x.N)


TN_CASES = [(1664, 1664, (64,), 0), (1664, 1660, (32, 64), 0), (1152, 1152, (96,), 6), (1152, 1156, (64, 96), 6),
            (256, 256, (64,), S32), (256, 260, (160,), S32), (4, 256, (32, 32, 32), S32)]


@pytest.mark.parametrize('M,N,Ks,kind', TN_CASES)
def test_tn_layout_large_64_row_and_skinny_tile(M, N, Ks, kind):
    """ops.gemm_bwd(..., TN) in mode 2 (no flop floor): planes of both transposes by one transposing split launch (kind
    16), then by tile count gemm_h3_kernel<LINEAR, false> (kind 0: >= 160 tiles), gemm_h3m_kernel<false> (kind 6: >= 80)
    or gemm_h3s_kernel<LINEAR, 1, 4> (kind 9); every form counts in isc_h3_launches.  K-segments, accumulate, bias0."""
    ops.set_h3_mode(2)
    x = Bwd(1500 + M + N + sum(Ks), ops.TN, M, N, Ks, acc=len(Ks) != 2, bias=M != 256)
    launch_bwd([x], ops.TN, {kind: 1, SPLIT: 1, 'h3': 1}, 'TN [%dx%d K%s]' % (M, N, '+'.join(map(str, Ks))),
               (M + N) * x.Kt + 1024)


def test_tn_one_segment_in_k_chunks_accumulates_in_fp32():
    """K = 1024 rows, M = N = 256 with a workspace of 512 * 512 + 1024 floats: two chunks of 512 rows, two launches of the
    skinny tile; chunk 2 accumulates onto chunk 1, which accumulates onto the prior; the bias goes in once.  Still exact."""
    ops.set_h3_mode(2)
    x = Bwd(1600, ops.TN, 256, 256, (1024,), acc=True, bias=True)
    launch_bwd([x], ops.TN, {S32: 2, SPLIT: 2, 'h3': 2}, 'TN K chunks', 512 * 512 + 1024)


def test_tn_grouped_three_problems_sharing_dy():
    """Three dW contractions from one dY [2048, 128] (sparse lattice), N = 64 / 64 / 32: one transposing split, one skinny
    launch (kc_max = 2048 fits the workspace in one chunk)."""
    ops.set_h3_mode(2)
    first = Bwd(1700, ops.TN, 128, 64, (2048,), acc=True)
    cases = [first, Bwd(1701, ops.TN, 128, 64, (2048,), bias=True, A=first.A), Bwd(1702, ops.TN, 128, 32, (2048,), A=first.A)]
    launch_bwd(cases, ops.TN, {S32: 1, SPLIT: 1, 'h3': 1}, 'TN grouped', (128 + 160) * 2048 + 4096)
