"""The exact-fp32 GEMM kernels of csrc/gemm_f32.hip, one by one: every case names the kernel it means to run, proves
with the launch counters (ops.f32_launches) that this kernel and no other ran, and holds the result to fp64.

Routes.  A tile override reaches pick_tile only when plan_splitk has not taken the launch first, and plan_splitk does
not look at the override - so every per-tile case hands the launch a private split-K workspace too small to split
(declared 1 float); the split-K cases hand it one of exactly S * sum(M * N) floats, which fixes the split count at S
where the plan's other caps (768 / blocks, 16, chunks / 4) are at least S.  Every private workspace is followed by
sentinel floats that must survive.

Bars: the project's - forward and NN atol 3e-5 + rtol 1e-5, TN atol 2e-4 max(1, sqrt(rows) / 8) + rtol 1e-5, LSTM h / c
/ gates 2e-5 - with operands uniform in [-1, 1], weights scaled by K ** -0.5 (TN: randn, as test_gemm_tn_vs_fp64).  All
tiles accumulate an output element over k in the same order, so the tiles of one layout agree bit for bit; a split-K
launch equals, bit for bit, S split-off 32-row launches over its K sub-ranges summed in slab order in fp32 with the
epilogue applied in epi_linear_finish's order.  Outputs sit in sentinel-filled buffers with ldc > N and one extra row.

err_kernel / max(err32, 2^-23 max|ref|) (tests/_bwd_ref.py: err32 is the same formula in fp32 torch on the CPU) is
recorded per kernel and printed by the file's last test under `pytest -s`; it is not asserted on (the CPU's blocked
summation is not the kernel's order).  The docstrings give what an MI355X measured."""
import ctypes as C

import numpy as np
import pytest
import torch

import _bwd_ref as R
from _split_f16 import planes as _planes
from insenticap_model_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = R.SENTINEL
ISENT = 123456789
F32, F64 = torch.float32, torch.float64
WORST = {}               # kernel -> (ratio, err_kernel, err32, case)
NT_KIND = {0: 0, 1: 5, 2: 2, 3: 3, 4: 4}        # override -> kind, plain linear NT launches (tile 1 = MD)


@pytest.fixture(autouse=True)
def _restore_routing():
    mode, rows = ops.h3_mode(), ops.set_gemv_rows(8)
    ops.set_gemv_rows(rows)
    yield
    ops.set_tile_override(-1)
    ops.set_tile_override(103)
    ops.set_h3_mode(mode)
    ops.set_gemv_rows(rows)


# ------------------------------------------------------------------------------------------------ helpers
def gen(seed):
    return torch.Generator().manual_seed(seed)


def uni(g, *shape, scale=1.0):
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def d(x):
    return None if x is None else x.to(DEV)


def counters():
    lib = _lib.load()
    return tuple(ops.f32_launches(k) for k in range(7)) + (lib.isc_h3_launches(), lib.isc_h3s_launches(),
                                                           lib.isc_gemv_launches())


class ran:
    """`with ran({kind: n, ...}):` - exactly these fp32 kinds went up, by exactly n; the split-f16 and matrix-vector
    counters did not move."""

    def __init__(self, want):
        self.want = want

    def __enter__(self):
        self.before = counters()
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            delta = tuple(a - b for a, b in zip(counters(), self.before))
            want = tuple(self.want.get(k, 0) for k in range(7)) + (0, 0, 0)
            assert delta == want, 'launch counters (kinds 0-6, h3, h3s, gemv) moved by %r, expected %r' % (delta, want)
        return False


def private_ws(floats):
    """(whole buffer, the declared workspace): `floats` floats followed by 64 sentinels."""
    buf = torch.full((floats + 64,), SENT, device=DEV)
    return buf, buf[:floats]


def ws_intact(buf, floats):
    assert bool((buf[floats:] == SENT).all()), 'the launch wrote past its declared split-K workspace'


def set_ws(problem, ws):
    problem.splitk_ws, problem.splitk_ws_floats = ws.data_ptr(), ws.numel()


def outbuf(M, N, ldc, prior=None):
    """(whole [M + 1, ldc] sentinel buffer, its owned [M, N] view)"""
    buf = torch.full((M + 1, ldc), SENT, device=DEV)
    if prior is not None:
        buf[:M, :N] = prior.to(DEV)
    return buf, buf[:M, :N]


def hold(got_buf, ref, ev32, kernel, case, atol, rtol=1e-5):
    """got_buf [M + extra, ld] against ref [M, N] (fp64) at the named bar; everything outside [M, N] keeps the sentinel.
    Records err_kernel / max(err32, 2^-23 max|ref|) under `kernel`."""
    got = got_buf.detach().cpu()
    sent = ISENT if got.dtype == torch.int32 else SENT
    M, N = ref.shape
    live = got[:M, :N]
    assert bool((got[M:] == sent).all()), '%s %s: a row past M lost its sentinel' % (kernel, case)
    assert bool((got[:M, N:] == sent).all()), '%s %s: a column past N lost its sentinel' % (kernel, case)
    assert bool(torch.isfinite(live).all()), (kernel, case)
    rule, err32 = R.bound(ref, ev32)
    err = float((live.to(F64) - ref).abs().max())
    ratio = err / (rule / R.FACTOR) if rule > 0 else (0.0 if err == 0 else float('inf'))      # (an all-zero reference)
    print('F32REF %-22s %-44s err_kernel %.3e  err32 %.3e  ratio %.2f' % (kernel, case, err, err32, ratio))
    if kernel not in WORST or ratio > WORST[kernel][0]:
        WORST[kernel] = (ratio, err, err32, case)
    np.testing.assert_allclose(live.numpy(), ref.to(F32).numpy(), atol=atol, rtol=rtol, err_msg='%s %s' % (kernel, case))
    return live


def chunk_slices(Ks, c0, c1):
    """The K sub-ranges [(segment, k0, k1)] of chunks [c0, c1) of a problem's chunk sequence (32-deep, per segment)."""
    out, base = [], 0
    for s, K in enumerate(Ks):
        n = (K + 31) // 32
        lo, hi = max(c0 - base, 0), min(c1 - base, n)
        if lo < hi:
            out.append((s, lo * 32, min(hi * 32, K)))
        base += n
    return out


def n_chunks(Ks):
    return sum((K + 31) // 32 for K in Ks)


def split_caps(blocks, chunks):
    return min(768 // blocks, 16, chunks // 4)


def slab_sum(parts):
    """The reduce kernels' sum: slab 0, then + slab 1, + slab 2 ... in fp32."""
    v = parts[0].clone()
    for p in parts[1:]:
        v = v + p
    return v


# ------------------------------------------------------------------------------------------------ 1. forward linear
def linear_ref(dt, segs, biases, prior, relu, keep, scale):
    z = sum(a.to(dt) @ w.to(dt).t() for a, w in segs)
    for b in biases:
        z = z + b.to(dt)
    if prior is not None:
        z = z + prior.to(dt)
    pre = torch.relu(z) if relu else z
    out = pre if keep is None else pre * keep.to(dt) * scale
    return {'out': out, 'pre': pre}


MS = (1, 33, 65, 129, 257, 300)
NS = ((1, None), (4, None), (124, None), (128, None), (130, 130), (130, 132), (132, None), (260, None))
KS = ((32,), (64,), (96,), (160,), (224,), (256,), (288,), (32, 32, 32), (64, 32, 96, 32))


def linear_case(i):
    M, (N, ldc), Ks = MS[i % 6], NS[i % 8], KS[i % 9]
    feat = dict(nbias=(0, 1, 3)[i % 3], acc=i % 4 == 1, relu=i % 2 == 0, mask=i % 5 == 3 and ldc is None, wide=i % 3 == 1)
    if ldc is None:
        ldc = N if feat['mask'] else (N + 3) // 4 * 4 + 4       # the keep-mask is read with ld = N: ldc == N is required
    return M, N, ldc, Ks, feat


class LinearData:
    """One problem's operands on both sides, its fp64 / fp32 references, and the problem struct for a fresh output."""

    def __init__(self, seed, M, N, ldc, Ks, nbias=0, acc=False, relu=False, mask=False, wide=False):
        g = gen(seed)
        self.M, self.N, self.ldc, self.Ks = M, N, ldc, Ks
        Kt = sum(Ks)
        self.segs, self.dsegs, self.keepalive = [], [], []
        for K in Ks:
            pad = 8 if wide else 0
            a, w = uni(g, M, K + pad), uni(g, N, K + 2 * pad, scale=Kt ** -0.5)
            da, dw = a.to(DEV), w.to(DEV)
            self.keepalive += [da, dw]
            self.segs.append((a[:, pad:], w[:, pad:pad + K]) if wide else (a, w))          # lda, ldw > K
            self.dsegs.append((da[:, pad:], dw[:, pad:pad + K]) if wide else (da, dw))
        self.biases = [uni(g, N) for _ in range(nbias)]
        self.dbiases = [b.to(DEV) for b in self.biases] + [None] * (3 - nbias)
        self.prior = uni(g, M, N) if acc else None
        self.relu = relu
        self.keep = (torch.rand(M, N, generator=g) > 0.5).to(torch.uint8) if mask else None
        self.dkeep = d(self.keep)
        self.scale = 2.0 if mask else 1.0
        self.ref, self.ev = R.both(linear_ref, self.segs, self.biases, self.prior, relu, self.keep, self.scale)

    def problem(self, segs=None, plain=False):
        """(problem, out buffer, pre buffer or None); plain: the bare contraction of `segs`, no epilogue feature."""
        buf, out = outbuf(self.M, self.N, self.ldc, None if plain else self.prior)
        pbuf = pre = None
        if self.keep is not None and not plain:
            pbuf, pre = outbuf(self.M, self.N, self.ldc)
        if plain:
            p = ops.linear_problem(segs, out)
        else:
            p = ops.linear_problem(segs or self.dsegs, out, *self.dbiases, relu=self.relu, keep_mask=self.dkeep,
                                   mask_scale=self.scale, out_pre=pre, accumulate=self.prior is not None)
        return p, buf, pbuf

    def check(self, buf, pbuf, kernel, case):
        hold(buf, self.ref['out'], self.ev['out'], kernel, case, atol=3e-5)
        if pbuf is not None:
            hold(pbuf, self.ref['pre'], self.ev['pre'], kernel, case + ' pre', atol=3e-5)


LIN_KERNEL = {0: 'gemm_kernel<L,NT,lin>', 1: 'gemm_md_kernel', 2: 'gemm_kernel<S,NT,lin>', 3: 'gemm_xl_kernel<lin>',
              4: 'gemm_ld_kernel<lin>', 'm': 'gemm_kernel<M,NT,lin>'}


def run_linear_all_tiles(datas, case):
    """The launch of `datas` (1-3 problems) under overrides 0-4 and under override 1 with the MD path off; returns after
    asserting kernels, fp64 bars, sentinels and bit equality across the six."""
    off_buf, off = private_ws(1)
    base = None
    for t in (0, 1, 2, 3, 4, 'm'):
        ops.set_tile_override(1 if t == 'm' else t)
        if t == 'm':
            ops.set_tile_override(102)
        probs = [x.problem() for x in datas]
        set_ws(probs[0][0], off)
        with ran({1 if t == 'm' else NT_KIND[t]: 1}):
            ops.linear_fwd([p[0] for p in probs])
            torch.cuda.synchronize()
        if t == 'm':
            ops.set_tile_override(103)
        for x, (_, buf, pbuf) in zip(datas, probs):
            x.check(buf, pbuf, LIN_KERNEL[t], case)
        cur = [b.cpu() for p in probs for b in p[1:] if b is not None]
        if base is None:
            base = cur
        else:
            assert all(torch.equal(a, b) for a, b in zip(base, cur)), '%s: tile %s differs from tile 0 in bits' % (case, t)
    ws_intact(off_buf, 1)


def test_linear_case_table_covers_the_issue_values():
    cases = [linear_case(i) for i in range(30)]
    assert {c[0] for c in cases} == set(MS) and {(c[1], c[2]) for c in cases} >= {(130, 130), (130, 132)}
    assert {c[1] for c in cases} == {1, 4, 124, 128, 130, 132, 260} and {c[3] for c in cases} == set(KS)
    assert {n_chunks(k) for k in KS if len(k) == 1} == {1, 2, 3, 5, 7, 8, 9}
    for f, n in (('acc', 2), ('relu', 2), ('mask', 2), ('wide', 2)):
        assert len({c[:2] for c in cases if c[4][f]}) >= n, f
    assert len({c[:2] for c in cases if c[4]['nbias'] == 3}) >= 2


@pytest.mark.parametrize('i', range(30))
def test_linear_fwd_each_tile_vs_fp64(i):
    """Split off; overrides 0-4 and override 1 with MD off (the register-staged 64-row NT kernel): one launch each, the
    counters name the kernel; fp64 at atol 3e-5 + rtol 1e-5; the six results agree in bits.  M in {1 .. 300}, N in
    {1, 4, 124, 128, 130 (ldc 130 / 132), 132, 260}, 1-9 chunks, segment switches at every ring position, lda / ldw > K,
    0 / 1 / 3 biases, accumulate, ReLU, keep-mask + scale + out_pre.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X, worst case: 10.94 on all six kernels alike (they agree
    in bits), at case 24 (1 x 1, K = 288: one dot product, err_kernel 9.3e-8 against an err32 of 8.5e-9 that the CPU's
    blocked sum happens to reach there); every case with more than one output stays below 4."""
    M, N, ldc, Ks, feat = linear_case(i)
    x = LinearData(1000 + i, M, N, ldc, Ks, **feat)
    run_linear_all_tiles([x], '[%d %dx%d ldc%d K%s]' % (i, M, N, ldc, '+'.join(map(str, Ks))))


@pytest.mark.parametrize('v', (0, 1))
def test_linear_fwd_grouped_three_problems_each_tile(v):
    """A 3-problem launch of different shapes and features per override: tile_start / map_tile past problem 0."""
    shapes = [[(129, 260, (96,)), (33, 124, (32, 32, 32)), (300, 4, (64,))],
              [(65, 130, (64, 32, 96, 32)), (257, 128, (160,)), (1, 132, (32,))]][v]
    datas = [LinearData(2000 + 10 * v + j, M, N, (N + 3) // 4 * 4 + 4 if j != 1 else N, Ks, nbias=(3, 1, 0)[j],
                        acc=j == 0, relu=j != 2, mask=j == 1, wide=j == 2) for j, (M, N, Ks) in enumerate(shapes)]
    run_linear_all_tiles(datas, '[grouped %d]' % v)


# ------------------------------------------------------------------------------------------------ 2. LSTM, vocabulary
def lstm_ref(dt, segs, b_ih, b_hh, c0, pre, pre_div, tab, ids):
    z = sum(a.to(dt) @ w.to(dt).t() for a, w in segs)
    if b_ih is not None:
        z = z + b_ih.to(dt) + b_hh.to(dt)
    if pre is not None:
        z = z + pre.to(dt).repeat_interleave(pre_div, dim=0)
    if tab is not None:
        z = z + tab.to(dt)[ids]
    H = c0.shape[1]
    i, f, gg, o = z.split(H, dim=1)
    c = torch.sigmoid(f) * c0.to(dt) + torch.sigmoid(i) * R.tanh_(gg)
    h = torch.sigmoid(o) * R.tanh_(c)
    return {'h': h, 'c': c, 'gates': torch.cat([torch.sigmoid(i), torch.sigmoid(f), R.tanh_(gg), torch.sigmoid(o)], 1)}


class LstmData:
    def __init__(self, seed, M, H, Ks, full, pre_div=1):
        g = gen(seed)
        self.M, self.H, self.full, self.pre_div = M, H, full, pre_div
        Kt = sum(Ks)
        self.segs = [(uni(g, M, K), uni(g, 4 * H, K, scale=Kt ** -0.5)) for K in Ks]
        self.dsegs = [(a.to(DEV), w.to(DEV)) for a, w in self.segs]
        self.b_ih, self.b_hh, self.c0 = uni(g, 4 * H), uni(g, 4 * H), uni(g, M, H)
        self.pre = uni(g, M // pre_div, 4 * H, scale=0.3) if full else None
        self.tab = uni(g, 50, 4 * H, scale=0.3) if full else None
        self.ids = torch.randint(0, 50, (M,), generator=g) if full else None
        self.keep = (torch.rand(M, H, generator=g) > 0.5).to(torch.uint8) if full else None
        self.dev = [d(v) for v in (self.b_ih, self.b_hh, self.c0, self.pre, self.tab, self.ids, self.keep)]
        self.ref, self.ev = R.both(lstm_ref, self.segs, self.b_ih, self.b_hh, self.c0, self.pre, pre_div, self.tab, self.ids)

    def run(self, ws, want, kernel, case, segs=None):
        """One launch; `want` = the counter deltas.  Returns (h, c) on the host."""
        M, H = self.M, self.H
        hb, cb = torch.full((M + 1, H), SENT, device=DEV), torch.full((M + 1, H), SENT, device=DEV)
        gb = torch.full((M + 1, 4 * H), SENT, device=DEV) if self.full else None
        db = torch.full((M + 1, H), SENT, device=DEV) if self.full else None
        hp = torch.empty(2, M, H, dtype=torch.float16, device=DEV) if self.full else None
        b_ih, b_hh, c0, pre, tab, ids, keep = self.dev
        with ran(want):
            ops.lstm_fwd(segs or self.dsegs, b_ih, b_hh, c0, hb[:M], cb[:M], gates_out=None if gb is None else gb[:M],
                         h_keep_mask=keep, mask_scale=2.0, hdrop_out=None if db is None else db[:M], pre=pre, tab=tab,
                         tab_ids=ids, h_planes=hp, pre_div=self.pre_div, ws=ws)
            torch.cuda.synchronize()
        hold(hb, self.ref['h'], self.ev['h'], kernel, case + ' h', atol=2e-5, rtol=0)
        hold(cb, self.ref['c'], self.ev['c'], kernel, case + ' c', atol=2e-5, rtol=0)
        if self.full:
            hold(gb, self.ref['gates'], self.ev['gates'], kernel, case + ' gates', atol=2e-5, rtol=0)
            assert torch.equal(db[:M], hb[:M] * keep.float() * 2.0) and bool((db[M:] == SENT).all()), case
            assert torch.equal(hp, _planes(hb[:M])), case + ': planes != a re-split of h'
        return hb[:M].cpu(), cb[:M].cpu()


@pytest.mark.parametrize('M,H,pre_div', [(33, 32, 3), (129, 96, 1), (300, 32, 2), (300, 96, 2)])
def test_lstm_fwd_each_tile_vs_fp64(M, H, pre_div):
    """pre (one row per pre_div rows: 2 at M = 300; the entry point asks M % pre_div == 0, so the odd M run 3 and 1), tab,
    keep-mask, planes, gates_out; split off.  Overrides 0, 1, 2, 4 run the
    register-staged 128 / 64 / 32-row kernels and LD; override 3 with `pre` runs tile 0 (allow_xl is false).  h, c and
    gates at 2e-5 against fp64, hdrop and planes exact, h and c equal in bits across the five.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X, worst case: 1.82 (c, 129 x 96) on every kernel."""
    x = LstmData(M * 7 + H, M, H, (H, 2 * H, 32), True, pre_div)
    off_buf, off = private_ws(1)
    base = None
    for t, kind, name in ((0, 0, 'gemm_kernel<L,NT,lstm>'), (1, 1, 'gemm_kernel<M,NT,lstm>'), (2, 2, 'gemm_kernel<S,NT,lstm>'),
                          (4, 4, 'gemm_ld_kernel<lstm>'), (3, 0, 'gemm_kernel<L,NT,lstm>')):
        ops.set_tile_override(t)
        cur = x.run(off, {kind: 1}, name, '[%dx%d div%d ovr%d]' % (M, H, pre_div, t))
        base = base or cur
        assert torch.equal(base[0], cur[0]) and torch.equal(base[1], cur[1]), t
    ws_intact(off_buf, 1)


@pytest.mark.parametrize('M,H', [(33, 32), (257, 96), (300, 32)])
def test_lstm_fwd_bias_only_xl_ragged_rows(M, H):
    """The bias-only cell under override 3 runs gemm_xl_kernel<EPI_LSTM> (kind 3) at row counts that are no multiple of
    256: fp64 at 2e-5, and the bits of tile 0.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X, worst case: 2.35 (h, 257 x 96), XL and tile 0 alike."""
    x = LstmData(M * 11 + H, M, H, (H, 2 * H, 32), False)
    off_buf, off = private_ws(1)
    ops.set_tile_override(0)
    base = x.run(off, {0: 1}, 'gemm_kernel<L,NT,lstm>', '[%dx%d bias-only]' % (M, H))
    ops.set_tile_override(3)
    cur = x.run(off, {3: 1}, 'gemm_xl_kernel<lstm>', '[%dx%d bias-only]' % (M, H))
    assert torch.equal(base[0], cur[0]) and torch.equal(base[1], cur[1])
    ws_intact(off_buf, 1)


class VocabData:
    def __init__(self, seed, M, V, K):
        g = gen(seed)
        self.M, self.V, self.K, self.nt = M, V, K, (V + 127) // 128
        self.h, self.W, self.bias = uni(g, M, K), uni(g, V, K, scale=4 * K ** -0.5), uni(g, V)
        self.dh, self.dW, self.dbias = self.h.to(DEV), self.W.to(DEV), self.bias.to(DEV)
        self.ref = self.h.double() @ self.W.double().t() + self.bias.double()
        self.ev = self.h @ self.W.t() + self.bias
        self.lse_ref = torch.logsumexp(self.ref, 1)

    def run(self, ws, want, kernel, case, logits_pad=None):
        """One launch; logits_pad None: no logits, else ld_logits = V + logits_pad.  Returns (pm, ps, pi, logits) on the
        host after the statistics checks of test_vocab_all_tiles."""
        M, V, nt = self.M, self.V, self.nt
        pm, ps = torch.full((M + 1, nt), SENT, device=DEV), torch.full((M + 1, nt), SENT, device=DEV)
        pi = torch.full((M + 1, nt), ISENT, device=DEV, dtype=torch.int32)
        lb = lg = None
        if logits_pad is not None:
            lb, lg = outbuf(M, V, V + logits_pad)
        with ran(want):
            ops.vocab_fwd(self.dh, self.dW, self.dbias, pm[:M], ps[:M], pi[:M], lg, ws=ws)
            torch.cuda.synchronize()
        assert bool((pm[M:] == SENT).all()) and bool((ps[M:] == SENT).all()) and bool((pi[M:] == ISENT).all()), case
        mx = pm[:M].max(1).values
        lse = mx + torch.log((ps[:M] * torch.exp(pm[:M] - mx[:, None])).sum(1))
        np.testing.assert_allclose(lse.cpu().numpy(), self.lse_ref.float().numpy(), atol=3e-5, rtol=1e-5, err_msg=case)
        col = pm[:M].argmax(1)                                   # first tile holding the row maximum
        arg = pi[:M].gather(1, col[:, None]).squeeze(1).long()
        if lg is not None:
            hold(lb, self.ref, self.ev, kernel, case, atol=3e-5)
            assert torch.equal(arg, lg.argmax(1)), case           # same fp32 values -> same arg-max, ties to the lower id
            tiles = torch.nn.functional.pad(lg, (0, nt * 128 - V), value=float('-inf')).view(M, nt, 128)
            assert torch.equal(pm[:M], tiles.max(2).values), case
        return pm[:M].cpu(), ps[:M].cpu(), pi[:M].cpu(), None if lg is None else lg.cpu()


VOCAB_TILES = ((0, 0, 'gemm_kernel<L,NT,vocab>'), (1, 1, 'gemm_kernel<M,NT,vocab>'), (2, 2, 'gemm_kernel<S,NT,vocab>'),
               (4, 4, 'gemm_ld_kernel<vocab>'), (3, 0, 'gemm_kernel<L,NT,vocab>'))


@pytest.mark.parametrize('M,V,K', [(33, 130, 96), (129, 1000, 64), (33, 1002, 160), (129, 1283, 96)])
def test_vocab_fwd_each_tile_vs_fp64(M, V, K):
    """Split off.  Overrides 0, 1, 2, 4: the register-staged tiles and LD; override 3 runs tile 0 (isc_vocab_fwd never
    allows XL: gemm_xl_kernel<EPI_VOCAB> has no caller).  With logits (ld_logits = V and V + 6) and without; lse and
    logits against fp64, the arg-max against the kernel's own logits, the tile maxima against them in bits; logits,
    maxima and arg-max ids in bits across the overrides (test_vocab_all_tiles' set: the 64-row tile folds the exp sums of
    two waves per row, so part_sum is held through lse), every statistic in bits across with / without logits.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X, worst case: logits 1.27 (129 x 1000 x 64), every tile."""
    x = VocabData(V + M, M, V, K)
    off_buf, off = private_ws(1)
    base = None
    for t, kind, name in VOCAB_TILES:
        ops.set_tile_override(t)
        case = '[%dx%dx%d ovr%d]' % (M, V, K, t)
        a = x.run(off, {kind: 1}, name, case, logits_pad=0)
        b = x.run(off, {kind: 1}, name, case + ' ld+6', logits_pad=6)
        c = x.run(off, {kind: 1}, name, case + ' no logits')
        base = base or a
        for r in (b, c):                      # one kernel, with / without logits: every statistic in bits
            assert all(torch.equal(p, q) for p, q in zip(a[:3], r[:3])), case
        # across tiles: maxima, arg-max ids and logits (the 64-row tile folds two waves' exp sums: part_sum may differ)
        assert torch.equal(base[0], a[0]) and torch.equal(base[2], a[2]), case
        assert torch.equal(base[3], a[3]) and torch.equal(base[3], b[3]), case
    ws_intact(off_buf, 1)


# ------------------------------------------------------------------------------------------------ 3. backward NN / TN
def bwd_ref(dt, layout, segs, prior, bias):
    if layout == ops.NN:
        z = sum(a.to(dt)[:, :w.shape[0]] @ w.to(dt) for a, w in segs)
    else:
        z = sum(a.to(dt).t() @ w.to(dt) for a, w in segs)
    if bias is not None:
        z = z + bias.to(dt)
    return {'out': z if prior is None else z + prior.to(dt)}


class BwdData:
    """One backward problem: NN A_s [M, lda] (zero padding to a multiple of 4, NaN past it where lda is wider: never
    read), W_s [K_s, N]; TN A_s [K_s, M], W_s [K_s, N]; every operand a column slice; out a column slice."""

    def __init__(self, seed, layout, M, N, Ks, acc, bias):
        g = gen(seed)
        self.layout, self.M, self.N, self.Ks = layout, M, N, Ks
        Kt = sum(Ks)
        self.segs, self.dsegs, self.keepalive = [], [], []
        for j, K in enumerate(Ks):
            if layout == ops.NN:
                K4 = (K + 3) // 4 * 4
                a = torch.full((M, K4 + 4 * (j % 2)), float('nan'))
                a[:, :K4] = 0
                a[:, :K] = uni(g, M, K)
                w = uni(g, K, N + 8, scale=Kt ** -0.5)
                self.segs.append((a, w[:, 4:4 + N]))
                da, dw = a.to(DEV), w.to(DEV)
                self.dsegs.append((da, dw[:, 4:4 + N]))
            else:
                a, w = torch.randn(K, M + 4, generator=g), torch.randn(K, N + 8, generator=g)
                self.segs.append((a[:, 4:], w[:, 4:4 + N]))
                da, dw = a.to(DEV), w.to(DEV)
                self.dsegs.append((da[:, 4:], dw[:, 4:4 + N]))
            self.keepalive += [da, dw]
        self.prior = uni(g, M, N) if acc else None
        self.bias = uni(g, N) if bias else None
        self.dbias = d(self.bias)
        self.ref, self.ev = R.both(bwd_ref, layout, self.segs, self.prior, self.bias)
        self.atol = 3e-5 if layout == ops.NN else 2e-4 * max(1.0, Kt ** 0.5 / 8)

    def problem(self, segs=None, plain=False):
        buf = torch.full((self.M + 1, self.N + 12), SENT, device=DEV)
        out = buf[:self.M, 4:4 + self.N]
        if self.prior is not None and not plain:
            out.copy_(self.prior)
        if plain:
            return ops.gemm_problem(segs, out, self.layout), buf
        return ops.gemm_problem(self.dsegs, out, self.layout, accumulate=self.prior is not None, bias0=self.dbias), buf

    def check(self, buf, kernel, case):
        got = buf.cpu()
        assert bool((got[:, :4] == SENT).all()) and bool((got[:, 4 + self.N:] == SENT).all()), case
        hold(buf[:, 4:4 + self.N], self.ref['out'], self.ev['out'], kernel, case, atol=self.atol)

    def sub_segments(self, c0, c1):
        """Device views of the operands over chunks [c0, c1) of the problem's chunk sequence."""
        out = []
        for s, k0, k1 in chunk_slices(self.Ks, c0, c1):
            a, w = self.dsegs[s]
            out.append((a[:, k0:], w[k0:k1]) if self.layout == ops.NN else (a[k0:k1], w[k0:k1]))
        return out


NN_M, NN_K = (1, 33, 65, 129, 130), (1, 5, 32, 33, 100, 288, 290)
TN_M, TN_K = (4, 36, 64, 68, 132), (1, 6, 31, 32, 33, 80, 100, 290)
BWD_N = (4, 124, 128, 132, 260)


def bwd_launch(layout, i):
    """Launch i of the table: 1-3 problems of different shapes, 1-4 segments each; the lists are walked in step so
    every M, N and K_s of the issue appears."""
    Ms, Kv = (NN_M, NN_K) if layout == ops.NN else (TN_M, TN_K)
    probs = []
    for j in range(i % 3 + 1):
        q = 2 * i + j
        nseg = (i + j) % 4 + 1
        Ks = tuple(Kv[(3 * i + 2 * j + s) % len(Kv)] for s in range(nseg))
        probs.append((Ms[q % 5], BWD_N[(q + i // 5) % 5], Ks, q % 2 == 1, q % 3 == 0))
    return probs


def test_bwd_case_table_covers_the_issue_values():
    for layout, Ms, Kv in ((ops.NN, NN_M, NN_K), (ops.TN, TN_M, TN_K)):
        ps = [p for i in range(10) for p in bwd_launch(layout, i)]
        assert {p[0] for p in ps} == set(Ms) and {p[1] for p in ps} == set(BWD_N)
        assert {k for p in ps for k in p[2]} == set(Kv) and {len(p[2]) for p in ps} == {1, 2, 3, 4}
        assert {p[3] for p in ps} == {False, True} == {p[4] for p in ps}


BWD_KERNEL = {0: 'gemm_kernel<L,%s>', 1: 'gemm_kernel<M,%s>', 2: 'gemm_kernel<S,%s>', 3: 'gemm_kernel<L,%s>', 4: 'gemm_kernel<L,%s>'}


@pytest.mark.parametrize('i', range(10))
@pytest.mark.parametrize('layout', ('NN', 'TN'))
def test_gemm_bwd_each_tile_vs_fp64(layout, i):
    """Split off.  Overrides 0, 1, 2 run gemm_kernel on the 128 / 64 / 32-row tile in the k-major layouts; overrides 3
    and 4 fall back to tile 0 (the LDS-DMA tiles are NT only) - all by the counters.  1-3 problems, 1-4 segments, K tails
    (K_s % 32, NN K_s % 4 with zero padding), accumulate 0 / 1 on a pre-filled out, bias0, operands and out column slices.
    fp64 at the NN / TN bars; the five results agree in bits.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X, worst case: NN 3.85 (65 x 132, K 288+290+1+5), TN 3.66
    (68 x 132, rows 80+100+290), the three tiles alike."""
    lay = ops.NN if layout == 'NN' else ops.TN
    datas = [BwdData(3000 + 100 * i + 10 * j + lay, lay, *p) for j, p in enumerate(bwd_launch(lay, i))]
    off_buf, off = private_ws(1)
    base = None
    for t in (0, 1, 2, 3, 4):
        ops.set_tile_override(t)
        probs = [x.problem() for x in datas]
        set_ws(probs[0][0], off)
        with ran({t if t < 3 else 0: 1}):
            ops.gemm_bwd([p[0] for p in probs], lay)
            torch.cuda.synchronize()
        for j, (x, (_, buf)) in enumerate(zip(datas, probs)):
            x.check(buf, BWD_KERNEL[t] % layout, '[%d.%d %dx%d K%s ovr%d]' % (i, j, x.M, x.N, '+'.join(map(str, x.Ks)), t))
        cur = [p[1].cpu() for p in probs]
        base = base or cur
        assert all(torch.equal(a, b) for a, b in zip(base, cur)), 'override %d differs from tile 0 in bits' % t
    ws_intact(off_buf, 1)


def test_gemm_bwd_refusals_launch_nothing():
    """Each bad argument is answered with its code on the host: no counter moves, the output keeps its sentinel."""
    lib = _lib.load()
    g = gen(9)
    a_nn, w, a_tn = d(uni(g, 8, 40)), d(uni(g, 40, 16)), d(uni(g, 40, 8))
    buf = torch.full((9, 20), SENT, device=DEV)

    def base(layout):
        return ops.gemm_problem([(a_nn if layout == ops.NN else a_tn[:32], w[:32])], buf[:8, :16], layout)

    def edit(layout, **kw):
        p = base(layout)
        for k, v in kw.items():
            if k in ('A', 'W', 'lda', 'ldw', 'K'):
                setattr(p.seg[0], k, v)
            else:
                setattr(p, k, v)
        return p

    cases = [(ops.NN, dict(N=14), -2), (ops.TN, dict(N=14), -2), (ops.NN, dict(ldc=18), -2), (ops.TN, dict(M=6), -2),
             (ops.NN, dict(lda=38), -3), (ops.TN, dict(ldw=18), -3), (ops.NN, dict(A=a_nn.data_ptr() + 4), -3),
             (ops.TN, dict(W=w.data_ptr() + 8), -3), (ops.NN, dict(K=0), -2), (ops.TN, dict(K=-32), -2),
             (ops.NN, dict(C=None), -1), (ops.TN, dict(C=None), -1)]
    for t in (-1, 0, 1, 2):
        ops.set_tile_override(t)
        for layout, kw, code in cases:
            p = edit(layout, **kw)
            with ran({}):
                assert lib.isc_gemm_bwd(C.byref(p), 1, layout, ops.stream()) == code, (kw, code)
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
    ops.set_tile_override(0)
    with ran({0: 1}):                                  # the unedited problem is taken: the refusals were the edits'
        ops.gemm_bwd([base(ops.NN)], ops.NN)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. split-K
def restated_partials(x, S, run):
    """The S slabs of a split-K launch restated: one split-off 32-row launch per K sub-range [s cps, (s + 1) cps) chunks
    (an empty range: zeros).  `run(problem)` launches one plain problem; x.problem(segs, plain=True) builds it."""
    chunks = n_chunks(x.Ks)
    cps = (chunks + S - 1) // S
    parts = []
    for s in range(S):
        segs = x.sub_segments(s * cps, min((s + 1) * cps, chunks)) if s * cps < chunks else []
        if not segs:
            parts.append(torch.zeros(x.M, x.N))
            continue
        made = x.problem(segs, plain=True)
        run(made[0])
        out = made[1][:x.M, 4:4 + x.N] if isinstance(x, BwdData) else made[1][:x.M, :x.N]
        parts.append(out.cpu().clone())
    return parts


def _lin_sub_segments(self, c0, c1):
    return [(self.dsegs[s][0][:, k0:k1], self.dsegs[s][1][:, k0:k1]) for s, k0, k1 in chunk_slices(self.Ks, c0, c1)]


LinearData.sub_segments = _lin_sub_segments


def finish_on_host(v, biases, prior, relu, keep, scale):
    """epi_linear_finish in its order, in fp32: biases, prior, ReLU, (pre-mask copy,) mask * scale."""
    for b in biases:
        v = v + b
    if prior is not None:
        v = v + prior
    if relu:
        v = torch.relu(v)
    return (v if keep is None else v * keep.float() * scale), v


LIN_SPLIT = [((2080,), 2), ((2080,), 3), ((2080,), 5), ((2080,), 16), ((96, 992, 416), 2), ((96, 992, 416), 3),
             ((96, 992, 416), 5)]


@pytest.mark.parametrize('Ks,S', LIN_SPLIT)
@pytest.mark.parametrize('nprob', (1, 2))
def test_splitk_linear_fwd_bit_equals_restated_slabs(Ks, S, nprob):
    """Mode 0, no override, M = 16, N = 128: the 32-row tile writes S slabs (kind 2) and splitk_linear_kernel finishes
    them (kind 6).  K = 2080 at S = 16 leaves slices 13-15 empty; (96, 992, 416) puts slices across segment borders;
    three biases, accumulate, ReLU, keep-mask + scale + out_pre; a second problem of another shape.  fp64 at the bar and
    bit equality with the restated slab sum + epilogue; the workspace's sentinels survive.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X, worst case of splitk_linear_kernel, forward and
    backward: 2.90 (NN 20 x 128, K = 2065, S = 2)."""
    ops.set_h3_mode(0)
    datas = [LinearData(4000 + S, 16, 128, 128, Ks, nbias=3, acc=True, relu=True, mask=True)]
    if nprob == 2:
        datas.append(LinearData(4100 + S, 9, 132, 136, Ks[::-1], nbias=1, acc=True, wide=True))
    blocks = sum((x.M + 31) // 32 * ((x.N + 127) // 128) for x in datas)
    assert split_caps(blocks, min(n_chunks(x.Ks) for x in datas)) >= S
    if Ks == (2080,) and S == 16:
        assert (S - 1) * ((65 + S - 1) // S) >= 65                  # empty K-slices
    floats = S * sum(x.M * x.N for x in datas)
    ws_buf, ws = private_ws(floats)
    probs = [x.problem() for x in datas]
    set_ws(probs[0][0], ws)
    with ran({2: 1, 6: 1}):
        ops.linear_fwd([p[0] for p in probs])
        torch.cuda.synchronize()
    ws_intact(ws_buf, floats)
    off_buf, off = private_ws(1)
    ops.set_tile_override(2)

    def run(p):
        set_ws(p, off)
        with ran({2: 1}):
            ops.linear_fwd([p])
            torch.cuda.synchronize()

    for j, (x, (_, buf, pbuf)) in enumerate(zip(datas, probs)):
        case = '[%dx%d K%s S%d p%d]' % (x.M, x.N, '+'.join(map(str, x.Ks)), S, j)
        x.check(buf, pbuf, 'splitk_linear_kernel', case)
        want, want_pre = finish_on_host(slab_sum(restated_partials(x, S, run)), x.biases, x.prior, x.relu, x.keep, x.scale)
        assert torch.equal(buf[:x.M, :x.N].cpu(), want), case + ': not the restated slab sum in bits'
        if pbuf is not None:
            assert torch.equal(pbuf[:x.M, :x.N].cpu(), want_pre), case
    ws_intact(off_buf, 1)


BWD_SPLIT = [((2065,), 2), ((2065,), 3), ((2065,), 5), ((2065,), 16), ((100, 1000, 33), 2), ((100, 1000, 33), 3),
             ((100, 1000, 33), 5)]


@pytest.mark.parametrize('Ks,S', BWD_SPLIT)
@pytest.mark.parametrize('layout', ('NN', 'TN'))
def test_splitk_gemm_bwd_bit_equals_restated_slabs(layout, Ks, S):
    """Mode 0, no override: the k-major 32-row kernel writes S slabs over K = 2065 / (100, 1000, 33) - K tails inside
    slices, slices across segment borders, empty slices at S = 16 - and splitk_linear_kernel adds bias0 and the prior
    once.  fp64 at the NN / TN bars and bit equality with the restated slab sum."""
    ops.set_h3_mode(0)
    lay = ops.NN if layout == 'NN' else ops.TN
    M, N = (20, 128) if lay == ops.NN else (36, 132)
    x = BwdData(5000 + S + lay, lay, M, N, Ks, True, True)
    assert split_caps((M + 31) // 32 * ((N + 127) // 128), n_chunks(Ks)) >= S
    floats = S * M * N
    ws_buf, ws = private_ws(floats)
    p, buf = x.problem()
    set_ws(p, ws)
    with ran({2: 1, 6: 1}):
        ops.gemm_bwd([p], lay)
        torch.cuda.synchronize()
    ws_intact(ws_buf, floats)
    case = '[%s %dx%d K%s S%d]' % (layout, M, N, '+'.join(map(str, Ks)), S)
    x.check(buf, 'splitk_linear_kernel', case)
    off_buf, off = private_ws(1)
    ops.set_tile_override(2)

    def run(q):
        set_ws(q, off)
        with ran({2: 1}):
            ops.gemm_bwd([q], lay)
            torch.cuda.synchronize()

    want, _ = finish_on_host(slab_sum(restated_partials(x, S, run)), [x.bias], x.prior, False, None, 1.0)
    assert torch.equal(buf[:M, 4:4 + N].cpu(), want), case + ': not the restated slab sum in bits'
    ws_intact(off_buf, 1)


@pytest.mark.parametrize('M,H,Ks,S,full', [(16, 32, (32, 64, 512), 2, True), (40, 64, (64, 128, 512), 5, True),
                                           (40, 32, (1024,), 3, False), (16, 64, (1024,), 5, True),
                                           (16, 64, (64, 128, 512), 3, False), (40, 32, (32, 64, 512), 3, True)])
def test_splitk_lstm_vs_fp64(M, H, Ks, S, full):
    """Mode 0, no override: slabs by the 32-row linear tile (kind 2), the cell by splitk_lstm_kernel (kind 6).  With
    pre (pre_div 2), tab, mask, planes and gates_out, and bare.  h, c, gates at 2e-5; planes equal a re-split of h.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X, worst case: 1.77 (c, 16 x 64, K 64+128+512, S = 3)."""
    ops.set_h3_mode(0)
    x = LstmData(M + H + S, M, H, Ks, full, 2 if full else 1)
    assert split_caps((M + 31) // 32 * (4 * H // 128), n_chunks(Ks)) >= S
    floats = S * M * 4 * H
    ws_buf, ws = private_ws(floats)
    x.run(ws, {2: 1, 6: 1}, 'splitk_lstm_kernel', '[%dx%d K%s S%d full%d]' % (M, H, '+'.join(map(str, Ks)), S, full))
    ws_intact(ws_buf, floats)


@pytest.mark.parametrize('K,S', [(512, 2), (512, 3), (2080, 5), (2080, 16)])
def test_splitk_vocab_bit_equals_restated_slabs(K, S):
    """Mode 0, no override, M = 12, V = 1000: slabs by the 32-row linear tile (kind 2), bias + statistics by
    splitk_vocab_kernel (kind 6).  Logits (ld_logits = V and V + 6) equal the restated slab sum + bias in bits; the
    statistics checks of the tile test; the same statistics without logits.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X, worst case: logits 2.00 (K = 2080, S = 5)."""
    ops.set_h3_mode(0)
    M, V = 12, 1000
    x = VocabData(K + S, M, V, K)
    assert split_caps(8, K // 32) >= S
    floats = S * M * V
    ws_buf, ws = private_ws(floats)
    case = '[%dx%dx%d S%d]' % (M, V, K, S)
    a = x.run(ws, {2: 1, 6: 1}, 'splitk_vocab_kernel', case, logits_pad=0)
    b = x.run(ws, {2: 1, 6: 1}, 'splitk_vocab_kernel', case + ' ld+6', logits_pad=6)
    c = x.run(ws, {2: 1, 6: 1}, 'splitk_vocab_kernel', case + ' no logits')
    ws_intact(ws_buf, floats)
    for r in (b, c):
        assert all(torch.equal(p, q) for p, q in zip(a[:3], r[:3])), case
    assert torch.equal(a[3], b[3])
    off_buf, off = private_ws(1)
    ops.set_tile_override(2)
    chunks = K // 32
    cps = (chunks + S - 1) // S
    parts = []
    for s in range(S):
        k0, k1 = s * cps * 32, min((s + 1) * cps, chunks) * 32
        if k0 >= k1:
            parts.append(torch.zeros(M, V))
            continue
        buf, out = outbuf(M, V, V + 4)
        p = ops.linear_problem([(x.dh[:, k0:k1], x.dW[:, k0:k1])], out)
        set_ws(p, off)
        with ran({2: 1}):
            ops.linear_fwd([p])
            torch.cuda.synchronize()
        parts.append(out.cpu().clone())
    assert torch.equal(a[3], slab_sum(parts) + x.bias), case + ': logits are not the restated slab sum + bias in bits'
    ws_intact(off_buf, 1)


def test_vocab_with_columns_off_four_does_not_split():
    """V = 1002 (N % 4 != 0): plan_splitk declines whatever the workspace - one tile launch, no reduce."""
    ops.set_h3_mode(0)
    x = VocabData(77, 12, 1002, 512)
    ws_buf, ws = private_ws(4 * 12 * 1002)
    before = counters()
    pm, ps = torch.full((13, x.nt), SENT, device=DEV), torch.full((13, x.nt), SENT, device=DEV)
    pi = torch.full((13, x.nt), ISENT, device=DEV, dtype=torch.int32)
    lb, lg = outbuf(12, 1002, 1002)
    ops.vocab_fwd(x.dh, x.dW, x.dbias, pm[:12], ps[:12], pi[:12], lg, ws=ws)
    torch.cuda.synchronize()
    delta = tuple(a - b for a, b in zip(counters(), before))
    assert delta[6] == 0 and sum(delta[:6]) == 1 and delta[7:] == (0, 0, 0), delta
    hold(lb, x.ref, x.ev, 'vocab (no split)', '[12x1002x512]', atol=3e-5)
    assert bool((ws_buf == SENT).all())


def test_zz_report_the_measured_ratios():
    """Prints err_kernel / max(err32, 2^-23 max|ref|), worst case per kernel (pytest -s).  Not asserted on: the CPU's
    blocked fp32 summation is not the kernels' order.  Measured on an MI355X: the docstrings above; the largest of all is
    10.94 (a single dot product of K = 288), everything else stays below 4."""
    for k in sorted(WORST):
        ratio, err, err32, case = WORST[k]
        print('WORST %-26s ratio %5.2f  err_kernel %.3e  err32 %.3e  at %s' % (k, ratio, err, err32, case))
