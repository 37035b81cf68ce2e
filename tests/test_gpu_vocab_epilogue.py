"""The classifier GEMM on the large split-f16 tiles under both geometries (csrc/gemm_f32.hip: gemm_h3_kernel<VOCAB, .> on
128 x 128 tiles, gemm_h3x_kernel<VOCAB, .> on 256 x 128; launch_h3_big chooses, ops.set_h3_vocab_tile forces).

Both kernels reach the one statistics epilogue (epi_vocab_frag over Frag16, eight column blocks per wave), so a row's
part_max / part_sum / part_idx and logits must be the same BITS whichever geometry the row count picks: the roll-out
compares half batches with whole ones by torch.equal (tests/test_gpu_parity.py).  Float tensors are compared through their
int32 views - equal bits, NaNs included."""
import contextlib
import functools

import pytest
import torch

from _split_f16 import planes as split_planes
from insenticap_model_amd import Captioner, _lib, ops, synth
from test_gpu_h3_kernels import Vocab, large_want, ran, vocab_all

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NONE = 0x7fffffff                     # part_idx of a tile whose logits are -inf / NaN alone


@contextlib.contextmanager
def routing(mode, tile):
    """h3 mode and classifier tile geometry for the block; both restored whatever happens inside."""
    prev_mode, prev_tile = ops.set_h3_mode(mode), ops.set_h3_vocab_tile(tile)
    try:
        yield
    finally:
        ops.set_h3_vocab_tile(prev_tile)
        ops.set_h3_mode(prev_mode)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b, what):
    assert torch.equal(bits(a), bits(b)), '%s: %d of %d elements differ in bits' % (
        what, int((bits(a) != bits(b)).sum()), a.numel())


# ------------------------------------------------------------------------------------------------ 1. the 256-row kernel
@functools.lru_cache(maxsize=None)
def lattice_case(M, V, K):
    return Vocab(2100 + M + V + K, M, V, K)


@pytest.mark.parametrize('planes', (True, False))
@pytest.mark.parametrize('K', (64, 160))
@pytest.mark.parametrize('M,V', [(257, 14353), (1, 28545)])
def test_h3x_256_row_tile_vocab(M, V, K, planes):
    """gemm_h3x_kernel<VOCAB, false / true> (kinds 3 / 4; isc_h3x_launches), mode 2: 2 x 113 = 226 tiles with one live row
    in the second row tile, and 224 tiles with one live row in all - the tile counts from which the other epilogues take
    this geometry; 2 and 5 chunks on the ring of three; edge tiles of 17 and 1 columns.  Held as test_h3_128_row_tile_vocab
    holds the 128-row kernel: part_max / part_idx / logits (ld = V, V + 6, none) exact against the lattice's fp64
    evaluation, tile and row log-sum-exp within its tolerances, sentinels and workspace intact.
    The geometry is forced: auto keeps the classifier on 128 rows at every tile count, because that measured faster at the
    benchmark's shape (launch_h3_big) - which the last lines pin with the same operands."""
    assert (M + 255) // 256 * ((V + 127) // 128) >= 224
    x, what = lattice_case(M, V, K), '[%dx%dx%d]' % (M, V, K)
    with routing(2, 256):
        vocab_all(x, large_want(256, planes), 'h3x 256 vocab ' + what, planes)
    with routing(2, 0):
        x.run(large_want(128, planes), 'h3 128 vocab on auto ' + what, planes, logits_pad=6)


# ------------------------------------------------------------------------------------------------ 2. geometry independence
DUP_SRC = 21
# copies of W row / bias 21 (column block 1, lane 5), all of them the maximum of every ordinary row of their tile:
#   26: another lane of the same column block;  128 + 22 / 128 + 70: one lane, column blocks 1 / 4;  256 + 100 / 256 + 41:
#   lane 4 of block 6 against lane 9 of block 2 - the LOWER column sits in the HIGHER lane;  384 + 7 / 640 + 7: other tiles;
#   1024 + 3 / 1024 + 16: inside the edge tile of 17 and of 127 columns
DUPS = (21, 26, 150, 198, 356, 297, 391, 647, 1027, 1040)
K0 = 5                                # the k at which the special rows are planted
ROW_INF, ROW_NAN = 3, -2              # rows (M >= 255) with +inf (and NaN) logits / with NaN logits alone


class Plain:
    """Random fp32 operands with tied tile maxima and, from 255 rows on, two rows of non-finite logits.  Column K0 of W is
    1 + 2^-12 (hi plane 1, lo plane > 0) but for 0 in the first column of every tile.  On planes, row ROW_INF of h is +inf
    at K0 and 0 elsewhere (lo plane 0): its logits are +inf but for the NaN of inf * 0 in each tile's first column.  Row
    ROW_NAN holds a NaN at K0: every logit is NaN.  (On fp32 rows the kernel splits +inf itself, lo = inf - inf: that row
    is NaN throughout as well.)"""

    def __init__(self, M, V, K):
        g = torch.Generator().manual_seed(7000 + 31 * M + V + K)
        self.M, self.V, self.K, self.nt = M, V, K, (V + 127) // 128
        h = torch.randn(M, K, generator=g)
        W = torch.randn(V, K, generator=g) * 0.05
        bias = torch.randn(V, generator=g) * 0.1
        W[:, K0] = 1.0 + 2.0 ** -12
        W[0::128, K0] = 0.0
        self.dups = [c for c in DUPS if c < V]
        for c in self.dups:
            W[c] = W[DUP_SRC]
        bias[self.dups] = 30.0                                      # |other logits| stay below 10
        self.special = M >= 255
        hi = h.to(torch.float16)
        lo = ((h - hi.float()) * 2048.0).to(torch.float16)
        if self.special:
            self.r_inf, self.r_nan = ROW_INF, M + ROW_NAN
            h[self.r_inf] = 0.0
            h[self.r_inf, K0] = float('inf')
            hi[self.r_inf], lo[self.r_inf] = 0.0, 0.0
            hi[self.r_inf, K0] = float('inf')
            h[self.r_nan, K0] = float('nan')
            hi[self.r_nan, K0], lo[self.r_nan, K0] = float('nan'), float('nan')
        # the interleaved plane layout of tests/_split_f16.py, from the patched planes
        self.h_planes = torch.stack([hi.view(M, K // 32, 32), lo.view(M, K // 32, 32)], dim=2).reshape(2, M, K).contiguous().to(DEV)
        if not self.special:
            assert torch.equal(self.h_planes.cpu(), split_planes(h))
        self.h, self.W, self.bias = h.to(DEV), W.to(DEV), bias.to(DEV)
        self.ordinary = torch.ones(M, dtype=torch.bool)
        if self.special:
            self.ordinary[[self.r_inf, self.r_nan]] = False

    def run(self, tile, planes):
        M, V, nt = self.M, self.V, self.nt
        pm, ps = torch.full((M, nt), 7.25, device=DEV), torch.full((M, nt), 7.25, device=DEV)
        pi = torch.full((M, nt), 123456789, device=DEV, dtype=torch.int32)
        lg = torch.full((M, V), 7.25, device=DEV)
        with routing(2, tile), ran(large_want(tile, planes)):
            ops.vocab_fwd(self.h, self.W, self.bias, pm, ps, pi, lg, h_planes=self.h_planes if planes else None)
            torch.cuda.synchronize()
        return pm.cpu(), ps.cpu(), pi.cpu(), lg.cpu()

    def check_ties(self, pm, pi, lg, planes, what):
        """Every ordinary row: a tile that holds copies reports the lowest of them, and all such tiles the same maximum."""
        rows = self.ordinary
        by_tile = {}
        for c in self.dups:
            by_tile.setdefault(c // 128, []).append(c)
        assert len(by_tile) >= 5 and any(len(v) > 1 for v in by_tile.values())
        first = pm[rows, DUP_SRC // 128]
        for t, cols in by_tile.items():
            for c in cols:
                same_bits(lg[rows, c], lg[rows, DUP_SRC], '%s: logits of the copy in column %d' % (what, c))
            same_bits(pm[rows, t], first, '%s: part_max of tile %d' % (what, t))
            same_bits(pm[rows, t], lg[rows, DUP_SRC], '%s: part_max of tile %d against the logit' % (what, t))
            assert bool((pi[rows, t] == min(cols)).all()), '%s: tile %d does not report the lowest of columns %r' % (what, t, cols)
        if self.special:
            assert bool(torch.isnan(lg[self.r_nan]).all()) and bool((pi[self.r_nan] == NONE).all())
            assert bool((pm[self.r_nan] == float('-inf')).all())
            if planes:                                               # +inf everywhere but each tile's first column
                want = torch.tensor([t * 128 + 1 if t * 128 + 1 < self.V else NONE for t in range(self.nt)], dtype=torch.int32)
                assert bool(torch.isnan(lg[self.r_inf, 0::128]).all())
                assert torch.equal(pi[self.r_inf], want), '%s: a NaN was selected, or not the first +inf' % what
                assert bool((pm[self.r_inf][want != NONE] == float('inf')).all())


@pytest.mark.parametrize('K', (32, 96))
@pytest.mark.parametrize('V', (1024, 1025, 1041, 1151))
def test_statistics_and_logits_do_not_depend_on_the_geometry(V, K):
    """The same operands under set_h3_vocab_tile(128) and (256), mode 2, M = 1 / 255 / 257 (one row; the last row of a
    128-row tile missing; one row into the next 256-row tile), no edge tile and edge tiles of 1, 17 and 127 columns, 1 and 3
    chunks, planes and fp32 rows: part_max, part_sum, part_idx and the logits in equal bits, with tied maxima in another
    lane, another column block and another tile (the lower column is reported) and with rows of +inf and of NaN logits."""
    for M in (1, 255, 257):
        x = Plain(M, V, K)
        for planes in (True, False):
            what = '[%dx%dx%d %s]' % (M, V, K, 'planes' if planes else 'rows')
            a, b = x.run(128, planes), x.run(256, planes)
            for name, u, v in zip(('part_max', 'part_sum', 'part_idx', 'logits'), a, b):
                same_bits(u, v, '%s %s under 128 and 256 rows' % (what, name))
            x.check_ties(a[0], a[2], a[3], planes, what)


# ------------------------------------------------------------------------------------------------ 3. the roll-out
def test_greedy_rollout_does_not_depend_on_the_classifier_geometry():
    """Greedy forward_rl, V = 10000, B = 520 (3 x 79 = 237 tiles of 256 rows, 5 x 79 of 128: past the skinny kernels'
    512 workgroups), T = 3, 4 regions, default widths, under auto, 128 and 256: seq, seq_logprobs, seq_masks equal, and
    the classifier's T launches counted in isc_h3x_launches under 256 and not under 128 or auto (= 128 rows)."""
    V, B, Tn, R = 10000, 520, 3, 4
    st = synth.DEFAULT_SETTINGS
    cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)
    cap.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(V, st, seed=0).items()})
    cap.to(DEV).eval()
    d = synth.make_inputs(B, V, st, regions=R, seq_len=Tn, seed=520)
    a = [torch.from_numpy(d[k]).to(DEV) for k in ('fc_feats', 'att_feats', 'cpt_words', 'senti_words', 'senti_labels')]
    lib = _lib.load()
    out, h3x = {}, {}
    for tile in (0, 128, 256):
        with routing(1, tile):
            n0 = lib.isc_h3x_launches()
            with torch.no_grad():
                out[tile] = [t.clone() for t in cap(*a, Tn, 1, mode='rl')]
            torch.cuda.synchronize()
            h3x[tile] = lib.isc_h3x_launches() - n0
    print('isc_h3x_launches per roll-out: %r' % h3x)
    for tile in (128, 256):
        for name, u, v in zip(('seq', 'seq_logprobs', 'seq_masks'), out[0], out[tile]):
            same_bits(u, v, '%s under auto and under %d rows' % (name, tile))
    # Every other launch of a step at these 520 rows has far fewer than 224 tiles of 256 rows (an LSTM cell: 3 x 2048 / 128
    # = 48) and stays off the 256-row kernel; the classifier's one launch per step is all that moves.  (At the benchmark's
    # batch both cells are on it as well: 2T under 128 rows, 3T under 256 - tests/test_gpu_bench_config.py pins the 2T.)
    others = 2 * Tn if (B + 255) // 256 * (4 * st['rnn_hid_dim'] // 128) >= 224 else 0
    assert others == 0
    assert h3x[128] == others and h3x[256] == others + Tn and h3x[0] == h3x[128], h3x


# ------------------------------------------------------------------------------------------------ 4. the setter
def test_the_setter_returns_the_previous_value_and_rejects_other_geometries():
    lib = _lib.load()
    first = ops.set_h3_vocab_tile(0)
    try:
        assert first == 0                                            # auto is the default, and every test puts it back
        assert ops.set_h3_vocab_tile(128) == 0
        assert ops.set_h3_vocab_tile(256) == 128
        for bad in (1, 64, 127, 129, 512, -1):
            with pytest.raises(ValueError):
                ops.set_h3_vocab_tile(bad)
            assert lib.isc_set_h3_vocab_tile(bad) == 256             # the library leaves the word as it is
        assert ops.set_h3_vocab_tile(0) == 256
        assert lib.isc_set_h3_vocab_tile(0) == 0
    finally:
        ops.set_h3_vocab_tile(first)
