"""The forward pointwise / scan kernels of csrc/pointwise.hip and csrc/attention.hip, one by one, against the fp64
references of tests/_fwd_ref.py at the shapes where a kernel goes wrong: unequal A / D / W, scalar fallbacks (sizes that
are no multiple of 4, misaligned views), every second trip of a lane loop, partial chunks, more than one block, optional
inputs null and given, leading dimensions wider than the row, rows and columns that belong to somebody else (sentinels),
and the refusals that must return before any launch.  Every call goes through ops.* or the ctypes structs of _lib.py.
The vocabulary statistics are made on the host (_fwd_ref.tile_stats): nothing here depends on isc_vocab_fwd.

Tolerances: the rule of tests/_bwd_ref.py, atol = 8 * max(err32, 2^-23 max|ref|) per floating output (err32: the same
formula in fp32 torch on the same inputs); torch.equal where an output has at most two roundings and no transcendental;
equality for ids, masks and counters; a sampled token by the interval test of tests/test_gpu_sampling.py (2e-6), after
which everything downstream of the token is exact given the token.  `err_kernel / max(err32, 2^-23 max|ref|)` (the bound
is 8) is printed per output by `pytest -m gpu -s` - the WORST lines of the file's last test; each test's docstring gives
what an MI355X measured (the largest of all: 2.36, the scan's alpha over 300 regions; no output needed a bound of its
own)."""
import ctypes as C
import functools

import pytest
import torch

import _fwd_ref as R
import _split_f16 as S16
from insenticap_model_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = R.SENTINEL
ISENT = -77                  # the sentinel of integer outputs
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def d(x):
    return None if x is None else x.to(DEV)


def sent(*shape, dtype=torch.float32):
    return torch.full(shape, SENT if dtype.is_floating_point else ISENT, device=DEV, dtype=dtype)


def off_by_one_float(x):
    """`x` on the device as a view that starts one float into its storage: not 16-byte aligned."""
    flat = torch.zeros(x.numel() + 4, device=DEV, dtype=x.dtype)
    v = flat[1:1 + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4
    return v


def plane_buffer(rows, K):
    """([2, rows, K] view handed to the kernel, the whole f16 buffer: one more row of sentinels behind the planes)"""
    flat = torch.full((2 * (rows + 1) * K,), SENT, device=DEV, dtype=torch.float16)
    return flat[:2 * rows * K].view(2, rows, K), flat


def check_planes(view, flat, out, name):
    """hi + lo reproduce `out` as tests/_split_f16.py defines the format, and the row behind the planes is untouched."""
    assert torch.equal(view.cpu(), S16.planes(out.cpu())), name
    assert bool((flat[view.numel():] == SENT).all()), name


# ------------------------------------------------------------------------------------------------ embeddings
@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('W', [4, 36, 260])
def test_embed_relu_fwd_bit_exact(W, B):
    """One wave per row, four rows per block (B = 5: three idle waves in block 1); W / 4 = 65 float4 is the lane loop's
    second trip.  ids contiguous and as a strided column of a [B, 3] tensor, add None and given, negative table entries,
    ids 0 and V - 1.  One max and one add: the bits of the fp32 torch expression.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8): out 0.47 (W = 260, B = 5, add; the
    float32 evaluation's own error: the same bits)"""
    g = gen(W * 10 + B)
    V = 11
    emb, add = rn(g, V, W), rn(g, B, W)
    ids3 = torch.randint(0, V, (B, 3), generator=g)
    ids3[0, 1], ids3[B - 1, 0] = V - 1, 0
    if B > 1:
        ids3[0, 0], ids3[1, 1] = V - 1, 0
    assert bool((emb < 0).any())
    ids3_d = ids3.to(DEV)
    for strided in (False, True):
        ids = ids3[:, 1] if strided else ids3[:, 0].contiguous()
        ids_d = ids3_d[:, 1] if strided else torch.tensor(ids.tolist(), device=DEV)
        assert ids_d.stride(0) == (3 if strided else 1) and {0, V - 1} & set(ids.tolist())
        for with_add in (False, True):
            buf = sent(B + 1, W)
            ops.embed_relu_fwd(d(emb), ids_d, buf[:B], add=d(add) if with_add else None)
            want = torch.relu(emb[ids]) + add if with_add else torch.relu(emb[ids])
            assert torch.equal(buf[:B].cpu(), want), (W, B, strided, with_add)
            ref, ev = R.both(R.embed_relu_ref, emb, ids, add=add if with_add else None)
            R.check_output(buf, ref['out'], ev['out'], 'fwd:embed_relu/out[W%d B%d col%d add%d]' % (W, B, strided, with_add))


def test_embed_relu_fwd_refuses_misaligned_pointers():
    """emb, out and add move as float4: a pointer that is not 16-byte aligned returns ISC_E_ALIGN in front of the launch
    (out keeps its sentinel); W % 4 != 0 stays ISC_E_SHAPE; the aligned call of the same shape runs."""
    lib, g = _lib.load(), gen(1)
    V, W, B = 11, 8, 3
    emb, add, ids = d(rn(g, V, W)), d(rn(g, B, W)), d(torch.tensor([0, 10, 4]))
    out = sent(B + 1, W)

    def rc_of(e, a, o, w=W):
        rc = lib.isc_embed_relu_fwd(e.data_ptr(), V, w, ids.data_ptr(), 1, ops.ptr(a), B, o.data_ptr(), ops.stream())
        torch.cuda.synchronize()
        return rc
    assert rc_of(off_by_one_float(emb), add, out) == E_ALIGN
    assert rc_of(emb, off_by_one_float(add), out) == E_ALIGN
    mis_out = off_by_one_float(sent(B, W))
    assert rc_of(emb, None, mis_out) == E_ALIGN and bool((mis_out == SENT).all())
    assert rc_of(emb, add, out, w=6) == E_SHAPE
    assert bool((out == SENT).all())
    assert rc_of(emb, None, out) == 0 and torch.equal(out[:B], torch.relu(emb[ids])) and bool((out[B] == SENT).all())


@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('C', [1, 8, 9, 17])
def test_embed_relu_mean_fwd_vs_fp64(C, B):
    """Eight words per chunk: C = 9 and 17 leave a last chunk of one, whose seven clamped loads must not be summed.
    W = 36 and 260 take the float4 path (260: the `i += 256` second trip), W = 6 the scalar path, W = 36 with the table
    one float into its storage the scalar path through misalignment.  Every row repeats an id.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    out 1.00 (C = 9, B = 1, W = 260: the float32 evaluation's own error - the kernel sums in the same order)"""
    g = gen(C * 10 + B)
    V = 11
    for W, misaligned in ((36, False), (260, False), (6, False), (36, True)):
        emb = rn(g, V, W)
        ids = torch.randint(0, V, (B, C), generator=g)
        if C > 1:
            ids[:, C // 2] = ids[:, 0]
        emb_d = off_by_one_float(emb) if misaligned else d(emb)
        buf = sent(B + 1, W)
        ops.embed_relu_mean_fwd(emb_d, d(ids), buf[:B])
        ref, ev = R.both(R.embed_relu_mean_ref, emb, ids)
        R.check_output(buf, ref['out'], ev['out'], 'fwd:embed_relu_mean/out[C%d B%d W%d mis%d]' % (C, B, W, misaligned))


@pytest.mark.parametrize('W', [6, 36, 100])
@pytest.mark.parametrize('B,n_words', [(1, 1), (3, 5)])
def test_embed_senti_words_fwd_vs_fp64(B, n_words, W):
    """Rows b (n_words + 1) + m, four per block: (3, 5) gives 18 rows.  Slot 0 is the row of pad_id = 2 (positive
    entries, so the slot differs from every other id's and from id 0's); the uint8 mask times scale = 2.  Without a mask
    the bits of torch's relu; with it two exact multiplications.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8): out 0.00 in every case"""
    g = gen(B * 100 + W)
    V, pad_id = 11, 2
    emb = rn(g, V, W)
    emb[pad_id] = emb[pad_id].abs() + 0.5
    ids = torch.randint(0, V, (B, n_words), generator=g)
    rows = B * (n_words + 1)
    mask = (torch.rand(B, n_words + 1, W, generator=g) > 0.4).to(torch.uint8)
    for with_mask in (False, True):
        buf = sent(rows + 1, W)
        ops.embed_senti_words_fwd(d(emb), d(ids), pad_id, buf[:rows], keep_mask=d(mask) if with_mask else None,
                                  mask_scale=2.0 if with_mask else 1.0)
        kw = dict(keep_mask=mask, mask_scale=2.0) if with_mask else {}
        ref, ev = R.both(R.embed_senti_words_ref, emb, ids, pad_id, **kw)
        assert torch.equal(buf[:rows].cpu(), ev['out'].reshape(rows, W)), (B, n_words, W, with_mask)
        R.check_output(buf, ref['out'].reshape(rows, W), ev['out'].reshape(rows, W),
                       'fwd:embed_senti_words/out[B%d n%d W%d mask%d]' % (B, n_words, W, with_mask))


# ------------------------------------------------------------------------------------------------ gate mix
# (B, A, D, z one float into its storage, w_bias, beta_out: 'col' = a strided column / 'row' = contiguous / None, planes)
GATE_CASES = [
    (1, 4, 4, False, False, 'row', False),
    (5, 36, 100, False, True, 'col', False),
    (3, 6, 10, False, True, 'row', False),           # both scalar paths
    (6, 516, 36, False, False, 'col', False),        # A / 4 = 129: three trips
    (5, 36, 100, True, True, 'row', False),          # scalar A path through misalignment, vector D path
    (3, 36, 64, False, True, None, True),            # planes of out (the format needs D % 32 == 0); beta_out null
]


@pytest.mark.parametrize('B,A,D,z_off,with_bias,beta_kind,with_planes', GATE_CASES)
def test_gate_mix_fwd_vs_fp64(B, A, D, z_off, with_bias, beta_kind, with_planes):
    """beta = sigmoid(w . tanh(z) + bias), out = beta v + (1 - beta) s with A != D.  The last row of every case with
    B > 1 has |z| of 30 ... 100, where tanh saturates to +-1 (exp overflows in the kernel's form): finite, and the bound
    holds.  beta_out as column 1 of a [B + 1, 3] buffer: columns 0 and 2 and the row behind keep their sentinel.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    beta 1.22, out 1.14 (both at 6 x 516 x 36)"""
    g = gen(B * 1000 + A + D + int(z_off))
    z, w, v, s = rn(g, B, A), rn(g, A, scale=0.3), rn(g, B, D), rn(g, B, D)
    bias = torch.tensor([0.7]) if with_bias else None
    if B > 1:
        z[B - 1] = (torch.rand(A, generator=g) * 70 + 30) * torch.where(torch.rand(A, generator=g) > 0.5, 1.0, -1.0)
    z_d = off_by_one_float(z) if z_off else d(z)
    out_buf = sent(B + 1, D)
    beta_buf = sent(B + 1, 3) if beta_kind == 'col' else sent(B + 1)
    beta = None if beta_kind is None else (beta_buf[:B, 1] if beta_kind == 'col' else beta_buf[:B])
    pl_view, pl_flat = plane_buffer(B, D) if with_planes else (None, None)
    ops.gate_mix_fwd(z_d, d(w), d(bias), d(v), d(s), out_buf[:B], beta_out=beta, out_planes=pl_view)
    ref, ev = R.both(R.gate_mix_ref, z, w, bias, v, s)
    tag = '[%dx%dx%d off%d bias%d %s]' % (B, A, D, z_off, with_bias, beta_kind)
    R.check_output(out_buf, ref['out'], ev['out'], 'fwd:gate_mix/out' + tag)
    if beta_kind == 'col':
        assert beta.stride(0) == 3
        R.check_output(beta_buf[:, 1], ref['beta'], ev['beta'], 'fwd:gate_mix/beta' + tag, pad='sentinel')
        assert bool((beta_buf[:, [0, 2]] == SENT).all())
    elif beta_kind == 'row':
        R.check_output(beta_buf, ref['beta'], ev['beta'], 'fwd:gate_mix/beta' + tag, pad='sentinel')
    if with_planes:
        check_planes(pl_view, pl_flat, out_buf[:B], tag)


def test_gate_mix_fwd_refuses_before_the_launch():
    """v one float into its storage with D % 4 == 0 -> ISC_E_ALIGN; out_hi without out_lo -> ISC_E_NULL; out and beta
    keep their sentinel; the same call with both fixed runs."""
    lib, g = _lib.load(), gen(2)
    B, A, D = 3, 8, 32
    z, w, v, s = d(rn(g, B, A)), d(rn(g, A)), d(rn(g, B, D)), d(rn(g, B, D))
    out, beta = sent(B, D), sent(B)
    pl_view, _ = plane_buffer(B, D)

    def rc_of(v_, hi, lo):
        rc = lib.isc_gate_mix_fwd(z.data_ptr(), w.data_ptr(), None, v_.data_ptr(), s.data_ptr(), B, A, D, out.data_ptr(),
                                  beta.data_ptr(), 1, hi, lo, ops.stream())
        torch.cuda.synchronize()
        return rc
    hi, lo = ops.planes_ptrs(pl_view)
    assert rc_of(off_by_one_float(v), hi, lo) == E_ALIGN
    assert rc_of(v, hi, None) == E_NULL
    assert bool((out == SENT).all()) and bool((beta == SENT).all()) and bool((pl_view == SENT).all())
    assert rc_of(v, hi, lo) == 0 and not bool((out == SENT).any())


# ------------------------------------------------------------------------------------------------ attention scan
def _scan_inputs(g, B, R_, A, D, with_q2, with_bias, n_table=0):
    """Per-row P / V, or (n_table > 0) tables with row_ids [B, R] (repeats) in a [B, R + 2] tensor."""
    x = dict(q=rn(g, B, A), w=rn(g, A, scale=0.3), q2=rn(g, B, A) if with_q2 else None,
             bias=torch.tensor([0.4]) if with_bias else None, ids=None)
    if n_table:
        x['P'], x['V'] = rn(g, n_table, A), rn(g, n_table, D)
        ids = torch.randint(0, n_table, (B, R_ + 2), generator=g)
        ids[:, 1] = ids[:, 0]
        x['ids_wide'], x['ids'] = ids, ids[:, :R_]
    else:
        x['P'], x['V'] = rn(g, B, R_, A), rn(g, B, R_, D)
    return x


def _scan_problem(x, rows_alloc, with_planes=False, alpha_extra=3):
    """The problem and its buffers: out [rows_alloc, D], alpha [rows_alloc, R + alpha_extra], planes - all sentinels."""
    B, A = x['q'].shape
    D = x['V'].shape[-1]
    R_ = x['ids'].shape[1] if x['ids'] is not None else x['P'].shape[1]
    out_buf, alpha_buf = sent(rows_alloc, D), sent(rows_alloc, R_ + alpha_extra)
    pl_view, pl_flat = plane_buffer(B, D) if with_planes else (None, None)
    ids_d = None if x['ids'] is None else x['ids_wide'].to(DEV)[:, :R_]
    xd = {k: d(x[k]) for k in ('P', 'V', 'q', 'w', 'bias', 'q2')}      # (the problem holds bare pointers: kept alive)
    prob = ops.scan_problem(xd['P'], xd['V'], xd['q'], xd['w'], xd['bias'], out_buf[:B],
                            alpha_out=alpha_buf[:B, :R_], q2=xd['q2'], out_planes=pl_view, row_ids=ids_d)
    assert prob.alpha_ld == R_ + alpha_extra and (ids_d is None or prob.row_ids_ld == R_ + 2)
    return prob, dict(out=out_buf, alpha=alpha_buf, planes=(pl_view, pl_flat), dev=xd, ids_d=ids_d)


def _scan_check(x, bufs, tag, B):
    ref, ev = R.both(R.scan_fwd_ref, x['P'], x['V'], x['q'], x['w'], w_bias=x['bias'], q2=x['q2'], row_ids=x['ids'])
    R.check_output(bufs['alpha'], ref['alpha'], ev['alpha'], 'fwd:attn_scan/alpha' + tag, pad='sentinel')
    R.check_output(bufs['out'], ref['out'], ev['out'], 'fwd:attn_scan/out' + tag)
    if bufs['planes'][0] is not None:
        check_planes(bufs['planes'][0], bufs['planes'][1], bufs['out'][:B], tag)


# (B, R, A, D, q2, w_bias, planes, alpha_ld - R)
SCAN_CASES = [
    (1, 1, 4, 4, False, False, False, 0),
    (3, 13, 36, 96, True, True, True, 3),            # the r0 += 12 tail; nd4 = 24: ngrp = 10, sixteen idle threads
    (2, 7, 260, 36, False, True, False, 3),          # NA = 2, nd4 = 9
    (2, 5, 1024, 1028, True, False, False, 3),       # NA = 4 and the nd4 > 256 branch
    (2, 300, 32, 32, True, True, True, 3),           # R > 256: the alpha loop's second trip
]


@pytest.mark.parametrize('B,R_,A,D,with_q2,with_bias,with_planes,alpha_extra', SCAN_CASES)
def test_attn_scan_fwd_vs_fp64(B, R_, A, D, with_q2, with_bias, with_planes, alpha_extra):
    """alpha = softmax_r(w . tanh(P + q (+ q2)) + bias), out = alpha V with A != D, one problem per launch.  alpha_out is
    a [B, R] view of rows R + 3 wide (columns R.. and the row behind keep their sentinel); out_planes where D % 32 == 0.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    alpha 2.36 (2 x 300 x 32 x 32), out 2.21 (2 x 5 x 1024 x 1028)"""
    g = gen(B * 1000 + R_ + A + D)
    x = _scan_inputs(g, B, R_, A, D, with_q2, with_bias)
    prob, bufs = _scan_problem(x, B + 1, with_planes, alpha_extra)
    ops.attn_scan_fwd([prob], B)
    _scan_check(x, bufs, '[%dx%dx%dx%d q2=%d bias=%d]' % (B, R_, A, D, with_q2, with_bias), B)


def test_attn_scan_fwd_gather_mode_vs_fp64():
    """Tables of 9 rows, row_ids [3, 6] with repeats as a view of a [3, 8] tensor, A = 32, D = 64: region r of row b is
    table row row_ids[b, r] for the scores AND for the weighted sum.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8): alpha 0.71, out 0.87"""
    g = gen(9)
    x = _scan_inputs(g, 3, 6, 32, 64, True, True, n_table=9)
    assert x['ids'].unique().numel() > 3 and bool((x['ids'] != torch.arange(6)).any())
    prob, bufs = _scan_problem(x, 4, with_planes=True)
    ops.attn_scan_fwd([prob], 3)
    _scan_check(x, bufs, '[gather 3x6x32x64]', 3)


def test_attn_scan_fwd_two_problem_launch():
    """One launch of two problems, rows = 5 and rows = 3, A = 32 and 516 (both run at NA = 4), different R and D: the grid
    spans 5 rows, so rows 3 and 4 of the shorter problem's out and alpha must keep their sentinel.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    alpha 1.38, out 1.07 (both in the five-row problem)"""
    g = gen(10)
    shapes = [(5, 6, 32, 96), (3, 9, 516, 20)]
    probs, keep = [], []
    for rows, R_, A, D in shapes:
        x = _scan_inputs(g, rows, R_, A, D, with_q2=rows == 3, with_bias=rows == 5)
        prob, bufs = _scan_problem(x, 5 + 1)
        assert isinstance(prob, _lib.ScanProblem)
        prob.rows = rows
        probs.append(prob)
        keep.append((x, bufs))
    ops.attn_scan_fwd(probs, 5)
    for i, (x, bufs) in enumerate(keep):
        assert bufs['out'].shape[0] == 6 and bufs['alpha'].shape[0] == 6
        _scan_check(x, bufs, '[two problems: %d rows%d]' % (i, shapes[i][0]), shapes[i][0])
    assert bool((keep[1][1]['out'][3:] == SENT).all()) and bool((keep[1][1]['alpha'][3:] == SENT).all())


def test_attn_scan_fwd_refuses_what_it_cannot_run():
    """A = 1028 (> 1024), A % 4 != 0, and R = 15000 at A = D = 4 (the scores and the 256 partial rows need
    (15000 + 1024) * 4 bytes of LDS > 60000) return ISC_E_SHAPE from the entry point's checks; nothing is written."""
    lib, g = _lib.load(), gen(11)

    def rc_of(B, R_, A, D):
        x = _scan_inputs(g, B, R_, A, D, False, False)
        prob, bufs = _scan_problem(x, B + 1)
        rc = lib.isc_attn_scan_fwd((_lib.ScanProblem * 1)(prob), 1, B, ops.stream())
        torch.cuda.synchronize()
        if rc != 0:
            assert bool((bufs['out'] == SENT).all()) and bool((bufs['alpha'] == SENT).all())
        return rc
    assert rc_of(1, 2, 1028, 4) == E_SHAPE
    assert rc_of(1, 2, 6, 4) == E_SHAPE
    assert (15000 + 3 + 256 * 4) * 4 > 60000
    assert rc_of(1, 15000, 4, 4) == E_SHAPE
    assert rc_of(1, 2, 8, 4) == 0


# ------------------------------------------------------------------------------------------------ log-softmax
def _logit_rows(g, M, V):
    """Rows shifted by +80, -80, 0, ...; for V > 128 row 0 has its maximum in the last tile, row 1 in tile 0."""
    x = rn(g, M, V, scale=2.0)
    if V > 128:
        x[0, V - 1] = 9.0
        if M > 1:
            x[1, 3] = 9.0
    for m in range(M):
        x[m] += (80.0, -80.0, 0.0)[m % 3]
    return x


@pytest.mark.parametrize('M,V,ld,with_lse', [(1, 1, 1, True), (3, 130, 136, False), (2, 2049, 2049, True),
                                             (2, 8321, 8321, True)])
def test_logsoftmax_apply_vs_fp64_from_host_statistics(M, V, ld, with_lse):
    """logp = (x - gmax) - log S in place from host-made tile statistics.  V = 2049: a second grid column of one element;
    V = 8321: 66 tiles, more than the 64 lanes that fold them, with the row maximum in tile 65 (row 0) and tile 0 (row
    1).  Rows around +80 and -80.  Columns V .. ld - 1 and the row behind keep their sentinel; lse_out null and given.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    logp 0.46 (3 x 130), lse 0.35 (2 x 2049)"""
    g = gen(V)
    x = _logit_rows(g, M, V)
    pm, ps, _ = R.tile_stats(x)
    if V == 8321:
        assert pm.shape[1] == 66 and int(pm[0].argmax()) == 65 and int(pm[1].argmax()) == 0
    buf = sent(M + 1, ld)
    buf[:M, :V] = x.to(DEV)
    lse_buf = sent(M + 1)
    ops.logsoftmax_apply(buf[:M, :V], d(pm), d(ps), lse_out=lse_buf[:M] if with_lse else None)
    ref, ev = R.both(R.logp_from_stats_ref, x, pm, ps)
    tag = '[%dx%d ld%d]' % (M, V, ld)
    R.check_output(buf, ref['logp'], ev['logp'], 'fwd:logsoftmax_apply/logp' + tag, pad='sentinel')
    if with_lse:
        R.check_output(lse_buf, ref['lse'], ev['lse'], 'fwd:logsoftmax_apply/lse' + tag, pad='sentinel')
    else:
        assert bool((lse_buf == SENT).all())


@pytest.mark.parametrize('variant', ['in_place', 'from_src', 'step_rows'])
def test_logsoftmax_apply_steps_vs_fp64(variant):
    """B = 3, T = 4, V = 130; logits is the [B, T, V] slice of a [B + 1, T, V + 6] buffer (ld_t = V + 6, the six columns
    and the last batch row keep their sentinel).  in place; from src [T, B, V]; step_rows = 5 with the statistics and src
    as views that start at row 2 of each step's five - rows 0 and 1 hold another branch's data.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    logp 0.53 (in place)"""
    g = gen(12)
    B, T, V, SR = 3, 4, 130, 5
    x_all = _logit_rows(g, T * SR, V).reshape(T, SR, V)               # rows of both branches, step by step
    pm_all, ps_all, _ = R.tile_stats(x_all.reshape(T * SR, V))
    nt = pm_all.shape[1]
    pm_all, ps_all = pm_all.reshape(T, SR, nt), ps_all.reshape(T, SR, nt)
    x, pm, ps = x_all[:, 2:], pm_all[:, 2:], ps_all[:, 2:]            # this branch: [T, B, .]
    buf = sent(B + 1, T, V + 6)
    logits = buf[:B, :, :V]
    if variant == 'in_place':
        logits.copy_(x.transpose(0, 1))
        ops.logsoftmax_apply_steps(logits, d(pm.contiguous()), d(ps.contiguous()))
    elif variant == 'from_src':
        ops.logsoftmax_apply_steps(logits, d(pm.contiguous()), d(ps.contiguous()), src_tbv=d(x.contiguous()))
    else:
        pm_d, ps_d, x_d = d(pm_all)[:, 2:], d(ps_all)[:, 2:], d(x_all)[:, 2:]
        assert pm_d.stride(0) == SR * nt and x_d.stride(0) == SR * V and not bool((x_all[:, :2] == x_all[:, 2:4]).any())
        ops.logsoftmax_apply_steps(logits, pm_d, ps_d, src_tbv=x_d, step_rows=SR)
    ref, ev = R.both(R.logp_from_stats_ref, x.reshape(T * B, V), pm.reshape(T * B, nt), ps.reshape(T * B, nt))
    to_btv = lambda y: y.reshape(T, B, V).transpose(0, 1).reshape(B * T, V)   # noqa: E731  (row (b, t) of the output)
    R.check_output(buf.view((B + 1) * T, V + 6), to_btv(ref['logp']), to_btv(ev['logp']),
                   'fwd:logsoftmax_apply_steps/logp[%s]' % variant, pad='sentinel')


def test_logsoftmax_apply_steps_refuses_fewer_step_rows_than_rows():
    """step_rows = 2 < B = 3 -> ISC_E_SHAPE from the entry point; the logits keep their bits."""
    g = gen(13)
    B, T, V = 3, 4, 130
    x = rn(g, T * B, V)
    pm, ps, _ = R.tile_stats(x)
    logits = d(x.reshape(T, B, V).transpose(0, 1).contiguous())
    before = logits.clone()
    rc = _lib.load().isc_logsoftmax_apply_steps(logits.data_ptr(), T * V, V, B, T, V, d(pm).data_ptr(), d(ps).data_ptr(),
                                                None, 2, ops.stream())
    torch.cuda.synchronize()
    assert rc == E_SHAPE and torch.equal(logits, before)


# ------------------------------------------------------------------------------------------------ roll-out step
ROLL_T, ROLL_t = 3, 1


@functools.lru_cache(maxsize=None)
def _roll_inputs(B, V):
    """Logits, host-made statistics and the row states of one roll-out step, made once per (B, V) and left unchanged.
    <EOS> = 5: rows b % 5 == 0 put all their mass on it (drawn whatever the mode; rows 0 and 10 are live, row 5 is
    finished); row 1's maximum stands at ids 7 and 129 - two tiles - with the same value; rows b % 3 == 2 are finished."""
    g = gen(B * 7 + V)
    eos = 5
    x = rn(g, B, V, scale=2.0)
    b = torch.arange(B)
    x[b % 5 == 0, eos] = 40.0
    x[1, [7, 129]] = 21.0
    unf = (b % 3 != 2).to(torch.int32)
    forced = torch.randint(0, V, (B, ROLL_T), generator=g)
    forced[b % 5 == 0, ROLL_t] = eos
    forced[1, ROLL_t], forced[3 % B, ROLL_t] = V - 1, 0
    u = torch.rand(B, ROLL_T, generator=g) * 0.98 + 0.01
    return dict(x=x, stats=R.tile_stats(x), unf=unf, eos=eos, forced=forced, u=u)


@pytest.mark.parametrize('mode', ['greedy', 'forced', 'sampled'])
@pytest.mark.parametrize('B,V,W', [(6, 130, 4), (6, 8321, 260), (1030, 130, 260), (1030, 8321, 4)])
def test_rollout_finalize_vs_the_state_machine(B, V, W, mode):
    """Step t = 1 of T = 3 in the three modes (greedy runs with logits = NULL).  B = 1030 takes the wide kernel, sixteen
    rows per block with six in the last; V = 8321 folds 66 tiles; W = 260 is the xt_next loop's second trip; xt_add is
    given where W = 4.  Tokens (greedy, forced), masks, raw_tokens, unfinished and alive[t + 1] are exact; a sampled
    token passes the interval test and everything behind it is exact given the token; seq_logprobs and xt_next by the
    rule.  Columns 0 and 2 of every [B, T] output, alive[0], alive[t] and alive[3], unfinished[B] and the row behind
    xt_next keep what they held.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    seq_logprobs 1.01 (greedy, B = 1030, V = 8321), xt_next 0.42 (the float32 evaluation's own bits)"""
    c = _roll_inputs(B, V)
    g = gen(B + V + W)
    T, t = ROLL_T, ROLL_t
    pm, ps, pi = c['stats']
    emb = rn(g, V, W)
    add = rn(g, B, W) if W == 4 else None
    xbuf = torch.zeros(B, V + 3)
    xbuf[:, :V] = c['x']
    x_d = xbuf.to(DEV)
    seq, raw = sent(B, T, dtype=torch.int64), sent(B, T, dtype=torch.int64)
    lp, mk = sent(B, T), sent(B, T)
    unf = sent(B + 1, dtype=torch.int32)
    unf[:B] = c['unf'].to(DEV)
    n_live = int(c['unf'].sum())
    alive = torch.tensor([ISENT, n_live, 0, ISENT], dtype=torch.int32, device=DEV)
    xt = sent(B + 1, W)
    keep = [d(pm), d(ps), d(pi), d(emb), d(add), d(c['forced']), d(c['u'])]
    st = _lib.RolloutStep()
    st.B, st.V, st.T, st.t, st.n_tile, st.W = B, V, T, t, pm.shape[1], W
    st.part_max, st.part_sum, st.part_idx = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()
    st.logits, st.ld_logits = (None if mode == 'greedy' else x_d.data_ptr()), V + 3
    st.forced = keep[5].data_ptr() if mode == 'forced' else None
    st.sample_u = keep[6].data_ptr() if mode == 'sampled' else None
    st.eos_id = c['eos']
    st.seq, st.seq_logprobs, st.seq_masks = seq.data_ptr(), lp.data_ptr(), mk.data_ptr()
    st.unfinished, st.alive, st.raw_tokens = unf.data_ptr(), alive.data_ptr(), raw.data_ptr()
    st.emb, st.xt_add, st.xt_next = keep[3].data_ptr(), ops.ptr(keep[4]), xt.data_ptr()
    ops.rollout_finalize(st)
    torch.cuda.synchronize()

    kw = {}
    if mode == 'forced':
        kw = dict(forced=c['forced'][:, t])
    elif mode == 'sampled':
        tok = raw[:, t].cpu()
        R.check_sample_interval(c['x'], c['u'][:, t], tok, 'rollout/sampled token')
        kw = dict(tokens=tok)
    ref, ev = R.both(R.rollout_finalize_ref, c['x'], pm, ps, pi, c['unf'], c['eos'], emb, xt_add=add, mode=mode, **kw)
    tag = '[%s B%d V%d W%d]' % (mode, B, V, W)
    R.check_exact(raw[:, t], ref['raw_tokens'], 'rollout/raw_tokens' + tag)
    R.check_exact(seq[:, t], ref['seq'], 'rollout/seq' + tag)
    R.check_exact(mk[:, t], ref['seq_masks'], 'rollout/seq_masks' + tag)
    R.check_exact(unf[:B], ref['unfinished'], 'rollout/unfinished' + tag)
    assert alive.tolist() == [ISENT, n_live, int(ref['alive_next']), ISENT] and int(unf[B]) == ISENT
    R.check_output(lp[:, t], ref['seq_logprobs'], ev['seq_logprobs'], 'fwd:rollout_finalize/seq_logprobs' + tag)
    R.check_output(xt, ref['xt_next'], ev['xt_next'], 'fwd:rollout_finalize/xt_next' + tag)
    for o in (seq, raw):
        assert bool((o[:, [0, 2]] == ISENT).all())
    for o in (lp, mk):
        assert bool((o[:, [0, 2]] == SENT).all())
    # what the case is there for: <EOS> drawn by live and by finished rows, the tie, a finished row's masked token
    eos_rows = ref['raw_tokens'] == c['eos']
    assert bool((eos_rows & (c['unf'] != 0)).any()) and bool((eos_rows & (c['unf'] == 0)).any())
    assert int(ref['alive_next']) < n_live and bool((ref['raw_tokens'][c['unf'] == 0] != 0).any())
    if mode == 'greedy':
        assert int(raw[1, t]) == 7


def test_rollout_finalize_writes_nothing_once_no_row_is_alive():
    """alive[t] == 0: the reference's early `break` - every output, alive[t + 1] and unfinished included, keeps what it
    held."""
    c = _roll_inputs(6, 130)
    B, V, W, T, t = 6, 130, 4, ROLL_T, ROLL_t
    pm, ps, pi = [d(s) for s in c['stats']]
    emb = d(rn(gen(3), V, W))
    seq, raw, lp, mk = sent(B, T, dtype=torch.int64), sent(B, T, dtype=torch.int64), sent(B, T), sent(B, T)
    unf, xt = sent(B, dtype=torch.int32), sent(B, W)
    alive = torch.tensor([ISENT, 0, ISENT, ISENT], dtype=torch.int32, device=DEV)
    st = _lib.RolloutStep()
    st.B, st.V, st.T, st.t, st.n_tile, st.W = B, V, T, t, pm.shape[1], W
    st.part_max, st.part_sum, st.part_idx = pm.data_ptr(), ps.data_ptr(), pi.data_ptr()
    st.eos_id = c['eos']
    st.seq, st.seq_logprobs, st.seq_masks = seq.data_ptr(), lp.data_ptr(), mk.data_ptr()
    st.unfinished, st.alive, st.raw_tokens = unf.data_ptr(), alive.data_ptr(), raw.data_ptr()
    st.emb, st.xt_next = emb.data_ptr(), xt.data_ptr()
    ops.rollout_finalize(st)
    torch.cuda.synchronize()
    assert all(bool((o == ISENT).all()) for o in (seq, raw, unf)) and all(bool((o == SENT).all()) for o in (lp, mk, xt))
    assert alive.tolist() == [ISENT, 0, ISENT, ISENT]


def test_rollout_finalize_refuses_misaligned_pointers():
    """With xt_next set, emb, xt_add and xt_next move as float4: one of them one float into its storage returns
    ISC_E_ALIGN in front of the launch and every output keeps its sentinel.  Without xt_next none of the three is read:
    the misaligned table is accepted and the step runs."""
    lib = _lib.load()
    c = _roll_inputs(6, 130)
    B, V, W, T, t = 6, 130, 4, ROLL_T, ROLL_t
    pm, ps, pi = [d(s) for s in c['stats']]
    g = gen(4)
    emb, add = d(rn(g, V, W)), d(rn(g, B, W))
    emb_off, add_off, xt_off = off_by_one_float(emb), off_by_one_float(add), off_by_one_float(sent(B, W))

    def rc_of(emb_, add_, xt_):
        seq, lp, mk = sent(B, T, dtype=torch.int64), sent(B, T), sent(B, T)
        unf = d(c['unf'].clone())
        alive = torch.tensor([ISENT, int(c['unf'].sum()), 0, ISENT], dtype=torch.int32, device=DEV)
        st = _lib.RolloutStep()
        st.B, st.V, st.T, st.t, st.n_tile, st.W = B, V, T, t, pm.shape[1], W
        st.part_max, st.part_sum, st.part_idx = pm.data_ptr(), ps.data_ptr(), pi.data_ptr()
        st.eos_id = c['eos']
        st.seq, st.seq_logprobs, st.seq_masks = seq.data_ptr(), lp.data_ptr(), mk.data_ptr()
        st.unfinished, st.alive = unf.data_ptr(), alive.data_ptr()
        st.emb, st.xt_add, st.xt_next = emb_.data_ptr(), ops.ptr(add_), ops.ptr(xt_)
        rc = lib.isc_rollout_finalize(C.byref(st), ops.stream())
        torch.cuda.synchronize()
        untouched = (bool((seq == ISENT).all()) and bool((lp == SENT).all()) and bool((mk == SENT).all())
                     and torch.equal(unf.cpu(), c['unf']) and int(alive[2]) == 0
                     and (xt_ is None or bool((xt_ == SENT).all())))
        return rc, untouched
    xt = sent(B, W)
    assert rc_of(emb_off, add, xt) == (E_ALIGN, True)
    assert rc_of(emb, add_off, xt) == (E_ALIGN, True)
    assert rc_of(emb, add, xt_off) == (E_ALIGN, True)
    assert rc_of(emb_off, None, None) == (0, False)
    assert rc_of(emb, add, xt) == (0, False)


@pytest.mark.parametrize('entry', ['filtered', 'constrained', 'constrained_filtered'])
def test_filtered_and_constrained_finalize_refuse_misaligned_pointers(entry):
    """The same refusal at the other two entry points: their kernels move emb, xt_add and xt_next as float4 through the
    same commit stage.  One of the three placed one float into its storage returns ISC_E_ALIGN, every output keeps its
    sentinel and the launch counter does not move - nothing is launched.  The aligned call is accepted."""
    lib = _lib.load()
    c = _roll_inputs(6, 130)
    B, V, W, T, t = 6, 130, 4, ROLL_T, ROLL_t
    pm, ps, pi = [d(s) for s in c['stats']]
    g = gen(5)
    emb, add, x_d, u_d = d(rn(g, V, W)), d(rn(g, B, W)), d(c['x']), d(c['u'])
    emb_off, add_off, xt_off = off_by_one_float(emb), off_by_one_float(add), off_by_one_float(sent(B, W))
    f = _lib.SampleFilter()
    f.temperature, f.top_k, f.top_p = 0.8, 50, 0.9
    cons = ops.decode_constraints([0, 1, 3], False, 0, 0)

    def rc_of(emb_, add_, xt_):
        seq, raw, lp, mk = sent(B, T, dtype=torch.int64), sent(B, T, dtype=torch.int64), sent(B, T), sent(B, T)
        slp = sent(B, T)
        unf = d(c['unf'].clone())
        alive = torch.tensor([ISENT, int(c['unf'].sum()), 0, ISENT], dtype=torch.int32, device=DEV)
        st = _lib.RolloutStep()
        st.B, st.V, st.T, st.t, st.n_tile, st.W = B, V, T, t, pm.shape[1], W
        st.part_max, st.part_sum, st.part_idx = pm.data_ptr(), ps.data_ptr(), pi.data_ptr()
        st.logits, st.ld_logits, st.sample_u, st.eos_id = x_d.data_ptr(), V, u_d.data_ptr(), c['eos']
        st.seq, st.seq_logprobs, st.seq_masks = seq.data_ptr(), lp.data_ptr(), mk.data_ptr()
        st.unfinished, st.alive, st.raw_tokens = unf.data_ptr(), alive.data_ptr(), raw.data_ptr()
        st.emb, st.xt_add, st.xt_next = emb_.data_ptr(), ops.ptr(add_), ops.ptr(xt_)
        f.sampling_logprobs = slp.data_ptr()
        n0 = lib.isc_rollout_finalize_launches()
        if entry == 'filtered':
            rc = lib.isc_rollout_finalize_filtered(C.byref(st), C.byref(f), ops.stream())
        else:
            rc = lib.isc_rollout_finalize_constrained(C.byref(st), C.byref(f) if entry == 'constrained_filtered' else None,
                                                      C.byref(cons), ops.stream())
        torch.cuda.synchronize()
        untouched = (all(bool((o == ISENT).all()) for o in (seq, raw))
                     and all(bool((o == SENT).all()) for o in (lp, mk, slp, xt_))
                     and torch.equal(unf.cpu(), c['unf']) and int(alive[2]) == 0)
        return rc, untouched, lib.isc_rollout_finalize_launches() - n0
    xt = sent(B, W)
    assert rc_of(emb_off, add, xt) == (E_ALIGN, True, 0)
    assert rc_of(emb, add_off, xt) == (E_ALIGN, True, 0)
    assert rc_of(emb, add, xt_off) == (E_ALIGN, True, 0)
    assert rc_of(emb, add, xt) == (0, False, 1)


# ------------------------------------------------------------------------------------------------ scheduled sampling
@pytest.mark.parametrize('ss_prob', [0.0, 1.0, 0.4])
@pytest.mark.parametrize('V', [300, 8321])
def test_sched_sample_raw_draws_from_the_raw_logits(V, ss_prob):
    """M = 9 (three blocks, one wave in the last), logits rows V + 5 apart, base_ids a strided column.  ss_prob = 0: every
    row keeps its base id; 1: every row is drawn; 0.4: both kinds.  A drawn row's token passes the interval test against
    the fp64 softmax of its raw logits; an undrawn row is exact; the element behind out_ids keeps its sentinel."""
    g = gen(V)
    M = 9
    x = _logit_rows(g, M, V)
    pm, ps, pi = R.tile_stats(x)
    xbuf = torch.zeros(M, V + 5)
    xbuf[:, :V] = x
    x_d = xbuf.to(DEV)[:, :V]
    caps = torch.randint(0, V, (M, 7), generator=g)
    caps_d = caps.to(DEV)
    u_sel, u_draw = torch.rand(M, generator=g), torch.rand(M, generator=g) * 0.98 + 0.01
    u_sel[0], u_sel[1] = 0.1, 0.9
    out = sent(M + 1, dtype=torch.int64)
    assert x_d.stride(0) == V + 5 and caps_d[:, 3].stride(0) == 7
    ops.sched_sample(x_d, d(pm), d(ps), d(pi), d(u_sel), d(u_draw), ss_prob, caps_d[:, 3], out[:M], raw=True)
    torch.cuda.synchronize()
    sel = u_sel < ss_prob
    assert {0.0: not bool(sel.any()), 1.0: bool(sel.all()), 0.4: bool(sel.any()) and not bool(sel.all())}[ss_prob]
    got = out[:M].cpu()
    R.check_exact(got[~sel], caps[:, 3][~sel], 'sched_sample_raw/undrawn rows')
    if bool(sel.any()):
        tok = torch.where(sel, got, torch.zeros_like(got))
        R.check_sample_interval(x, u_draw, tok, 'sched_sample_raw/drawn rows', rows=sel.numpy())
    assert int(out[M]) == ISENT


# ------------------------------------------------------------------------------------------------ beam state gather
@pytest.mark.parametrize('H', [4, 1028])
def test_beam_gather_equals_an_index_of_the_concatenation(H):
    """planes = 4, rows = 5; H / 4 = 257 float4 is the copy loop's second trip; gather mixes entries < rows (the next
    state) and >= rows (the current one).  A copy: torch.equal; the row behind `out` keeps its sentinel."""
    g = gen(H)
    planes, rows = 4, 5
    nxt, cur = rn(g, planes, rows, H), rn(g, planes, rows, H)
    gather = torch.tensor([7, 0, 9, 4, 5])
    buf = sent(planes * rows + 1, H)
    ops.beam_gather(d(nxt), d(cur), d(gather), buf[:planes * rows].view(planes, rows, H))
    want = torch.cat([nxt, cur], dim=1)[:, gather]
    assert torch.equal(buf[:planes * rows].cpu().view(planes, rows, H), want)
    assert bool((buf[planes * rows] == SENT).all())


def test_beam_gather_refuses_before_the_launch():
    """H = 6 -> ISC_E_SHAPE; `out` one float into its storage -> ISC_E_ALIGN; nothing is written."""
    lib, g = _lib.load(), gen(6)
    planes, rows = 4, 5
    gather = d(torch.tensor([7, 0, 9, 4, 5]))

    def rc_of(H, out):
        nxt, cur = d(rn(g, planes, rows, H)), d(rn(g, planes, rows, H))
        rc = lib.isc_beam_gather(nxt.data_ptr(), cur.data_ptr(), gather.data_ptr(), out.data_ptr(), planes, rows, H,
                                 ops.stream())
        torch.cuda.synchronize()
        return rc
    out = sent(planes * rows, 8)
    assert rc_of(6, out) == E_SHAPE and bool((out == SENT).all())
    out_off = off_by_one_float(sent(planes * rows, 8))
    assert rc_of(8, out_off) == E_ALIGN and bool((out_off == SENT).all())
    assert rc_of(8, out) == 0 and not bool((out == SENT).any())


def test_zz_report_the_measured_ratios():
    """Prints err_kernel / err32 of every output this file measured (pytest -s): the table of the file's docstrings."""
    mine = {k: v for k, v in R.WORST.items() if k.startswith('fwd:')}
    for k in sorted(mine):
        err, err32, ratio, name = mine[k]
        print('WORST %-40s ratio %5.2f  err_kernel %.3e  err32 %.3e  at %s' % (k, ratio, err, err32, name))
    assert all(v[2] <= R.FACTOR for v in mine.values())
