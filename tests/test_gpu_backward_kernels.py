"""The pointwise / scan kernels of csrc/backward.hip and the two criteria kernels of csrc/pointwise.hip, one by one,
against the fp64 references of tests/_bwd_ref.py at the shapes where a kernel goes wrong: tail columns, last rows, chunk
and block boundaries, null optional inputs, accumulate flags, leading dimensions wider than the row, rows that belong to
a sibling (sentinels).  Every call goes through ops.* or the ctypes structs of _lib.py.

Tolerances: the helper's rule, atol = 8 * max(err32, 2^-23 max|ref|) per output (err32: the same formula in fp32 torch
on the same inputs); torch.equal where an output has at most three roundings and no transcendental; the project's bars
where named.  `err_kernel / err32` (denominator max(err32, 2^-23 max|ref|); the bound is 8) is printed per output by
`pytest -m gpu -s` - the WORST lines of the file's last test; each test's docstring gives what an MI355X measured (the
largest of all: 4.98, gate_mix_bwd's db_rows; every other output stays below 3)."""
import pytest
import torch

import _bwd_ref as R
from insenticap_model_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = R.SENTINEL


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def d(x):
    return None if x is None else x.to(DEV)


def sent(*shape):
    return torch.full(shape, SENT, device=DEV)


def prefilled(pre, extra_rows=1):
    """`pre` on the device, followed by `extra_rows` sentinel rows the kernel must not touch: (whole buffer, owned view)."""
    buf = sent(pre.shape[0] + extra_rows, *pre.shape[1:])
    buf[:pre.shape[0]] = pre.to(DEV)
    return buf, buf[:pre.shape[0]]


# ------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize('M,N', [(1, 1), (3, 65), (255, 64), (256, 130), (257, 63), (4097, 10)])
def test_colsum_vs_fp64(M, N):
    """(4097, 10): the 64-chunk cap, rows per chunk 65, the chunk count recomputed.  ld = N and ld > N (the column slice
    autograd hands in for the classifier bias), accumulate 0 / 1 on a pre-filled out, out[N:] untouched, M >= 256 (two
    stages) bit-repeatable.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    out 1.86 (255 x 64, accumulate)"""
    g = gen(M * 131 + N)
    for extra in (0, 5):
        big = rn(g, M, N + extra)
        x, xd = big[:, :N], big.to(DEV)[:, :N]
        for acc in (0, 1):
            pre = rn(g, N)
            outs = []
            for rep in range(2 if M >= 256 else 1):
                out = sent(N + 3)
                out[:N] = pre.to(DEV)
                ops.colsum(xd, out, accumulate=bool(acc))
                outs.append(out)
            ref, ev = R.both(R.colsum_ref, x, prefill=pre if acc else None)
            R.check_output(outs[0], ref['out'], ev['out'], 'colsum/out[%dx%d ld+%d acc%d]' % (M, N, extra, acc), pad='sentinel')
            assert all(torch.equal(o, outs[0]) for o in outs)


def test_colsum_multi_26_jobs_vs_fp64_and_vs_colsum():
    """26 jobs = two library calls (ISC_COLSUM_MAX_JOBS = 24); single-chunk (M < 256) and multi-chunk jobs interleaved so
    blk0, blk1 and part_off all advance; 1-3 outputs, accumulate 0 / 1, ld > N.  M < 256: ops.colsum's bits.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    out 1.88 (job 17, 4100 x 64)"""
    assert _lib.ISC_COLSUM_MAX_JOBS < 26
    g = gen(77)
    Ms, Ns = [1, 256, 7, 1000, 255, 4100], [1, 63, 64, 65, 200]
    jobs, meta = [], []
    for i in range(26):
        M, N, n_out, acc, extra = Ms[i % 6], Ns[i % 5], i % 3 + 1, (i // 3) % 2, 3 if i % 4 in (1, 2) else 0
        big = rn(g, M, N + extra)
        xd = big.to(DEV)[:, :N]
        pres = [rn(g, N) for _ in range(n_out)]
        outs = []
        for p in pres:
            o = sent(N + 2)
            o[:N] = p.to(DEV)
            outs.append(o)
        jobs.append((xd, outs, bool(acc)))
        meta.append((big[:, :N], pres, acc, M, N))
    assert {m[2] for m in meta if m[3] < 256} == {0, 1} == {m[2] for m in meta if m[3] >= 256}
    ops.colsum_multi(jobs)
    for i, ((xd, outs, _), (x, pres, acc, M, N)) in enumerate(zip(jobs, meta)):
        for k, (o, p) in enumerate(zip(outs, pres)):
            ref, ev = R.both(R.colsum_ref, x, prefill=p if acc else None)
            R.check_output(o, ref['out'], ev['out'], 'colsum_multi/out[job%d %dx%d out%d acc%d]' % (i, M, N, k, acc),
                           pad='sentinel')
            if M < 256:
                one = sent(N + 2)
                one[:N] = p.to(DEV)
                ops.colsum(xd, one, accumulate=bool(acc))
                assert torch.equal(one, o), (i, M, N)


# ------------------------------------------------------------------------------------------------ LSTM cell backward
@pytest.mark.parametrize('M,H', [(1, 4), (5, 33), (7, 512), (300, 96)])
def test_lstm_bwd_vs_fp64(M, H):
    """Activated gates saved in fp32; |c| up to 8 plus saturated cells c = +-50 (tanh = +-1 exactly: finite, and no
    gradient reaches c through the tanh term); at (5, 33) all eight combinations of dh2 / dc_next / dgates_sum present or
    None; dgates_sum is += on non-zero values.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    dgates 1.53, dc_prev 1.00, dgates_sum 1.00"""
    g = gen(M + H)
    dh, dh2, dcn = rn(g, M, H), rn(g, M, H), rn(g, M, H)
    gates = torch.cat([torch.sigmoid(rn(g, M, 2 * H)), torch.tanh(rn(g, M, H)), torch.sigmoid(rn(g, M, H))], dim=1)
    c_prev = rn(g, M, H)
    c = (torch.rand(M, H, generator=g) * 2 - 1) * 8
    satm = torch.zeros(M, H, dtype=torch.bool)
    if M > 1:
        satm[-1] = True
    else:
        satm[0, -2:] = True
    c[satm] = torch.tensor([50.0, -50.0]).repeat(H)[:int(satm.sum())]
    combos = [(a, b, s) for a in (0, 1) for b in (0, 1) for s in (0, 1)] if (M, H) == (5, 33) else [(1, 1, 1), (0, 0, 0)]
    for use_dh2, use_dcn, use_sum in combos:
        a_dh2, a_dcn = (dh2 if use_dh2 else None), (dcn if use_dcn else None)
        pre = rn(g, M, 4 * H) if use_sum else None
        dg_buf, dg = prefilled(torch.full((M, 4 * H), SENT))
        dc_buf, dc = prefilled(torch.full((M, H), SENT))
        ds_buf, ds = prefilled(pre) if use_sum else (None, None)
        ops.lstm_bwd(d(dh), d(a_dh2), d(a_dcn), d(gates), d(c_prev), d(c), dg, dc, ds)
        ref, ev = R.both(R.lstm_bwd_ref, dh, a_dh2, a_dcn, gates, c_prev, c, dgates_sum=pre)
        tag = '[%dx%d dh2=%d dc_next=%d sum=%d]' % (M, H, use_dh2, use_dcn, use_sum)
        R.check_output(dg_buf, ref['dgates'], ev['dgates'], 'lstm_bwd/dgates' + tag)
        R.check_output(dc_buf, ref['dc_prev'], ev['dc_prev'], 'lstm_bwd/dc_prev' + tag)
        if use_sum:
            R.check_output(ds_buf, ref['dgates_sum'], ev['dgates_sum'], 'lstm_bwd/dgates_sum' + tag)
        dcp, dgc = dc.cpu(), dg.cpu()
        if use_dcn:           # d c = 0 * d h o + dc_next exactly; one rounding into dc_prev
            assert torch.equal(dcp[satm], (dcn * gates[:, H:2 * H])[satm])
        else:
            assert bool((dcp[satm] == 0).all())
            for k in range(3):                                   # d i, d f, d g carry d c as a factor
                assert bool((dgc[:, k * H:(k + 1) * H][satm] == 0).all())


# ------------------------------------------------------------------------------------------------ gate mix backward
@pytest.mark.parametrize('B', [1, 3, 4, 5, 130])
def test_gate_mix_bwd_vs_fp64(B):
    """Four rows per workgroup: B around 4 and 130 = 32 full workgroups + 2 rows; A, D below / at / above / not a multiple
    of the 64 lanes; beta = column t of a [B, T] tensor (beta_ld = T); accumulate 0 / 1 on pre-filled dw_rows / db_rows; dv,
    ds, dz overwritten either way.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    dv 0.45, ds 0.66, dz 2.93, dw_rows 2.24, db_rows 4.98
    (B = 1, A = 4, accumulate: err 1.2e-7 where err32 is 4e-10 and the one element is 0.2, so 2^-23 max|ref| divides)"""
    g = gen(B)
    T, t = 3, 1
    for A in (4, 64, 100):
        for D in (4, 32, 96):
            z, w, v, s, dfeat = rn(g, B, A), rn(g, A, scale=0.3), rn(g, B, D), rn(g, B, D), rn(g, B, D)
            beta_all = torch.sigmoid(rn(g, B, T))
            beta_d = beta_all.to(DEV)[:, t]
            assert beta_d.stride(0) == T
            for acc in (0, 1):
                pw, pb = rn(g, B, A), rn(g, B)
                dv_buf, dv_ = prefilled(torch.full((B, D), SENT))
                ds_buf, ds_ = prefilled(torch.full((B, D), SENT))
                dz_buf, dz_ = prefilled(torch.full((B, A), SENT))
                dw_buf, dw_ = prefilled(pw)
                db_buf, db_ = prefilled(pb)
                ops.gate_mix_bwd(d(z), d(w), d(v), d(s), beta_d, d(dfeat), dv_, ds_, dz_, dw_, db_, acc)
                ref, ev = R.both(R.gate_mix_bwd_ref, z, w, v, s, beta_all[:, t], dfeat,
                                 dw_rows=pw if acc else None, db_rows=pb if acc else None)
                tag = '[B%d A%d D%d acc%d]' % (B, A, D, acc)
                for k, buf in (('dv', dv_buf), ('ds', ds_buf), ('dz', dz_buf), ('dw_rows', dw_buf)):
                    R.check_output(buf, ref[k], ev[k], 'gate_mix_bwd/%s%s' % (k, tag))
                R.check_output(db_buf, ref['db_rows'], ev['db_rows'], 'gate_mix_bwd/db_rows' + tag, pad='sentinel')


# ------------------------------------------------------------------------------------------------ ReLU / dropout backward
@pytest.mark.parametrize('n', [1, 255, 256, 257, 70001])
def test_relu_mask_bwd_exact(n):
    """dz = dy (y > 0) [mask scale]: at most two roundings, so the fp32 torch expression's bits.  y holds exact +0.0, -0.0
    and negatives (all closed); y = None (pure dropout backward); uint8 mask with scale 2; in place (dz is dy)."""
    g = gen(n)
    dy, y = rn(g, n), rn(g, n)
    y[::3] = 0.0
    y[1::7] = -0.0
    mask = (torch.rand(n, generator=g) > 0.4).to(torch.uint8)
    for use_y in (True, False):
        for use_mask in (False, True):
            for inplace in (False, True):
                want = torch.where(y > 0, dy, torch.zeros_like(dy)) if use_y else dy.clone()
                if use_mask:
                    want = want * (mask.float() * 2.0)
                src_buf, src = prefilled(dy)
                dst_buf, dst = (src_buf, src) if inplace else prefilled(torch.full((n,), SENT))
                ops.relu_mask_bwd(src, d(y) if use_y else None, dst, keep_mask=d(mask) if use_mask else None, scale=2.0)
                assert torch.equal(dst.cpu(), want), (n, use_y, use_mask, inplace)
                assert float(dst_buf[n]) == SENT and float(src_buf[n]) == SENT
                if not inplace:
                    assert torch.equal(src.cpu(), dy)


# ------------------------------------------------------------------------------------------------ log-softmax backward
LSM_B, LSM_T = 3, 7


def _lsm_rows(remap_T, step_rows):
    """Output row of input row m = b T + t."""
    M = LSM_B * LSM_T
    if not remap_T:
        return list(range(M))
    return [(m % LSM_T) * step_rows + m // LSM_T for m in range(M)]


@pytest.mark.parametrize('V', [1, 5, 255, 256, 257, 1000])
def test_logsoftmax_bwd_dense_vs_fp64(V):
    """dlogits = dlogp - exp(logp) sum(dlogp) on the saved fp32 log-probs; V around the 256 threads; ld_out = V and V + 27
    with the padding pre-filled (zeros must be written); rows b-major or remapped to t-major.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    dlogits 1.64 (V = 256)"""
    g = gen(V)
    M = LSM_B * LSM_T
    logp = torch.log_softmax(rn(g, M, V, scale=3.0), dim=-1)
    dlogp = rn(g, M, V)
    ref, ev = R.both(R.logsoftmax_bwd_ref, logp, dense=dlogp)
    for ld in (V, V + 27):
        for remap in (0, LSM_T):
            out = sent(M + 1, ld)
            ops.logsoftmax_bwd(d(dlogp), d(logp), out, M, V, remap_T=remap)
            R.check_output(out, ref['dlogits'], ev['dlogits'], 'logsoftmax_bwd/dlogits[V%d ld%d remap%d]' % (V, ld, remap),
                           rows=_lsm_rows(remap, LSM_B))


@pytest.mark.parametrize('V', [1, 5, 255, 256, 257, 1000])
def test_logsoftmax_bwd_sparse_vs_fp64(V):
    """scale (dense + scatter - exp(logp) tot): a dense part only, one pair, two pairs (rows where both name the same
    column, rows whose coefficients are all 0) with and without a dense part; scale None and 2^7; out_step_rows = B + 2:
    the two sibling rows of every step keep their sentinel.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    dlogits 1.84 (V = 255, dense + two pairs)"""
    g = gen(1000 + V)
    B, T, M = LSM_B, LSM_T, LSM_B * LSM_T
    logp = torch.log_softmax(rn(g, M, V, scale=3.0), dim=-1)
    dense = rn(g, M, V)
    ids1, ids2 = torch.randint(0, V, (M,), generator=g), torch.randint(0, V, (M,), generator=g)
    ids1[0], ids1[1] = 0, V - 1
    ids2[::2] = ids1[::2]
    cf1, cf2 = rn(g, M), rn(g, M)
    cf1[2] = cf2[2] = cf1[5] = cf2[5] = 0.0
    variants = {'dense': (dense, []), 'one': (None, [(ids1, cf1)]), 'two': (None, [(ids1, cf1), (ids2, cf2)]),
                'dense+two': (dense, [(ids1, cf1), (ids2, cf2)])}
    for vname, (dn, sp) in variants.items():
        sp_d = [(i.to(DEV), c.to(DEV)) for i, c in sp]
        for scale in (None, 128.0):
            ref, ev = R.both(R.logsoftmax_bwd_ref, logp, dense=dn, sparse=sp, scale=scale)
            sc_d = None if scale is None else torch.tensor([scale], device=DEV)
            for ld in (V, V + 27):
                for remap, osr in ((0, 0), (T, 0), (T, B + 2)):
                    step_rows = osr if osr else B
                    out = sent((T * step_rows if remap else M) + 1, ld)
                    ops.logsoftmax_bwd_sparse(d(dn), d(logp), sp_d, out, M, V, remap_T=remap, scale=sc_d, out_step_rows=osr)
                    R.check_output(out, ref['dlogits'], ev['dlogits'],
                                   'logsoftmax_bwd_sparse/dlogits[V%d %s scale=%s ld%d remap%d osr%d]'
                                   % (V, vname, scale, ld, remap, osr), rows=_lsm_rows(remap, step_rows))
        if vname == 'two':                 # rows whose coefficients are all zero: exact zeros
            assert bool((out.cpu()[_lsm_rows(T, B + 2)][[2, 5]] == 0).all())


# ------------------------------------------------------------------------------------------------ the criteria on raw logits
@pytest.mark.parametrize('V', [5, 129, 257, 300])
def test_gather_logp_raw_and_logsoftmax_bwd_raw_vs_fp64(V):
    """Logits and tile statistics from the project's own classifier forward (ops.vocab_fwd, logits= given, step-stacked
    rows t * step_rows + b with step_rows = B + 2); reference: fp64 log_softmax of the fp32 logits the forward wrote.
    V = 300: the float4 path of the backward; 5, 129, 257: the scalar path; one or two statistics tiles.  Both memory
    layouts of the logits - [T, step_rows, V] as the forward leaves them ((ld_b, ld_t) = (V, step_rows V)) and a [B, T, V']
    copy ((T V', V')) - live given / None, one or two pairs, scale, out_step_rows > B with sentinels.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    gather_logp_raw logp 0.67, logsoftmax_bwd_raw dlogits 0.75"""
    g = gen(V)
    B, T, Bs, K = 3, 4, 5, 32
    M, nt = T * Bs, (V + 127) // 128
    h, W, bias = rn(g, M, K), rn(g, V, K, scale=0.5), rn(g, V)
    pm, ps = torch.empty(M, nt, device=DEV), torch.empty(M, nt, device=DEV)
    pi = torch.empty(M, nt, device=DEV, dtype=torch.int32)
    lg = torch.empty(M, V, device=DEV)
    ops.vocab_fwd(d(h), d(W), d(bias), pm, ps, pi, lg)
    torch.cuda.synchronize()
    lt = lg.view(T, Bs, V)[:, :B]                                   # [T, B, V]: this branch's rows
    logits_bt = lt.transpose(0, 1).contiguous().cpu()               # [B, T, V], what both kernels read
    Vp = V + 4
    bm = sent(B, T, Vp)
    bm[:, :, :V] = lt.transpose(0, 1)
    layouts = {'time_major': (lg, V, Bs * V), 'batch_major': (bm, T * Vp, Vp)}
    ids1, ids2 = torch.randint(0, V, (B, T), generator=g), torch.randint(0, V, (B, T), generator=g)
    ids1[0, 0], ids1[0, 1] = 0, V - 1
    ids2[0] = ids1[0]
    cf1, cf2 = rn(g, B, T), rn(g, B, T)
    cf1[1, 2] = cf2[1, 2] = cf1[2, 3] = cf2[2, 3] = 0.0
    lref, lev = R.both(R.logp_of_logits_ref, logits_bt)
    live = torch.tensor([1.0, 0.0, 1.0, 0.5])
    osr = B + 2
    rows = [t * osr + b for b in range(B) for t in range(T)]
    for lname, (raw, ld_b, ld_t) in layouts.items():
        for lv in (None, live):
            out = sent(B * T)
            ops.gather_logp_raw(raw, ld_b, ld_t, B, T, V, pm, ps, Bs, d(ids1), out, live=d(lv))
            want = [x['logp'].gather(2, ids1.unsqueeze(2)).squeeze(2) for x in (lref, lev)]
            if lv is not None:
                want = [want[0] * lv.double(), want[1] * lv]
            R.check_output(out.view(B, T), want[0], want[1], 'gather_logp_raw/logp[V%d %s live=%d]' % (V, lname, lv is not None))
        for sp in ([(ids1, cf1)], [(ids1, cf1), (ids2, cf2)]):
            sp_d = [(i.to(DEV), c.to(DEV)) for i, c in sp]
            for scale in (None, 128.0):
                ref, ev = R.both(R.raw_bwd_ref, logits_bt.view(B * T, V), sp, scale=scale)
                sc_d = None if scale is None else torch.tensor([scale], device=DEV)
                for ld in (V, V + 28):
                    out = sent(T * osr + 1, ld)
                    ops.logsoftmax_bwd_raw(raw, ld_b, ld_t, B, T, V, pm, ps, Bs, sp_d, out, scale=sc_d, out_step_rows=osr)
                    R.check_output(out, ref['dlogits'], ev['dlogits'], 'logsoftmax_bwd_raw/dlogits[V%d %s pairs%d scale=%s ld%d]'
                                   % (V, lname, len(sp), scale, ld), rows=rows)
                    assert bool((out.cpu()[[2 * osr + 1, 3 * osr + 2]] == 0).all())     # all-zero coefficients: exact zeros
    assert float(bm[:, :, V:].min()) == SENT == float(bm[:, :, V:].max())


# ------------------------------------------------------------------------------------------------ XE criterion
@pytest.mark.parametrize('B,T,V', [(1, 1, 3), (3, 7, 11), (70, 20, 50)])
def test_xe_criterion_kernels(B, T, V):
    """xe_loss_fwd / xe_loss_tokens_fwd {sum, count} against fp64 (the count exactly); xe_loss_bwd_sparse's coefficients
    are -gout / count at the unmasked positions (one division: the fp32 expression's bits) and 0 elsewhere; xe_loss_bwd
    is exactly their scatter into a zeroed [B, T, V].  Lengths 0, T and above T; (70, 20, 50): 1400 positions, more than
    one pass of the single workgroup's 256 threads.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    sum 0.41 for both entry points (70 x 20 x 50; err 2.4e-4 on a sum near 4800)"""
    g = gen(B * T + V)
    logp = torch.log_softmax(rn(g, B, T, V, scale=2.0), dim=-1)
    target = torch.randint(0, V, (B, T), generator=g)
    lengths = torch.randint(0, T + 4, (B,), generator=g).to(torch.int32)
    lengths[:3] = torch.tensor([0, T, T + 3], dtype=torch.int32)[:B] if B >= 3 else torch.tensor([T], dtype=torch.int32)
    assert int(lengths.max()) > 0
    mask = torch.arange(T)[None, :] < lengths[:, None]
    tlp = logp.gather(2, target.unsqueeze(2)).squeeze(2)
    ref, ev = R.both(R.xe_loss_ref, tlp, mask)
    len_d, tgt_d = lengths.to(DEV), target.to(DEV)
    out_a, out_b = sent(3), sent(3)
    ops.xe_loss_fwd(d(logp), tgt_d, len_d, out_a)
    ops.xe_loss_tokens_fwd(d(tlp), len_d, out_b)
    for name, o in (('xe_loss_fwd', out_a), ('xe_loss_tokens_fwd', out_b)):
        R.check_output(o[:1], ref['sum'], ev['sum'], '%s/sum[%dx%dx%d]' % (name, B, T, V))
        assert float(o[1]) == float(mask.sum()) and float(o[2]) == SENT
    assert torch.equal(out_a, out_b)                  # (the same summation order by construction: the same bits)
    gout = torch.tensor([1.7])
    coef_want = torch.where(mask, -gout / out_a.cpu()[1], torch.zeros(1)).float()
    coef_buf = sent(B * T + 1)
    ops.xe_loss_bwd_sparse(len_d, T, d(gout), out_a, coef_buf[:B * T])
    assert torch.equal(coef_buf[:B * T].cpu().view(B, T), coef_want) and float(coef_buf[B * T]) == SENT
    dl_buf = sent(B * T * V + 1)
    dl_buf[:B * T * V] = 0.0
    dlogp = dl_buf[:B * T * V].view(B, T, V)
    ops.xe_loss_bwd(tgt_d, len_d, d(gout), out_a, dlogp)
    want = torch.zeros(B, T, V).scatter_(2, target.unsqueeze(2), coef_want.unsqueeze(2))
    assert torch.equal(dlogp.cpu(), want) and float(dl_buf[B * T * V]) == SENT
    assert int((dlogp != 0).sum()) == int(mask.sum())


# ------------------------------------------------------------------------------------------------ attention scan backward
def _scan_inputs(g, B, R_, A, D, with_q2, T=3, t=1):
    P, V, q, w = rn(g, B, R_, A), rn(g, B, R_, D), rn(g, B, A), rn(g, A, scale=0.3)
    q2 = rn(g, B, A) if with_q2 else None
    alpha_all = torch.softmax(rn(g, B, T, R_), dim=-1)
    dout = rn(g, B, D)
    x = dict(P=P, V=V, q=q, w=w, q2=q2, alpha=alpha_all[:, t], alpha_d=alpha_all.to(DEV)[:, t], dout=dout)
    # a problem struct holds bare addresses: the device copies live as long as x, whatever is allocated before the launch
    x['dev'] = {k: d(x[k]) for k in ('P', 'V', 'q', 'w', 'q2', 'dout')}
    return x


def _scan_run(x, acc, pre, with_dP=True, with_dV=True, rows_alloc=None):
    """One launch; returns the whole buffers (one sentinel row behind the owned ones, or rows_alloc rows in all)."""
    B, R_, A = x['P'].shape
    D = x['V'].shape[2]
    extra = 1 if rows_alloc is None else rows_alloc - B
    bufs = {'de': prefilled(torch.full((B, R_), SENT), extra), 'dq': prefilled(torch.full((B, A), SENT), extra),
            'dw_rows': prefilled(pre['dw_rows'], extra), 'dP': prefilled(pre['dP'], extra), 'dV': prefilled(pre['dV'], extra)}
    xd = x['dev']
    prob = ops.scan_bwd_problem(xd['P'], xd['V'], xd['q'], xd['w'], x['alpha_d'], xd['dout'],
                                bufs['dP'][1] if with_dP else None, bufs['dV'][1] if with_dV else None, bufs['dq'][1],
                                bufs['dw_rows'][1], acc, q2=xd['q2'], de_out=bufs['de'][1])
    return prob, bufs


def _scan_ref(x, acc, pre):
    kw = dict(dP0=pre['dP'], dV0=pre['dV'], dw0=pre['dw_rows']) if acc else {}
    return R.both(R.scan_bwd_ref, x['P'], x['V'], x['q'], x['w'], x['alpha'], x['dout'], q2=x['q2'], **kw)


def _scan_pre(g, B, R_, A, D):
    return {'dP': rn(g, B, R_, A), 'dV': rn(g, B, R_, D), 'dw_rows': rn(g, B, A)}


@pytest.mark.parametrize('with_q2', [False, True], ids=['q', 'q+q2'])
@pytest.mark.parametrize('B,R_,A,D', [(1, 1, 4, 4), (3, 6, 32, 32), (5, 37, 64, 128), (2, 196, 512, 512), (4, 11, 1024, 64),
                                      (3, 50, 96, 32), (2, 5, 288, 96)])
def test_attn_scan_bwd_all_five_outputs_vs_fp64(B, R_, A, D, with_q2):
    """d e, d q, dw_rows, dP, dV of ONE step against fp64 autograd of e = w . tanh(P + q (+ q2)), out = alpha V at the
    saved alpha (a strided [B, T, R] view).  One region / one float4 column up to A = 1024 (four region groups) and 196
    regions; widths whose quarter does not divide the 1024 threads (A = 96: 42 region groups and 16 idle threads, more
    regions than groups; A = 288: 14 groups; D = 96); accumulate 0 / 1 on pre-filled dP, dV, dw_rows (dq is overwritten
    either way); dP = None or dV = None with de_out given leaves every other output's bits alone.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    d e 1.91, dq 1.38, dw_rows 1.26, dP 1.42, dV 0.44"""
    g = gen(B * 1000 + R_ + A + D + int(with_q2))
    x = _scan_inputs(g, B, R_, A, D, with_q2)
    assert x['alpha_d'].stride(0) == 3 * R_
    tag = '[%dx%dx%dx%d q2=%d' % (B, R_, A, D, with_q2)
    kept = None
    for acc in (0, 1):
        pre = _scan_pre(g, B, R_, A, D)
        prob, bufs = _scan_run(x, acc, pre)
        ops.attn_scan_bwd([prob], B)
        ref, ev = _scan_ref(x, acc, pre)
        for k in ('de', 'dq', 'dw_rows', 'dP', 'dV'):
            R.check_output(bufs[k][0], ref[k], ev[k], 'attn_scan_bwd/%s%s acc%d]' % (k, tag, acc))
        if acc == 0:
            kept = {k: b[0].clone() for k, b in bufs.items()}
    pre = _scan_pre(g, B, R_, A, D)
    for drop in ('dP', 'dV'):
        prob, bufs = _scan_run(x, 0, pre, with_dP=drop != 'dP', with_dV=drop != 'dV')
        ops.attn_scan_bwd([prob], B)
        for k in ('de', 'dq', 'dw_rows', 'dP', 'dV'):
            if k == drop:
                assert torch.equal(bufs[k][0][:B].cpu(), pre[k]) and bool((bufs[k][0][B:] == SENT).all())   # never touched
            else:
                assert torch.equal(bufs[k][0], kept[k]), (drop, k)


def test_attn_scan_bwd_two_problem_launch():
    """One launch over two problems built from _lib.ScanBwdProblem directly: rows = 5 and rows = 3, different R, A, D; the
    grid spans 5 rows, so rows 3 and 4 of the shorter problem's outputs must keep their sentinel.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    d e 0.79, dq 1.48, dw_rows 1.45, dP 1.05, dV 0.42"""
    g = gen(5)
    shapes = [(5, 6, 32, 32), (3, 9, 64, 16)]
    probs, keep = [], []
    for rows, R_, A, D in shapes:
        x = _scan_inputs(g, rows, R_, A, D, with_q2=rows == 3)
        pre = _scan_pre(g, rows, R_, A, D)
        prob, bufs = _scan_run(x, 1, pre, rows_alloc=5 + 1)
        assert isinstance(prob, _lib.ScanBwdProblem)
        prob.rows = rows
        probs.append(prob)
        keep.append((x, pre, bufs))
    ops.attn_scan_bwd(probs, 5)
    for i, (x, pre, bufs) in enumerate(keep):
        ref, ev = _scan_ref(x, 1, pre)
        for k in ('de', 'dq', 'dw_rows', 'dP', 'dV'):
            assert bufs[k][0].shape[0] == 6
            R.check_output(bufs[k][0], ref[k], ev[k], 'attn_scan_bwd2/%s[problem%d rows%d]' % (k, i, shapes[i][0]))


def test_attn_scan_bwd_refuses_what_it_cannot_run():
    """Every one of these returns from the entry point's checks, in front of the launch (csrc/backward.hip,
    isc_attn_scan_bwd: A > 1024 and D > 4096 -> ISC_E_SHAPE; the dynamic LDS need (R + 2 * 1024 / (A / 4) * A
    floats) above 60000 bytes -> ISC_E_SHAPE; a P that is not 16-byte aligned -> ISC_E_ALIGN): the outputs stay untouched."""
    lib, g = _lib.load(), gen(6)

    def rc_of(B, R_, A, D, misalign=False):
        x = _scan_inputs(g, B, R_, A, D, False)
        if misalign:
            flat = torch.zeros(B * R_ * A + 4, device=DEV)
            x_P = flat[1:1 + B * R_ * A].view(B, R_, A)
            assert x_P.data_ptr() % 16 == 4
        pre = _scan_pre(g, B, R_, A, D)
        prob, bufs = _scan_run(x, 0, pre)
        if misalign:
            prob.P = x_P.data_ptr()
        arr = (_lib.ScanBwdProblem * 1)(prob)
        rc = lib.isc_attn_scan_bwd(arr, 1, B, ops.stream())
        torch.cuda.synchronize()
        if rc != 0:
            for k in ('de', 'dq'):
                assert bool((bufs[k][0] == SENT).all())
            for k in ('dP', 'dV', 'dw_rows'):
                assert torch.equal(bufs[k][0][:B].cpu(), pre[k])
        return rc
    assert rc_of(1, 2, 4, 8192) == -2          # D > 4096: more float4 columns than threads
    assert rc_of(1, 2, 96, 4) == 0             # (1024 % 24 != 0 runs: test_attn_scan_bwd_all_five_outputs_vs_fp64)
    assert rc_of(1, 2, 2048, 4) == -2          # A > 1024
    assert (7000 + 2 * 1024 * 4) * 4 > 60000
    assert rc_of(1, 7000, 4, 4) == -2          # LDS
    assert rc_of(1, 2, 8, 8, misalign=True) == -3
    assert rc_of(1, 2, 8, 8) == 0              # (the same shape, aligned: runs)


# ------------------------------------------------------------------------------------------------ dV / dP after the sweep
@pytest.mark.parametrize('T', [25, 33])
def test_dv_dp_after_the_sweep_beyond_the_unrolled_step_count(T):
    """T > ISC_DV_TMAX = 24: attn_dv_from_alpha's loop that is not unrolled (and attn_dp_from_de over as many steps)
    against fp64 and, bit for bit, against attn_scan_bwd accumulating dV / dP at every step in the sweep's order.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    dV 1.22 (T = 25), 0.82 (T = 33); dP 1.00 at both"""
    g = gen(T)
    B, R_, A = 3, 11, 32
    P, V, w = rn(g, B, R_, A), rn(g, B, R_, A), rn(g, A, scale=0.3)
    q, q2 = rn(g, T, B, A), rn(g, B, A)
    alpha = torch.softmax(rn(g, B, T, R_), dim=-1)
    dout = rn(g, T, B, A)
    Pd, Vd, wd, qd, q2d, ad, dod = d(P), d(V), d(w), d(q), d(q2), d(alpha), d(dout)
    dP, dV = sent(B, R_, A), sent(B, R_, A)
    de, dq, dw = sent(T, B, R_), sent(T, B, A), sent(B, A)
    for i, t in enumerate(range(T - 1, -1, -1)):
        ops.attn_scan_bwd([ops.scan_bwd_problem(Pd, Vd, qd[t], wd, ad[:, t], dod[t], dP, dV, dq[t], dw, i > 0, q2=q2d,
                                                de_out=de[t])], B)
    dV2, dP2 = sent(B + 1, R_, A), sent(B + 1, R_, A)
    ops.attn_dv_from_alpha(ad, dod, dV2[:B])
    ops.attn_dp_from_de(Pd, qd, wd, de, dP2[:B], q2=q2d)
    assert torch.equal(dV2[:B], dV) and torch.equal(dP2[:B], dP)
    ref, ev = R.both(R.dv_from_alpha_ref, alpha, dout)
    R.check_output(dV2, ref['dV'], ev['dV'], 'attn_dv_from_alpha/dV[T%d vs the sweep]' % T)
    ref, ev = R.both(R.dp_from_de_ref, P, q, w, de.cpu(), q2=q2)          # (d e: the fp32 values the kernel receives)
    R.check_output(dP2, ref['dP'], ev['dP'], 'attn_dp_from_de/dP[T%d vs the sweep]' % T)


@pytest.mark.parametrize('B,T,R_,D,extra', [(2, 5, 7, 1028, 0), (3, 4, 5, 12, 0), (3, 6, 11, 32, 2), (1, 25, 700, 32, 0)],
                         ids=['second_column_block', 'three_float4', 'step_rows', 'r700'])
def test_attn_dv_from_alpha_edges_vs_fp64(B, T, R_, D, extra):
    """D = 1028: a second column block of ONE float4; D = 12; dout as the [:, :B] rows of a [T, B + 2, D] stack (step_rows);
    700 regions at T = 25: more than the 60000-byte [T][Rc] image holds at once.  alpha: a [B, T, R] view of wider rows.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    dV 0.82, 0.30, 0.58, 0.99 in the order of the cases"""
    g = gen(B + T + R_ + D)
    alpha_w = torch.softmax(rn(g, B, T, R_ + 3), dim=-1)
    alpha = alpha_w[:, :, :R_]
    big = rn(g, T, B + extra, D)
    dV = sent(B + 1, R_, D)
    ops.attn_dv_from_alpha(alpha_w.to(DEV)[:, :, :R_], big.to(DEV)[:, :B], dV[:B], step_rows=B + extra if extra else 0)
    ref, ev = R.both(R.dv_from_alpha_ref, alpha, big[:, :B])
    R.check_output(dV, ref['dV'], ev['dV'], 'attn_dv_from_alpha/dV[%dx%dx%dx%d rows+%d]' % (B, T, R_, D, extra))


@pytest.mark.parametrize('B,T,R_,A,with_q2', [(2, 5, 7, 1028, True), (3, 4, 5, 12, False), (1, 25, 700, 32, True)],
                         ids=['second_column_block', 'three_float4', 'r700'])
def test_attn_dp_from_de_edges_vs_fp64(B, T, R_, A, with_q2):
    """A = 1028: a second column block of one float4; A = 12; 700 regions at T = 25: several region chunks.  Random d e.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    dP 1.13, 1.06, 1.45 in the order of the cases"""
    g = gen(B + T + R_ + A + 1)
    P, q, w, de = rn(g, B, R_, A), rn(g, T, B, A), rn(g, A, scale=0.3), rn(g, T, B, R_, scale=0.1)
    q2 = rn(g, B, A) if with_q2 else None
    dP = sent(B + 1, R_, A)
    ops.attn_dp_from_de(d(P), d(q), d(w), d(de), dP[:B], q2=d(q2))
    ref, ev = R.both(R.dp_from_de_ref, P, q, w, de, q2=q2)
    R.check_output(dP, ref['dP'], ev['dP'], 'attn_dp_from_de/dP[%dx%dx%dx%d q2=%d]' % (B, T, R_, A, with_q2))


# ------------------------------------------------------------------------------------------------ clamp + Adam
@pytest.mark.parametrize('clip', [0.0, 0.1])
def test_clamp_adam_50_tensors_vs_torch(clip):
    """Three steps against torch.optim.Adam at test_clamp_adam_vs_torch's bar (tests/test_gpu_backward.py: atol = 2e-6):
    50 tensors (two launches: ISC_ADAM_MAX_TENSORS = 48), sizes around the 1024 elements of a workgroup, weight_decay =
    1e-2; clip = 0 leaves the gradients' bits alone, clip = 0.1 clamps them in place; the device-resident `hyper` form
    (ops.adam_hyper) gives the scalar form's bits.  The parameters lie in one arena with a sentinel between neighbours."""
    ADAM_ATOL = 2e-6
    lr, b1, b2, eps, wd = 4e-4, 0.9, 0.999, 1e-8, 1e-2
    g = gen(50)
    sizes = [1, 1023, 1024, 1025, 3000] * 10
    ps = [rn(g, n) for n in sizes]
    gs = [rn(g, n, scale=0.3) for n in sizes]
    ref_p = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.Adam(ref_p, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)

    def state():
        arena = sent(sum(sizes) + len(sizes))
        views, off = [], 0
        for p in ps:
            views.append(arena[off:off + p.numel()])
            views[-1].copy_(p)
            off += p.numel() + 1
        return arena, views, [torch.zeros(n, device=DEV) for n in sizes], [torch.zeros(n, device=DEV) for n in sizes]
    (arena, p1, m1, v1), (arena2, p2, m2, v2) = state(), state()
    for it in range(3):
        g_it = [x * (it + 1) for x in gs]
        g_want = [x.clamp(-clip, clip) if clip else x for x in g_it]
        for q, x in zip(ref_p, g_want):
            q.grad = x.clone()
        opt.step()
        gd1, gd2 = [x.to(DEV) for x in g_it], [x.to(DEV) for x in g_it]
        ops.clamp_adam(p1, gd1, m1, v1, lr, b1, b2, eps, wd, clip, it + 1)
        hyper = torch.tensor(ops.adam_hyper(lr, b1, b2, it + 1), dtype=torch.float32, device=DEV)
        ops.clamp_adam(p2, gd2, m2, v2, lr, b1, b2, eps, wd, clip, it + 1, hyper=hyper)
        for a, b, want in zip(gd1, gd2, g_want):
            assert torch.equal(a.cpu(), want) and torch.equal(b.cpu(), want)
    for i, (a, b) in enumerate(zip(ref_p, p1)):
        err = float((b.cpu() - a.detach()).abs().max())
        assert err <= ADAM_ATOL, (i, sizes[i], err)
        st = opt.state[a]
        assert float((m1[i].cpu() - st['exp_avg']).abs().max()) <= ADAM_ATOL
        assert float((v1[i].cpu() - st['exp_avg_sq']).abs().max()) <= ADAM_ATOL
    assert torch.equal(arena, arena2)
    for x, y in zip(m1 + v1, m2 + v2):
        assert torch.equal(x, y)
    gaps = torch.ones(arena.numel(), dtype=torch.bool)
    off = 0
    for n in sizes:
        gaps[off:off + n] = False
        off += n + 1
    assert bool((arena.cpu()[gaps] == SENT).all()) and int(gaps.sum()) == len(sizes)


def test_zz_report_the_measured_ratios():
    """Prints err_kernel / err32 of every output this file measured (pytest -s): the table of the file's docstrings."""
    for k in sorted(R.WORST):
        err, err32, ratio, name = R.WORST[k]
        print('WORST %-36s ratio %5.2f  err_kernel %.3e  err32 %.3e  at %s' % (k, ratio, err, err32, name))
    assert all(v[2] <= R.FACTOR for v in R.WORST.values())
