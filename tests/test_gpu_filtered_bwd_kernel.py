"""isc_logsoftmax_bwd_raw_filtered alone: d logits of the sampled distribution's log-probability (plus zero to two model
pairs) against the fp64 formula of tests/_filtered_rl_ref.py.  The saved scalars (K*, the largest allowed logit, log Z,
the banned ids) come from the reference, so the kernel is tested apart from the forward that normally writes them.

Bound: the project's yardstick with the issue's factor, 4 * max(e, 2^-23 max|ref|), e = the error of the same formula in
torch fp32 on the CPU.  `err_kernel / max(e, 2^-23 max|ref|)` is printed per call by `pytest -m gpu -s`; an MI355X
measured at most 0.99 (the bound is 4)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _filtered_rl_ref as FR
from insenticap_model_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = -7.0
LOG2E = 1.4426950408889634


def pad32(v):
    return (v + 31) // 32 * 32


def make_rows(V, tau, seed, B=3, T=4):
    """B x T rows of fp32 logits and, per row, its controls -> (kept set, banned ids, token, coefficient).  Row r = b*T + t:
    0 filter off (K = everything); 1 top_k = 1; 2 top_k = 5; 3 top_p = 0.8; 4 tied logits straddling K* (top_k = 2 over
    x[0] > x[1] == x[3]: id 1 kept, id 3 not); 5 two banned ids in the top ranks (one listed twice) under top_k = 4;
    6 every coefficient zero and the logits NaN; 7 filtered coefficient zero, model coefficients not; then top_k = 3 with
    top_p = 0.9, and the same again."""
    rng = np.random.default_rng(seed)
    M = B * T
    x = (3.0 * rng.standard_normal((M, V))).astype(np.float32)
    rows = []
    ctl = [(0, 1.0), (1, 1.0), (5, 1.0), (0, 0.8), (2, 1.0), (4, 1.0), (0, 1.0), (0, 0.7), (3, 0.9)]
    for r in range(M):
        k, p = ctl[r % len(ctl)]
        ban = []
        if r % len(ctl) == 4:
            top = np.abs(x[r]).max() + 1.0
            x[r, 0], x[r, 1], x[r, 3] = top + 1.0, top, top
        if r % len(ctl) == 5:
            o = np.argsort(-x[r].astype(np.float64), kind='stable')
            ban = [int(o[0]), int(o[2]), int(o[0])]
        kept = FR.kept_ids(x[r], tau, k, p, ban)
        tok = int(kept[rng.integers(len(kept))])
        coef = np.float32(rng.standard_normal())
        if r % len(ctl) in (6, 7):
            coef = np.float32(0.0)
        rows.append(dict(kept=kept, ban=ban, tok=tok, coef=coef, dead=r % len(ctl) == 6))
    assert M <= 4 or set(rows[4]['kept']) == {0, 1}
    return x, rows


def saved(x, rows, tau):
    M = len(rows)
    ks, gm, lz = np.zeros(M, np.int64), np.zeros(M, np.float32), np.zeros(M, np.float32)
    ban = np.full((M, FR.CON_MAX), -1, np.int32)
    for r, row in enumerate(rows):
        ks[r], gm[r], lz[r] = FR.saved_scalars(x[r], tau, row['kept'])
        ban[r, :len(row['ban'])] = row['ban']
    return ks, gm, lz, ban


def reference(x, rows, tau, pairs, scale, dtype):
    """[M, V] d logits in `dtype` (float64: the reference; float32: the same formula, for the yardstick's e)."""
    M, V = x.shape
    out = torch.zeros(M, V, dtype=dtype)
    xt = torch.from_numpy(x).to(dtype)
    sc = 1.0 if scale is None else scale
    for r, row in enumerate(rows):
        if row['dead']:
            continue
        if pairs:
            lp = torch.log_softmax(xt[r], dim=0)
            v = torch.zeros(V, dtype=dtype)
            tot = torch.zeros((), dtype=dtype)
            for ids, cf in pairs:
                v[int(ids[r])] += float(cf[r])
                tot = tot + torch.tensor(float(cf[r]), dtype=dtype)
            out[r] = (v - torch.exp(lp) * tot) * sc
        if row['coef'] != 0:
            if dtype == torch.float64:
                f = torch.from_numpy(FR.row_grad(x[r], tau, row['kept'], row['tok']))
            else:
                ks, gm, lz = FR.saved_scalars(x[r], tau, row['kept'])
                q = torch.exp2((xt[r] - float(gm)) * np.float32(LOG2E / tau)) * torch.exp(torch.tensor(-lz))
                keep = torch.zeros(V, dtype=torch.bool)
                keep[torch.from_numpy(row['kept'])] = True
                ind = torch.zeros(V, dtype=dtype)
                ind[row['tok']] = 1.0
                f = (ind - torch.where(keep, q.clamp(max=1.0), torch.zeros(()))) * np.float32(1.0 / tau)
            out[r] = out[r] + f.to(dtype) * float(row['coef']) * sc
    return out


def tile_stats(x):
    """(part_max, part_sum) per 128-column tile of fp32 rows, as the classifier forward leaves them."""
    M, V = x.shape
    nt = (V + 127) // 128
    pm, ps = np.zeros((M, nt), np.float32), np.zeros((M, nt), np.float32)
    for j in range(nt):
        t = x[:, j * 128:(j + 1) * 128]
        pm[:, j] = t.max(1)
        ps[:, j] = np.exp(t - pm[:, j:j + 1]).sum(1)
    return pm, ps


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def layouts(x, B, T, pm, ps):
    """The two memory layouts of the logits: a contiguous [B, T, V] and a time-major [T, Bs, V] with Bs = B + 1 (the
    statistics stacked the same way).  Yields (name, raw, ld_b, ld_t, pm, ps, step_rows)."""
    M, V = x.shape
    nt = pm.shape[1]
    yield 'btv', dv(x.reshape(B, T, V)), T * V, V, dv(pm.reshape(B, T, nt).transpose(1, 0, 2)), \
        dv(ps.reshape(B, T, nt).transpose(1, 0, 2)), B
    Bs = B + 1
    xt = np.full((T, Bs, V), np.nan, np.float32)
    xt[:, :B] = x.reshape(B, T, V).transpose(1, 0, 2)
    pmt, pst = np.zeros((T, Bs, nt), np.float32), np.zeros((T, Bs, nt), np.float32)
    pmt[:, :B], pst[:, :B] = pm.reshape(B, T, nt).transpose(1, 0, 2), ps.reshape(B, T, nt).transpose(1, 0, 2)
    yield 'tbv', dv(xt), V, Bs * V, dv(pmt), dv(pst), Bs


def run(raw, ld_b, ld_t, B, T, V, pm, ps, step_rows, pairs, flt, scale, osr):
    out = torch.full((T * osr + 1, pad32(V)), SENT, device=DEV)
    sc = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=DEV)
    ops.logsoftmax_bwd_raw_filtered(raw, ld_b, ld_t, B, T, V, pm, ps, step_rows, pairs, flt, out[:T * osr], scale=sc,
                                    out_step_rows=osr)
    return out


def owned(out, B, T, osr):
    """[M, Vp] rows of the output in [B,T] order."""
    return out[:T * osr].view(T, osr, -1)[:, :B].transpose(0, 1).reshape(B * T, -1)


def check(out, ref64, ref32, B, T, V, osr, what):
    o = out.cpu()
    got = owned(o, B, T, osr)
    assert bool((got[:, V:] == 0).all()), what                                  # pad columns: exact zeros
    assert bool((o[:T * osr].view(T, osr, -1)[:, B:] == SENT).all()) and bool((o[T * osr:] == SENT).all()), what
    e = float((ref32.double() - ref64).abs().max())
    floor = max(e, 2.0 ** -23 * float(ref64.abs().max()))
    err = float((got[:, :V].double() - ref64).abs().max())
    print('FLTBWD %s: err_kernel / max(e, 2^-23 max|ref|) = %.2f' % (what, err / floor if floor else 0.0))
    assert err <= 4 * floor, (what, err, floor)
    return got


@pytest.mark.parametrize('tau', [0.5, 1.0, 2.5])
@pytest.mark.parametrize('V', [5, 64, 129, 200])
def test_filtered_dlogits_vs_fp64(V, tau):
    """V = 64, 200: the float4 path; 5, 129: the scalar path (129: a partial second tile).  Both layouts of the logits,
    out_step_rows = B + 2 with sentinel rows, ld_out = pad32(V) with zero pad columns, scale given and NULL; zero, one and
    two model pairs in the same launch - in bits isc_logsoftmax_bwd_raw's result plus the filtered-only result; top_k = 1
    and the columns outside K exactly 0.0; the all-zero row exact zeros although its logits are NaN."""
    B, T = 3, 4
    M = B * T
    x, rows = make_rows(V, tau, seed=V * 10 + int(tau * 2))
    ks, gm, lz, ban = saved(x, rows, tau)
    rng = np.random.default_rng(V)
    pair_np = [(rng.integers(0, V, size=M).astype(np.int64), rng.standard_normal(M).astype(np.float32)) for _ in range(2)]
    for _, cf in pair_np:
        cf[[r for r, row in enumerate(rows) if row['dead']]] = 0.0
    xs = x.copy()
    xs[[r for r, row in enumerate(rows) if row['dead']]] = 0.0
    pm, ps = tile_stats(xs)
    xn = x.copy()
    xn[[r for r, row in enumerate(rows) if row['dead']]] = np.nan
    flt = dict(tok=dv(np.array([r['tok'] for r in rows], np.int64)), coef=dv(np.array([r['coef'] for r in rows], np.float32)),
               inv_tau=1.0 / tau, kstar=dv(ks), gmax=dv(gm), logz=dv(lz), ban=dv(ban))
    osr = B + 2
    for name, raw, ld_b, ld_t, pmd, psd, srows in layouts(xn, B, T, pm, ps):
        for scale in (None, 0.25):
            f_only = None
            for n in (0, 1, 2):
                pairs = [(dv(i), dv(c)) for i, c in pair_np[:n]]
                out = run(raw, ld_b, ld_t, B, T, V, pmd, psd, srows, pairs, flt, scale, osr)
                ref64 = reference(x, rows, tau, pair_np[:n], scale, torch.float64)
                ref32 = reference(x, rows, tau, pair_np[:n], scale, torch.float32)
                got = check(out, ref64, ref32, B, T, V, osr, 'V%d tau%g %s scale=%s pairs%d' % (V, tau, name, scale, n))
                for r, row in enumerate(rows):
                    if row['dead']:
                        assert bool((got[r] == 0).all())
                if n == 0:
                    f_only = out
                    for r, row in enumerate(rows):
                        outside = np.setdiff1d(np.arange(V), np.append(row['kept'], row['tok']))
                        assert bool((got[r, outside] == 0).all()), r
                        if len(row['kept']) == 1:                         # top_k = 1: the whole row, exactly
                            assert bool((got[r] == 0).all()), r
                    assert bool((got[1] == 0).all())
                else:
                    a_only = torch.full_like(out, SENT)
                    sc = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=DEV)
                    ops.logsoftmax_bwd_raw(raw, ld_b, ld_t, B, T, V, pmd, psd, srows, pairs, a_only[:T * osr], scale=sc,
                                           out_step_rows=osr)
                    want = owned(a_only, B, T, osr) + owned(f_only, B, T, osr)
                    assert torch.equal(owned(out, B, T, osr).view(torch.int32), want.view(torch.int32)), (name, scale, n)


def test_filtered_dlogits_past_the_staging_limit_and_repeatable():
    """V = 12 289 (past ISC_FLT_STAGE_MAX = 12 288, scalar path, 97 statistics tiles), B x T = 2 x 2, one model pair;
    without a ban list; two runs give equal bits."""
    V, tau, B, T = 12289, 0.7, 2, 2
    x, rows = make_rows(V, tau, seed=1, B=B, T=T)
    for row in rows:
        assert not row['ban']
    ks, gm, lz, _ = saved(x, rows, tau)
    pm, ps = tile_stats(x)
    rng = np.random.default_rng(2)
    pair_np = [(rng.integers(0, V, size=B * T).astype(np.int64), rng.standard_normal(B * T).astype(np.float32))]
    flt = dict(tok=dv(np.array([r['tok'] for r in rows], np.int64)), coef=dv(np.array([r['coef'] for r in rows], np.float32)),
               inv_tau=1.0 / tau, kstar=dv(ks), gmax=dv(gm), logz=dv(lz), ban=None)
    name, raw, ld_b, ld_t, pmd, psd, srows = next(layouts(x, B, T, pm, ps))
    pairs = [(dv(i), dv(c)) for i, c in pair_np]
    outs = [run(raw, ld_b, ld_t, B, T, V, pmd, psd, srows, pairs, flt, None, B + 1) for _ in range(2)]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    check(outs[0], reference(x, rows, tau, pair_np, None, torch.float64), reference(x, rows, tau, pair_np, None, torch.float32),
          B, T, V, B + 1, 'V12289')


def test_filtered_dlogits_refusals_leave_the_output_untouched():
    lib = _lib.load()
    B, T, V = 2, 2, 8
    raw = torch.zeros(B, T, V, device=DEV)
    pm, ps = torch.zeros(B * T, 1, device=DEV), torch.ones(B * T, 1, device=DEV)
    i64 = torch.zeros(B * T, dtype=torch.int64, device=DEV)
    f32 = torch.ones(B * T, device=DEV)
    out = torch.full((B * T, 32), SENT, device=DEV)
    ids, cf = (C.c_void_p * 1)(i64.data_ptr()), (C.c_void_p * 1)(f32.data_ptr())

    def call(**kw):
        a = dict(raw=raw.data_ptr(), ld_b=T * V, ld_t=V, B=B, T=T, V=V, pm=pm.data_ptr(), ps=ps.data_ptr(), srows=0, ids=ids,
                 cf=cf, n=1, tok=i64.data_ptr(), coef=f32.data_ptr(), inv_tau=1.0, kstar=i64.data_ptr(), gmax=f32.data_ptr(),
                 logz=f32.data_ptr(), ban=None, scale=None, out=out.data_ptr(), ld_out=32, osr=0)
        a.update(kw)
        return lib.isc_logsoftmax_bwd_raw_filtered(*a.values(), ops.stream())
    for k in ('raw', 'out', 'tok', 'coef', 'kstar', 'gmax', 'logz', 'pm', 'ps'):
        assert call(**{k: None}) == -1, k
    assert call(ids=None) == -1 and call(ids=(C.c_void_p * 1)(None)) == -1
    for kw in (dict(B=0), dict(T=-1), dict(V=0), dict(ld_out=V - 1), dict(n=-1), dict(n=3), dict(srows=B - 1), dict(osr=B - 1),
               dict(inv_tau=0.0), dict(inv_tau=-1.0), dict(inv_tau=float('nan')), dict(inv_tau=float('inf'))):
        assert call(**kw) == -2, kw
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    assert call(n=0, pm=None, ps=None) == 0                  # the filtered term alone needs no statistics
    torch.cuda.synchronize()
    assert bool((out[:, :V] != SENT).all())
