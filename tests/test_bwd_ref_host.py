"""The helper the backward-kernel tests stand on (tests/_bwd_ref.py), on the host: the float32 evaluation of every
reference passes its own bound, the float64 scan reference (autograd) agrees with the derivatives written out, and the
comparison function can fail - one defect at a time, each of the kinds a kernel produces: a tail column, a last row, an
element on a 64-column / 256-row boundary, a padding column, a row that belongs to somebody else."""
import pytest
import torch

import _bwd_ref as R


def _rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _case(rows=300, N=130, ld=135, extra_rows=2, seed=0):
    """A [rows, N] output inside a [rows + extra_rows, ld] buffer: reference, float32 evaluation, and the buffer as a
    correct kernel leaves it (zero padding columns, untouched sentinel rows)."""
    g = torch.Generator().manual_seed(seed)
    x, w, d = _rn(g, rows, N), _rn(g, N, scale=0.3), _rn(g, rows, 1)

    def f(dt):
        t = R.tanh_(x.to(dt))
        return d.to(dt) * w.to(dt) * (1 - t * t)
    ref, ev32 = f(R.F64), f(R.F32)
    buf = torch.full((rows + extra_rows, ld), R.SENTINEL)
    buf[:rows, :N] = ev32
    buf[:rows, N:] = 0.0
    return buf, ref, ev32


def test_fp32_evaluation_passes_and_reports_ratio_one():
    buf, ref, ev32 = _case()
    ratio = R.check_output(buf, ref, ev32, 'host/clean')
    assert 0.0 < ratio <= 1.0
    atol, err32 = R.bound(ref, ev32)
    assert atol == R.FACTOR * max(err32, R.EPS32 * float(ref.abs().max())) and err32 > 0.0
    # an exact output: the floor 2^-23 max|ref| keeps the bound positive
    atol0, err0 = R.bound(ref, ref)
    assert err0 == 0.0 and atol0 == R.FACTOR * R.EPS32 * float(ref.abs().max())


DEFECTS = {
    'last_column': lambda b, top: b[:300, 129].add_(1e-3 * top),
    'last_column_one_element': lambda b, top: b[17, 129:130].add_(1e-3 * top),
    'last_row': lambda b, top: b[299, :130].add_(1e-3 * top),
    'last_row_one_element': lambda b, top: b[299, 5:6].add_(1e-3 * top),
    'column_64_boundary': lambda b, top: b[10, 64:65].add_(1e-3 * top),
    'column_63_boundary': lambda b, top: b[10, 63:64].sub_(1e-3 * top),
    'row_256_boundary': lambda b, top: b[256, 3:4].add_(1e-3 * top),
    'row_255_boundary': lambda b, top: b[255, 3:4].sub_(1e-3 * top),
    'padding_column_nonzero': lambda b, top: b[299, 134:135].fill_(1e-30),
    'padding_column_holds_sentinel': lambda b, top: b[0, 130:131].fill_(R.SENTINEL),
    'sentinel_row_overwritten': lambda b, top: b[301, 0:1].fill_(0.0),
    'sentinel_row_overwritten_in_padding': lambda b, top: b[300, 134:135].fill_(0.0),
    'nan': lambda b, top: b[100, 100:101].fill_(float('nan')),
}


@pytest.mark.parametrize('kind', sorted(DEFECTS))
def test_every_single_defect_raises(kind):
    buf, ref, ev32 = _case()
    DEFECTS[kind](buf, float(ref.abs().max()))
    with pytest.raises(AssertionError):
        R.check_output(buf, ref, ev32, 'host/' + kind)


def test_scattered_rows_and_untouched_padding():
    """rows=: a time-major output with sibling rows in between; pad='sentinel': columns the kernel must leave alone."""
    _, ref, ev32 = _case(rows=6, N=10)
    rows = [0, 1, 2, 5, 6, 7]                                  # 3 rows per step of 5
    buf = torch.full((10, 13), R.SENTINEL)
    buf[rows, :10] = ev32
    R.check_output(buf, ref, ev32, 'host/scattered', rows=rows, pad='sentinel')
    with pytest.raises(AssertionError):                        # zero padding where nothing may be written
        R.check_output(buf, ref, ev32, 'host/scattered', rows=rows, pad='zero')
    bad = buf.clone()
    bad[3, 2] = 0.0                                            # a sibling row written
    with pytest.raises(AssertionError):
        R.check_output(bad, ref, ev32, 'host/scattered', rows=rows, pad='sentinel')
    swapped = buf.clone()
    swapped[[5, 6]] = buf[[6, 5]]                              # right values, wrong rows
    with pytest.raises(AssertionError):
        R.check_output(swapped, ref, ev32, 'host/scattered', rows=rows, pad='sentinel')
    with pytest.raises(AssertionError):                        # a tail element, 1-D form
        R.check_output(ev32[0] + torch.tensor([0.0] * 9 + [1e-3]), ref[0], ev32[0], 'host/1d')
    R.check_output(ev32[0], ref[0], ev32[0], 'host/1d')


def test_tanh_of_the_float32_evaluation_is_the_published_form():
    x = torch.tensor([-50.0, -8.0, -1e-4, 0.0, 1e-4, 3.0, 8.0, 44.5, 50.0])
    t = R.tanh_(x)
    assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    assert t[0] == -1.0 and t[-1] == 1.0 and t[-2] == 1.0 and t[3] == 0.0
    assert float((t.double() - torch.tanh(x.double())).abs().max()) < 3e-7
    assert torch.equal(R.tanh_(x.double()), torch.tanh(x.double()))


def _inputs(seed=1, B=3, R_=7, A=8, D=12, T=4, M=5, H=6, V=11):
    g = torch.Generator().manual_seed(seed)
    return dict(
        colsum=(R.colsum_ref, (_rn(g, 37, 9),), dict(prefill=_rn(g, 9))),
        lstm=(R.lstm_bwd_ref, (_rn(g, M, H), _rn(g, M, H), _rn(g, M, H),
                               torch.cat([torch.sigmoid(_rn(g, M, 2 * H)), torch.tanh(_rn(g, M, H)),
                                          torch.sigmoid(_rn(g, M, H))], 1), _rn(g, M, H),
                               torch.cat([_rn(g, M - 1, H, scale=4.0), torch.tensor([[50.0, -50.0] * (H // 2)])])),
              dict(dgates_sum=_rn(g, M, 4 * H))),
        gate=(R.gate_mix_bwd_ref, (_rn(g, B, A), _rn(g, A, scale=0.3), _rn(g, B, D), _rn(g, B, D),
                                   torch.sigmoid(_rn(g, B)), _rn(g, B, D)), dict(dw_rows=_rn(g, B, A), db_rows=_rn(g, B))),
        lsm=(R.logsoftmax_bwd_ref, (torch.log_softmax(_rn(g, M, V, scale=3.0), -1),),
             dict(dense=_rn(g, M, V), sparse=[(torch.randint(0, V, (M,), generator=g), _rn(g, M)),
                                              (torch.randint(0, V, (M,), generator=g), _rn(g, M))], scale=128.0)),
        scan=(R.scan_bwd_ref, (_rn(g, B, R_, A), _rn(g, B, R_, D), _rn(g, B, A), _rn(g, A, scale=0.3),
                               torch.softmax(_rn(g, B, R_), -1), _rn(g, B, D)),
              dict(q2=_rn(g, B, A), dP0=_rn(g, B, R_, A), dV0=_rn(g, B, R_, D), dw0=_rn(g, B, A))),
        dv=(R.dv_from_alpha_ref, (torch.softmax(_rn(g, B, T, R_), -1), _rn(g, T, B, D)), {}),
        dp=(R.dp_from_de_ref, (_rn(g, B, R_, A), _rn(g, T, B, A), _rn(g, A, scale=0.3), _rn(g, T, B, R_)),
            dict(q2=_rn(g, B, A))),
    )


@pytest.mark.parametrize('which', ['colsum', 'lstm', 'gate', 'lsm', 'scan', 'dv', 'dp'])
def test_float32_evaluation_of_every_reference_passes_its_own_bound(which):
    fn, args, kw = _inputs()[which]
    ref, ev32 = R.both(fn, *args, **kw)
    assert ref.keys() == ev32.keys()
    for k in ref:
        assert ref[k].dtype == torch.float64 and ev32[k].dtype == torch.float32 and ref[k].shape == ev32[k].shape
        assert R.check_output(ev32[k], ref[k], ev32[k], 'host/%s/%s' % (which, k)) <= 1.0
        bad = ev32[k].clone()
        bad.view(-1)[-1] += 1e-3 * float(ref[k].abs().max()) + 1e-6
        with pytest.raises(AssertionError):
            R.check_output(bad, ref[k], ev32[k], 'host/%s/%s' % (which, k))


def test_scan_reference_autograd_equals_the_derivatives_written_out():
    """float64 takes autograd, float32 the closed forms: evaluate the closed forms in float64 too (tanh_ is torch.tanh
    there) and the two must agree to float64 rounding; saturated LSTM rows give an exactly zero tanh term."""
    fn, args, kw = _inputs()['scan']
    ref = fn(R.F64, *args, **kw)
    P, V, q, w, al, do = [a.double() for a in args]
    qq = q + kw['q2'].double()
    d_al = torch.einsum('bd,brd->br', do, V)
    de = al * (d_al - (al * d_al).sum(1, keepdim=True))
    t = torch.tanh(P + qq.unsqueeze(1))
    dP = de.unsqueeze(-1) * w * (1 - t * t)
    for k, v in (('de', de), ('dq', dP.sum(1)), ('dP', kw['dP0'].double() + dP),
                 ('dw_rows', kw['dw0'].double() + (de.unsqueeze(-1) * t).sum(1)),
                 ('dV', kw['dV0'].double() + al.unsqueeze(-1) * do.unsqueeze(1))):
        assert float((ref[k] - v).abs().max()) <= 1e-13 * max(1.0, float(v.abs().max())), k
    fn, args, kw = _inputs()['lstm']
    for dt in (R.F64, R.F32):
        out = fn(dt, args[0], args[1], None, *args[3:])
        assert bool((out['dc_prev'][-1] == 0).all()) and bool(torch.isfinite(out['dgates']).all())
