"""fp64 references of the pointwise / scan backward kernels (csrc/backward.hip, the criteria of csrc/pointwise.hip) and
the comparison the kernel tests hold them to (tests/test_gpu_backward_kernels.py; checked on the host by
tests/test_bwd_ref_host.py).

Every reference is the operation's formula in plain torch on the CPU, written once over a dtype: evaluated in float64 it
is the reference, evaluated in float32 on the same inputs it measures what fp32 arithmetic itself loses (`err32`).  The
bound of an output is

    atol = 8 * max(err32, 2^-23 * max|ref|)

- 8 for a different summation order and the approximate exp / reciprocal instructions of the kernels.  In the float32
evaluation tanh is written the way csrc/common.h publishes it, 1 - 2 / (1 + exp(2x)), so its absolute error near 0
(~1.2e-7) is part of err32; the float64 evaluation uses torch.tanh.  Saved activations (the activated LSTM gates, beta of
the gate mix, alpha of the scan) are inputs: promoted, never recomputed."""
import torch

EPS32 = 2.0 ** -23
FACTOR = 8.0
SENTINEL = 7.25          # what the tests pre-fill rows / columns with that a kernel must not touch
F32, F64 = torch.float32, torch.float64

RATIOS = {}              # name -> (err_kernel, err32, err_kernel / max(err32, 2^-23 max|ref|)): filled by check_output
WORST = {}               # the same per output ('kernel/output', the name up to its '[case]'): the largest ratio seen


def tanh_(x):
    """float64: torch.tanh; float32: common.h's form (isc_tanh), saturating to +-1 where exp overflows."""
    if x.dtype == F64:
        return torch.tanh(x)
    return 1.0 - 2.0 / (1.0 + torch.exp(2.0 * x))


def _c(x, dt):
    return None if x is None else x.detach().cpu().to(dt)


def both(fn, *args, **kw):
    """(reference in float64, the same formula in float32) of `fn(dtype, ...)`; each a dict name -> tensor."""
    return fn(F64, *args, **kw), fn(F32, *args, **kw)


def bound(ref, ev32):
    """(atol, err32) of one output by the rule above."""
    ref = ref.to(F64)
    err32 = float((ev32.to(F64) - ref).abs().max()) if ref.numel() else 0.0
    top = float(ref.abs().max()) if ref.numel() else 0.0
    return FACTOR * max(err32, EPS32 * top), err32


def check_output(got, ref, ev32, name, rows=None, pad='zero', sentinel=SENTINEL, atol=None):
    """Hold a kernel output to its reference, element by element, layout included.

    got   [rows_total, ld] (or 1-D = one row): the whole buffer the kernel wrote into, pre-filled with `sentinel`
    ref   [n, N] float64, ev32 the float32 evaluation of the same formula (same shape)
    rows  indices of the n buffer rows the kernel owns (default: the first n); every other row must still hold the
          sentinel in every column
    pad   what columns N..ld-1 of the owned rows must hold: 'zero' (the kernel zero-fills its padding) or 'sentinel'
          (the kernel must not touch them)
    atol  overrides the rule's bound (a named project bar; never wider than the caller can justify in a comment)
    Returns err_kernel / max(err32, 2^-23 max|ref|) (<= 8 when the rule's bound holds) and records it in RATIOS."""
    got = got.detach().cpu()
    ref, ev32 = ref.detach().cpu().to(F64), ev32.detach().cpu()
    if got.dim() == 1:
        got = got.unsqueeze(0)
    if ref.dim() == 1:
        ref, ev32 = ref.unsqueeze(0), ev32.unsqueeze(0)
    got, ref, ev32 = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1), ev32.reshape(ref.shape[0], -1)
    n, N = ref.shape
    assert got.shape[0] >= n and got.shape[1] >= N, (name, tuple(got.shape), tuple(ref.shape))
    rows = torch.arange(n) if rows is None else torch.as_tensor(rows, dtype=torch.int64)
    assert rows.numel() == n and rows.unique().numel() == n, name
    own = got[rows]
    rule, err32 = bound(ref, ev32)
    tol = rule if atol is None else atol
    live = own[:, :N]
    assert bool(torch.isfinite(live).all()), (name, 'non-finite output')
    diff = (live.to(F64) - ref).abs()
    err = float(diff.max()) if diff.numel() else 0.0
    denom = rule / FACTOR
    ratio = err / denom if denom > 0 else (0.0 if err == 0 else float('inf'))
    RATIOS[name] = (err, err32, ratio)
    group = name.split('[')[0]
    if group not in WORST or ratio > WORST[group][2]:
        WORST[group] = (err, err32, ratio, name)
    print('BWDREF %-58s err_kernel %.3e  err32 %.3e  ratio %.2f' % (name, err, err32, ratio))
    if err > tol:
        i = int(diff.argmax())
        raise AssertionError('%s: |got - ref| = %.3e > %.3e at owned row %d, column %d (err32 %.3e, max|ref| %.3e)'
                             % (name, err, tol, i // N, i % N, err32, float(ref.abs().max())))
    if got.shape[1] > N:
        want = 0.0 if pad == 'zero' else sentinel
        bad = own[:, N:] != want
        assert not bool(bad.any()), '%s: padding column %d of owned row %d holds %r, not %r' % (
            name, N + int(bad.nonzero()[0, 1]), int(bad.nonzero()[0, 0]), float(own[:, N:][bad][0]), want)
    other = torch.ones(got.shape[0], dtype=torch.bool)
    other[rows] = False
    if bool(other.any()):
        bad = (got[other] != sentinel).any(dim=1)
        assert not bool(bad.any()), '%s: row %d is not the kernel\'s to write, and lost its sentinel' % (
            name, int(other.nonzero().flatten()[bad][0]))
    return ratio


# ------------------------------------------------------------------------------------------------ the formulas
def colsum_ref(dt, x, prefill=None):
    s = _c(x, dt).sum(0)
    return {'out': s if prefill is None else _c(prefill, dt) + s}


def lstm_bwd_ref(dt, dh, dh2, dc_next, gates, c_prev, c, dgates_sum=None):
    """gates [M, 4H]: the ACTIVATED (i, f, g, o) the forward saved."""
    H = c.shape[1]
    g = _c(gates, dt)
    gi, gf, gg, go = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
    d_h = _c(dh, dt) if dh2 is None else _c(dh, dt) + _c(dh2, dt)
    tc = tanh_(_c(c, dt))
    d_c = d_h * go * (1 - tc * tc)
    if dc_next is not None:
        d_c = d_c + _c(dc_next, dt)
    dg = torch.cat([d_c * gg * gi * (1 - gi), d_c * _c(c_prev, dt) * gf * (1 - gf), d_c * gi * (1 - gg * gg),
                    d_h * tc * go * (1 - go)], dim=1)
    out = {'dgates': dg, 'dc_prev': d_c * gf}
    if dgates_sum is not None:
        out['dgates_sum'] = _c(dgates_sum, dt) + dg
    return out


def gate_mix_bwd_ref(dt, z, w, v, s, beta, dfeat, dw_rows=None, db_rows=None):
    """feat = beta v + (1 - beta) s, beta = sigmoid(w . tanh(z) + b) saved; dw_rows / db_rows: what is accumulated onto."""
    z, w, v, s, bt, g = _c(z, dt), _c(w, dt).reshape(-1), _c(v, dt), _c(s, dt), _c(beta, dt).reshape(-1, 1), _c(dfeat, dt)
    du = (g * (v - s)).sum(1, keepdim=True) * bt * (1 - bt)
    t = tanh_(z)
    dw, db = du * t, du.reshape(-1)
    return {'dv': bt * g, 'ds': (1 - bt) * g, 'dz': du * w * (1 - t * t),
            'dw_rows': dw if dw_rows is None else _c(dw_rows, dt) + dw,
            'db_rows': db if db_rows is None else _c(db_rows, dt) + db}


def logsoftmax_bwd_ref(dt, logp, dense=None, sparse=(), scale=None):
    """scale * (dense + scatter - exp(logp) * tot), tot = sum_v dense + sum_j coef_j; logp [M, V] saved log-probs."""
    lp = _c(logp, dt)
    g = torch.zeros_like(lp) if dense is None else _c(dense, dt).clone()
    tot = g.sum(1, keepdim=True)
    for ids, coef in sparse:
        cf = _c(coef, dt).reshape(-1, 1)
        g.scatter_add_(1, ids.detach().cpu().reshape(-1, 1), cf)
        tot = tot + cf
    out = g - torch.exp(lp) * tot
    return {'dlogits': out if scale is None else out * float(scale)}


def logp_of_logits_ref(dt, logits):
    return {'logp': torch.log_softmax(_c(logits, dt), dim=-1)}


def raw_bwd_ref(dt, logits, sparse, scale=None):
    """The sparse log-softmax backward from RAW logits [M, V]: the log-probs are log_softmax(logits) in the same dtype."""
    return logsoftmax_bwd_ref(dt, torch.log_softmax(_c(logits, dt), dim=-1), None, sparse, scale)


def xe_loss_ref(dt, tlp, mask):
    """-sum of log p(target) over the unmasked positions."""
    return {'sum': -(_c(tlp, dt)[mask.detach().cpu()]).sum().reshape(1)}


def scan_bwd_ref(dt, P, V, q, w, alpha, dout, q2=None, dP0=None, dV0=None, dw0=None):
    """One step of the attention scan's backward: e = w . tanh(P + q (+ q2)), out = alpha V with the SAVED alpha =
    softmax(e).  float64: d alpha and dV by autograd of out = alpha V, d e by the softmax Jacobian at the saved alpha,
    dP / dq / dw by autograd of e; float32: the same derivatives written out.  dP0 / dV0 / dw0: accumulated onto."""
    P, V, w, al, do = _c(P, dt), _c(V, dt), _c(w, dt).reshape(-1), _c(alpha, dt), _c(dout, dt)
    qq = _c(q, dt) if q2 is None else _c(q, dt) + _c(q2, dt)
    if dt == F64:
        al_, V_ = al.clone().requires_grad_(True), V.clone().requires_grad_(True)
        d_al, dV = torch.autograd.grad(torch.einsum('br,brd->bd', al_, V_), (al_, V_), do)
        de = al * (d_al - (al * d_al).sum(1, keepdim=True))
        P_, q_, w_ = P.clone().requires_grad_(True), qq.clone().requires_grad_(True), w.clone().requires_grad_(True)
        wb = w_.unsqueeze(0).expand(P.shape[0], -1)                   # per-row gradient of the shared w
        wb.retain_grad()
        e = (torch.tanh(P_ + q_.unsqueeze(1)) * wb.unsqueeze(1)).sum(-1)
        e.backward(de)
        dP, dq, dw = P_.grad, q_.grad, wb.grad
    else:
        d_al = torch.einsum('bd,brd->br', do, V)
        de = al * (d_al - (al * d_al).sum(1, keepdim=True))
        dV = al.unsqueeze(-1) * do.unsqueeze(1)
        t = tanh_(P + qq.unsqueeze(1))
        dP = de.unsqueeze(-1) * w * (1 - t * t)
        dq = dP.sum(1)
        dw = (de.unsqueeze(-1) * t).sum(1)
    return {'de': de, 'dq': dq, 'dw_rows': dw if dw0 is None else _c(dw0, dt) + dw,
            'dP': dP if dP0 is None else _c(dP0, dt) + dP, 'dV': dV if dV0 is None else _c(dV0, dt) + dV}


def dv_from_alpha_ref(dt, alpha, dout_all):
    """dV[b,r,:] = sum_t alpha[b,t,r] dout[t,b,:]"""
    return {'dV': torch.einsum('btr,tbd->brd', _c(alpha, dt), _c(dout_all, dt))}


def dp_from_de_ref(dt, P, q_all, w, de_all, q2=None):
    """dP[b,r,:] = sum_t de[t,b,r] w (1 - tanh^2(P[b,r,:] + q[t,b,:] (+ q2[b,:])))"""
    P, w = _c(P, dt), _c(w, dt).reshape(-1)
    acc = torch.zeros_like(P)
    for t in range(q_all.shape[0]):
        qq = _c(q_all[t], dt) if q2 is None else _c(q_all[t], dt) + _c(q2, dt)
        th = tanh_(P + qq.unsqueeze(1))
        acc = acc + _c(de_all[t], dt).unsqueeze(-1) * w * (1 - th * th)
    return {'dP': acc}
