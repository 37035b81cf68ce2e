"""Teacher-forced XE training on n captions per image without repeating the image (`forward_xe(captions_per_image=n)`):
the scan backward with per-image P / V / q2 (isc_scan_bwd_problem.row_div), the two reductions after the sweep over the
rows of an image (isc_attn_dv_from_alpha_group / isc_attn_dp_from_de_group) and the whole call + loss + backward against
the float64 oracle on the expanded inputs and against this build's own repeated form.

Kernel tolerances: tests/_bwd_ref.py's rule, atol = 8 * max(err32, 2^-23 max|ref|) - the fp32 evaluation of a group sum
runs over the n*T terms, so err32 carries the longer sum; torch.equal where two launches run the same per-row
arithmetic.  End to end: the bars of tests/test_gpu_backward.py."""
import numpy as np
import pytest
import torch

import _bwd_ref as R
from insenticap_model_amd import Captioner, XECriterion, _lib, ops, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = R.SENTINEL
GRAD_RTOL = 1e-4   # gradients within 1e-4 relative to the tensor's max


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def d(x):
    return None if x is None else x.to(DEV)


def sent(*shape):
    return torch.full(shape, SENT, device=DEV)


# ------------------------------------------------------------------------------------------------ scan backward, row_div
def _scan_case(g, I, n, R_, A, D, with_q2):
    """Per-image P / V / q2, per-row q / alpha (a strided [B, T, R] view) / dout; everything on the device as well."""
    B = I * n
    x = dict(P=rn(g, I, R_, A), V=rn(g, I, R_, D), q=rn(g, B, A), w=rn(g, A, scale=0.3),
             q2=rn(g, I, A) if with_q2 else None, dout=rn(g, B, D))
    alpha_all = torch.softmax(rn(g, B, 3, R_), dim=-1)
    x['alpha'] = alpha_all[:, 1]
    x['dev'] = {k: d(v) for k, v in x.items()}
    x['dev']['alpha'] = d(alpha_all)[:, 1]
    x['rep'] = {k: (None if x[k] is None else d(x[k].repeat_interleave(n, 0))) for k in ('P', 'V', 'q2')}
    return x


def _scan_launch(x, n, grouped, acc, pre_dw, rows=None):
    """One problem (grouped on the per-image tensors, or plain on the repeated ones) and its whole output buffers: one
    sentinel row behind the owned rows."""
    xd, B = x['dev'], x['q'].shape[0]
    R_, A = x['P'].shape[1:]
    bufs = {'de': sent(B + 1, R_), 'dq': sent(B + 1, A), 'dw_rows': sent(B + 1, A)}
    bufs['dw_rows'][:B] = pre_dw.to(DEV)
    src = xd if grouped else x['rep']
    prob = ops.scan_bwd_problem(src['P'], src['V'], xd['q'], xd['w'], xd['alpha'], xd['dout'], None, None, bufs['dq'][:B],
                                bufs['dw_rows'][:B], acc, q2=src['q2'], de_out=bufs['de'][:B],
                                row_div=n if grouped else 1)
    if rows is not None:
        prob.rows = rows
    return prob, bufs


def _scan_check(x, n, acc, pre_dw, bufs, tag):
    P, V, q2 = (None if x[k] is None else x[k].repeat_interleave(n, 0) for k in ('P', 'V', 'q2'))
    kw = dict(dw0=pre_dw) if acc else {}
    ref, ev = R.both(R.scan_bwd_ref, P, V, x['q'], x['w'], x['alpha'], x['dout'], q2=q2, **kw)
    for k in ('de', 'dq', 'dw_rows'):
        R.check_output(bufs[k], ref[k], ev[k], 'attn_scan_bwd_group/%s%s acc%d]' % (k, tag, acc))


@pytest.mark.parametrize('I,n,R_,A,D', [(1, 2, 1, 4, 4), (3, 5, 6, 32, 32), (2, 8, 37, 64, 128), (2, 3, 196, 512, 512),
                                        (2, 4, 11, 1024, 64)])
def test_attn_scan_bwd_row_div_is_the_repeated_launch_bit_for_bit(I, n, R_, A, D):
    """row b of a grouped launch reads P / V / q2 of image b // n: d e, dq and dw_rows (accumulate 0 and 1) must be the
    plain launch's on repeat_interleave'd tensors, torch.equal - the same per-row arithmetic - and within the rule's
    bound of fp64.  q2 on the odd-R cases.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    d e 0.89, dq 1.28, dw_rows 1.41"""
    g = gen(I * 1000 + n * 100 + R_ + A + D)
    x = _scan_case(g, I, n, R_, A, D, with_q2=bool(R_ & 1))
    tag = '[%dx%dx%dx%dx%d' % (I, n, R_, A, D)
    for acc in (0, 1):
        pre_dw = rn(g, I * n, A)
        got, ref_run = [], []
        for grouped, keep in ((True, got), (False, ref_run)):
            prob, bufs = _scan_launch(x, n, grouped, acc, pre_dw)
            ops.attn_scan_bwd([prob], I * n)
            keep.append(bufs)
        for k in ('de', 'dq', 'dw_rows'):
            assert torch.equal(got[0][k], ref_run[0][k]), (k, acc)
        _scan_check(x, n, acc, pre_dw, got[0], tag)


def test_attn_scan_bwd_row_div_two_problem_launch():
    """A problem of 10 rows (2 images x 5) and a second one with q2 and fewer rows (6 = 2 images x 3, other R / A / D)
    in ONE launch: the grid spans 10 rows, the row behind the shorter problem's 6 keeps its sentinel.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8), worst case:
    d e 0.47, dq 1.47, dw_rows 0.82"""
    g = gen(77)
    xa = _scan_case(g, 2, 5, 6, 32, 32, False)
    xb = _scan_case(g, 2, 3, 9, 64, 16, True)
    pa, ba = _scan_launch(xa, 5, True, 0, torch.zeros(10, 32))
    pb, bb = _scan_launch(xb, 3, True, 0, torch.zeros(6, 64), rows=6)
    ops.attn_scan_bwd([pa, pb], 10)
    _scan_check(xa, 5, 0, None, ba, '[two-problem A')
    _scan_check(xb, 3, 0, None, bb, '[two-problem B')
    # the plain launch of each problem on repeated tensors: the same bits
    for x, n, bufs in ((xa, 5, ba), (xb, 3, bb)):
        prob, plain = _scan_launch(x, n, False, 0, torch.zeros(x['q'].shape[0], x['P'].shape[2]))
        ops.attn_scan_bwd([prob], x['q'].shape[0])
        for k in ('de', 'dq', 'dw_rows'):
            assert torch.equal(bufs[k][:x['q'].shape[0]], plain[k][:x['q'].shape[0]]), k


def test_attn_scan_bwd_row_div_refusals_leave_the_buffers_alone():
    """row_div > 1 with a dP or a dV to accumulate into (n workgroups would read-modify-write one image's entry), and
    rows % row_div != 0: ISC_E_SHAPE from the entry point's checks, nothing launched - every buffer keeps its sentinel."""
    lib, g = _lib.load(), gen(9)
    x = _scan_case(g, 2, 3, 5, 32, 32, True)

    def rc_of(dP=False, dV=False, rows=None):
        prob, bufs = _scan_launch(x, 3, True, 0, torch.full((6, 32), SENT), rows=rows)
        big = {'dP': sent(2, 5, 32), 'dV': sent(2, 5, 32)}
        prob.dP = big['dP'].data_ptr() if dP else None
        prob.dV = big['dV'].data_ptr() if dV else None
        rc = lib.isc_attn_scan_bwd((_lib.ScanBwdProblem * 1)(prob), 1, 6, ops.stream())
        torch.cuda.synchronize()
        if rc != 0:
            for b in list(bufs.values()) + list(big.values()):
                assert bool((b == SENT).all())
        return rc
    assert rc_of(dP=True) == -2
    assert rc_of(dV=True) == -2
    assert rc_of(rows=5) == -2
    assert rc_of(rows=4) == -2
    assert rc_of() == 0                      # (the same problem without them: runs)


# ------------------------------------------------------------------------------------------------ the two group reductions
@pytest.mark.parametrize('B,T,R_,D,extra', [(2, 5, 7, 1028, 0), (3, 4, 5, 12, 0), (3, 6, 11, 32, 2), (1, 25, 700, 32, 0)],
                         ids=['second_column_block', 'three_float4', 'step_rows', 'r700'])
def test_attn_dv_group_of_one_is_the_old_entry_point(B, T, R_, D, extra):
    """group = 1 through ops against isc_attn_dv_from_alpha itself (ctypes): torch.equal, on the shapes of
    test_attn_dv_from_alpha_edges_vs_fp64."""
    g = gen(B + T + R_ + D)
    alpha = d(torch.softmax(rn(g, B, T, R_ + 3), dim=-1))[:, :, :R_]
    big = d(rn(g, T, B + extra, D))
    a, b = sent(B + 1, R_, D), sent(B + 1, R_, D)
    ops.attn_dv_from_alpha(alpha, big[:, :B], a[:B], step_rows=B + extra if extra else 0, group=1)
    rc = _lib.load().isc_attn_dv_from_alpha(alpha.data_ptr(), alpha.stride(0), alpha.stride(1), big.data_ptr(), B, T, R_, D,
                                            b.data_ptr(), B + extra if extra else 0, ops.stream())
    assert rc == 0 and torch.equal(a, b) and bool((a[B:] == SENT).all())


@pytest.mark.parametrize('B,T,R_,A,with_q2', [(2, 5, 7, 1028, True), (3, 4, 5, 12, False), (1, 25, 700, 32, True)],
                         ids=['second_column_block', 'three_float4', 'r700'])
def test_attn_dp_group_of_one_is_the_old_entry_point(B, T, R_, A, with_q2):
    """group = 1 through ops against isc_attn_dp_from_de itself (ctypes): torch.equal, on the shapes of
    test_attn_dp_from_de_edges_vs_fp64."""
    g = gen(B + T + R_ + A + 1)
    P, q, w, de = d(rn(g, B, R_, A)), d(rn(g, T, B, A)), d(rn(g, A, scale=0.3)), d(rn(g, T, B, R_, scale=0.1))
    q2 = d(rn(g, B, A)) if with_q2 else None
    a, b = sent(B + 1, R_, A), sent(B + 1, R_, A)
    ops.attn_dp_from_de(P, q, w, de, a[:B], q2=q2, group=1)
    rc = _lib.load().isc_attn_dp_from_de(P.data_ptr(), q.data_ptr(), ops.ptr(q2), w.data_ptr(), de.data_ptr(), B, T, R_, A,
                                         b.data_ptr(), ops.stream())
    assert rc == 0 and torch.equal(a, b) and bool((a[B:] == SENT).all())


GROUP_SHAPES = [(2, 2, 5, 7, 1028, 0), (3, 5, 4, 5, 12, 0), (3, 3, 6, 11, 32, 2), (1, 7, 25, 200, 32, 0),
                (1, 2, 20, 36, 512, 0)]
GROUP_IDS = ['second_column_block', 'three_float4', 'step_rows', 'nT175_chunks', 'workload_rows']


def _group_sum64(per_row, I, n):
    """The per-row reference [I*n, ...] summed over each image's rows, in the reference's own dtype."""
    return per_row.reshape(I, n, *per_row.shape[1:]).sum(1)


@pytest.mark.parametrize('I,n,T,R_,D,extra', GROUP_SHAPES, ids=GROUP_IDS)
def test_attn_dv_from_alpha_group_vs_fp64(I, n, T, R_, D, extra):
    """dV[i] = sum_j sum_t alpha[i*n + j, t] x dout[t, i*n + j] against the per-row fp64 reference summed over the group
    (the fp32 evaluation sums the same n*T terms: err32 carries the longer sum).  D = 1028: a second column block of one
    float4; D = 12; dout as rows of a [T, I*n + 2, D] stack; n*T = 175 with 200 regions: past the unrolled form, several
    region chunks; (1, 2, 20, 36, 512): the workload's row geometry.  One spare image behind the output keeps its
    sentinel; a second call gives the same bits.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8):
    dV 1.19, 0.92, 1.25, 2.76, 1.47 in the order of the cases"""
    g = gen(I + n + T + R_ + D)
    B = I * n
    alpha_w = torch.softmax(rn(g, B, T, R_ + 3), dim=-1)
    alpha = alpha_w[:, :, :R_]
    big = rn(g, T, B + extra, D)
    ad, bd = d(alpha_w)[:, :, :R_], d(big)[:, :B]
    dV, dV2 = sent(I + 1, R_, D), sent(I + 1, R_, D)
    for out in (dV, dV2):
        ops.attn_dv_from_alpha(ad, bd, out[:I], step_rows=B + extra if extra else 0, group=n)
    assert torch.equal(dV, dV2)
    ref, ev = R.both(R.dv_from_alpha_ref, alpha, big[:, :B])
    R.check_output(dV, _group_sum64(ref['dV'], I, n), _group_sum64(ev['dV'], I, n),
                   'attn_dv_from_alpha_group/dV[%dx%dx%dx%dx%d rows+%d]' % (I, n, T, R_, D, extra))


@pytest.mark.parametrize('I,n,T,R_,A,extra', GROUP_SHAPES, ids=GROUP_IDS)
def test_attn_dp_from_de_group_vs_fp64(I, n, T, R_, A, extra):
    """dP[i] = sum_j sum_t de[t, i*n + j] w (1 - tanh^2(P[i] + q[t, i*n + j] (+ q2[i]))) against the per-row fp64
    reference on the expanded P / q2, summed over the group; q2 on two of the cases.  One spare image behind the output
    keeps its sentinel; a second call gives the same bits.
    err_kernel / max(err32, 2^-23 max|ref|) measured on an MI355X (the bound is 8):
    dP 0.86, 0.82, 1.44, 1.78, 1.00 in the order of the cases"""
    g = gen(I + n + T + R_ + A + 1)
    B = I * n
    with_q2 = extra == 0 and A in (1028, 32)
    P, q, w, de = rn(g, I, R_, A), rn(g, T, B, A), rn(g, A, scale=0.3), rn(g, T, B, R_, scale=0.1)
    q2 = rn(g, I, A) if with_q2 else None
    Pd, qd, wd, ded, q2d = d(P), d(q), d(w), d(de), d(q2)
    dP, dP2 = sent(I + 1, R_, A), sent(I + 1, R_, A)
    for out in (dP, dP2):
        ops.attn_dp_from_de(Pd, qd, wd, ded, out[:I], q2=q2d, group=n)
    assert torch.equal(dP, dP2)
    ref, ev = R.both(R.dp_from_de_ref, P.repeat_interleave(n, 0), q, w, de,
                     q2=None if q2 is None else q2.repeat_interleave(n, 0))
    R.check_output(dP, _group_sum64(ref['dP'], I, n), _group_sum64(ev['dP'], I, n),
                   'attn_dp_from_de_group/dP[%dx%dx%dx%dx%d q2=%d]' % (I, n, T, R_, A, with_q2))


def test_group_reductions_follow_the_documented_order_of_additions():
    """j ascending outermost, t = T-1 down inside: the group result is, bit for bit, the per-row sweep accumulating into
    ONE image's dV / dP - row 0's steps T-1 .. 0, then row 1's, ... (attn_scan_bwd with accumulate, one row at a time)."""
    g = gen(31)
    n, T, R_, A = 3, 4, 6, 32
    P, V, w = d(rn(g, 1, R_, A)), d(rn(g, 1, R_, A)), d(rn(g, A, scale=0.3))
    q, dout = d(rn(g, T, n, A)), d(rn(g, T, n, A))
    alpha = d(torch.softmax(rn(g, n, T, R_), dim=-1))
    dP, dV = sent(1, R_, A), sent(1, R_, A)
    de, dq, dw = sent(T, n, R_), sent(T, n, A), sent(n, A)
    first = True
    for j in range(n):
        for t in range(T - 1, -1, -1):
            ops.attn_scan_bwd([ops.scan_bwd_problem(P, V, q[t, j:j + 1], w, alpha[j:j + 1, t], dout[t, j:j + 1], dP, dV,
                                                    dq[t, j:j + 1], dw[j:j + 1], not first, de_out=de[t, j:j + 1])], 1)
            first = False
    dV2, dP2 = sent(1, R_, A), sent(1, R_, A)
    ops.attn_dv_from_alpha(alpha, dout, dV2, group=n)
    ops.attn_dp_from_de(P, q, w, de, dP2, group=n)
    assert torch.equal(dV2, dV) and torch.equal(dP2, dP)


def test_group_reductions_refuse_more_terms_than_the_lds_holds():
    """n*T beyond the 15000 (row, step) pairs that 60000 bytes hold for one region, and rows that are no multiple of the
    group: ISC_E_SHAPE as the library's error through ops, nothing launched - the outputs keep their sentinels."""
    n, T = 4, 3751
    assert n * T > 15000 >= (n - 1) * T
    B = n
    alpha, dout = torch.zeros(B, T, 1, device=DEV), torch.zeros(T, B, 4, device=DEV)
    dV, dP = sent(1, 1, 4), sent(1, 1, 4)
    with pytest.raises(_lib.HipLibraryError):
        ops.attn_dv_from_alpha(alpha, dout, dV, group=n)
    with pytest.raises(_lib.HipLibraryError):
        ops.attn_dp_from_de(torch.zeros(1, 1, 4, device=DEV), torch.zeros(T, B, 4, device=DEV),
                            torch.zeros(4, device=DEV), torch.zeros(T, B, 1, device=DEV), dP, group=n)
    lib = _lib.load()
    assert lib.isc_attn_dv_from_alpha_group(alpha.data_ptr(), T, 1, dout.data_ptr(), 4, 3, 2, 1, 4, dV.data_ptr(), 0,
                                            ops.stream()) == -2
    assert lib.isc_attn_dp_from_de_group(dP.data_ptr(), dout.data_ptr(), None, dout.data_ptr(), alpha.data_ptr(), 4, 3, 2,
                                         1, 4, dP.data_ptr(), ops.stream()) == -2
    torch.cuda.synchronize()
    assert bool((dV == SENT).all()) and bool((dP == SENT).all())


# ------------------------------------------------------------------------------------------------ end to end
def _captioner(w, V, st, train):
    cap = Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)
    cap.load_state_dict({k: torch.from_numpy(x) for k, x in w.items()})
    cap.to(DEV)
    cap.train(train)
    return cap


def _group_batch(I, n, V, st, R_, T, seed):
    """Features / concept words of I images and captions / labels of I*n image-major rows (unsorted lengths; the
    labels differ inside an image)."""
    img = synth.make_inputs(I, V, st, regions=R_, seq_len=T, seed=seed)
    row = synth.make_inputs(I * n, V, st, regions=1, seq_len=T, seed=seed + 1)
    row['senti_labels'][:2] = (0, 1)                 # (two captions of image 0 with different labels)
    return dict(fc_feats=img['fc_feats'], att_feats=img['att_feats'], cpt_words=img['cpt_words'],
                captions=row['captions'], lengths=[int(x) for x in row['lengths']], senti_labels=row['senti_labels'],
                image_labels=img['senti_labels'])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _hip_run(cap, b, n, labels, masks=None, grouped=True, ss_prob=0.0):
    """forward_xe + XE loss + domain-alignment loss + backward.  grouped: captions_per_image = n on the per-image
    inputs; else the plain call on inputs (and per-image masks) repeated n times."""
    rep = (lambda x: x) if grouped else (lambda x: x.repeat_interleave(n, 0))
    m = masks
    if masks is not None and not grouped:
        I, R_ = b['att_feats'].shape[:2]
        m = dict(masks, fc=masks['fc'].repeat_interleave(n, 0),
                 att=masks['att'].view(I, R_, -1).repeat_interleave(n, 0).reshape(I * n * R_, -1))
    if not grouped and labels.shape[0] != b['captions'].shape[0]:
        labels = labels.repeat_interleave(n, 0)
    kw = dict(captions_per_image=n) if grouped else {}
    cap.zero_grad()
    pred = cap.forward_xe(rep(_dev(b['fc_feats'])), rep(_dev(b['att_feats'])), rep(_dev(b['cpt_words'])),
                          _dev(b['captions']), labels.to(DEV), ss_prob, _masks=m, **kw)
    xe = XECriterion()(pred, _dev(b['captions'])[:, 1:], b['lengths'])
    da = torch.nn.MSELoss()(cap.cpt_feats, cap.fc_feats.detach())
    (xe + da).backward()
    grads = {k: q.grad.detach().cpu().numpy().copy() for k, q in cap.named_parameters() if q.grad is not None}
    return pred.detach().cpu().numpy(), (float(xe.detach()), float(da.detach())), grads, tuple(cap.fc_feats.shape)


def _oracle_run(w, V, b, n, labels, masks, p_drop):
    """The oracle with float64 parameters and autograd on the EXPANDED inputs (per-image masks repeated)."""
    from oracle import captioner_oracle as O
    p = O.to_params(w, dtype=torch.float64, requires_grad=True)
    ids = O.Ids(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES)
    I, R_ = b['att_feats'].shape[:2]
    rep = lambda a: torch.from_numpy(np.ascontiguousarray(a)).repeat_interleave(n, 0)
    if labels.shape[0] == I:
        labels = labels.repeat_interleave(n, 0)
    om = None
    if masks is not None:
        T = b['captions'].shape[1] - 1
        om = dict(fc=masks['fc'].repeat_interleave(n, 0), att=masks['att'].view(I, R_, -1).repeat_interleave(n, 0),
                  label=masks['label'], out=torch.stack([masks['out%d' % t] for t in range(T)]))
    caps = torch.from_numpy(b['captions'])
    logp, P, _ = O.forward_xe(p, ids, rep(b['fc_feats']).double(), rep(b['att_feats']).double(), rep(b['cpt_words']),
                              caps, labels, masks=om, p_drop=p_drop)
    xe = O.xe_criterion(logp, caps[:, 1:], b['lengths'])
    da = O.domain_align_loss(P.cpt, P.fc_raw)
    (xe + da).backward()
    return logp.detach().numpy(), (float(xe.detach()), float(da.detach())), {k: q.grad.numpy() for k, q in p.items() if q.grad is not None}


def _compare(got, ref, what):
    (lp, losses, grads, _), (rlp, rlosses, rgrads) = got, ref[:3]
    np.testing.assert_allclose(lp, rlp, atol=1e-4, err_msg=what)
    np.testing.assert_allclose(losses, rlosses, rtol=2e-5, err_msg=what)
    n = 0
    for k, r in rgrads.items():
        assert k in grads, (what, k)
        np.testing.assert_allclose(grads[k], r, atol=GRAD_RTOL * np.abs(r).max() + 1e-7, err_msg='%s %s' % (what, k))
        n += 1
    assert n >= 20 and set(grads) == set(rgrads), what


@pytest.mark.parametrize('mode', [1, 0], ids=['split_f16', 'exact_fp32'])
@pytest.mark.parametrize('n', [2, 5])
def test_grouped_xe_tiny_vs_float64_oracle_on_the_expanded_inputs(n, mode):
    """'tiny' settings, V = 64, I = 3, R = 6, T = 8, both GEMM engines: log-probs within 1e-4, XE and domain-alignment
    losses within rtol 2e-5 and every parameter gradient within GRAD_RTOL * max|ref| + 1e-7 of the oracle's float64
    autograd on the expanded inputs - with dropout off and in training mode with explicit masks (per-image masks 'fc'
    [I,E] and 'att' [I*R,E], repeated for the oracle; 'label' and 'out<t>' per row), each with per-caption labels that
    differ inside an image and with per-image labels.  The XE + domain-alignment total exercises the [I, E] attribute
    gradients."""
    V, I, R_, T, st = 64, 3, 6, 8, synth.TINY_SETTINGS
    w = synth.make_weights(V, st, seed=3)
    b = _group_batch(I, n, V, st, R_, T, seed=50 + n)
    E, H, Wd, p_drop = st['feat_emb_dim'], st['rnn_hid_dim'], st['word_emb_dim'], st['dropout_p']
    g = gen(n)
    keep = lambda *shape: (torch.rand(*shape, generator=g) >= p_drop).to(torch.uint8)
    masks = dict(fc=keep(I, E), att=keep(I * R_, E), label=keep(I * n, Wd), **{'out%d' % t: keep(I * n, H) for t in range(T)})
    prev = ops.h3_mode()
    ops.set_h3_mode(mode)
    try:
        for train, m in ((False, None), (True, masks)):
            cap = _captioner(w, V, st, train)
            for lab in ('senti_labels', 'image_labels'):
                labels = torch.from_numpy(b[lab])
                assert labels.shape[0] == (I * n if lab == 'senti_labels' else I)
                got = _hip_run(cap, b, n, labels, m)
                assert got[0].shape == (I * n, T, V) and got[3] == (I, E)
                _compare(got, _oracle_run(w, V, b, n, labels, m, p_drop), 'n=%d train=%d %s' % (n, train, lab))
    finally:
        ops.set_h3_mode(prev)


@pytest.mark.parametrize('I,n,R_', [(2, 5, 36), (2, 3, 196)], ids=['36_regions', '196_regions'])
def test_grouped_xe_default_dims_vs_the_repeated_form(I, n, R_):
    """Default dimensions, V = 10000, T = 20: the grouped call against this build's own repeated call (dropout off) at
    the same bars, and the grouped call's peak device memory below the repeated call's."""
    V, T, st = 10000, 20, synth.DEFAULT_SETTINGS
    w = synth.make_weights(V, st, seed=5)
    b = _group_batch(I, n, V, st, R_, T, seed=70 + n)
    cap = _captioner(w, V, st, False)
    labels = torch.from_numpy(b['senti_labels'])
    peak = {}
    runs = {}
    for grouped in (False, True):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        runs[grouped] = _hip_run(cap, b, n, labels, None, grouped=grouped)
        torch.cuda.synchronize()
        peak[grouped] = torch.cuda.max_memory_allocated()
    print('GROUPXE peak bytes grouped %d repeated %d' % (peak[True], peak[False]))
    _compare(runs[True], runs[False], 'I=%d n=%d R=%d' % (I, n, R_))
    assert peak[True] < peak[False]


def test_grouped_xe_under_token_logprobs_and_row_counts_is_the_full_unroll():
    """Inside token_logprobs() the call returns [I*n, T]; an active row_counts(...) is ignored (the rows are not sorted
    by length): same loss and gradients as the plain grouped call, bit for bit."""
    V, I, n, R_, T, st = 64, 3, 2, 6, 8, synth.TINY_SETTINGS
    w = synth.make_weights(V, st, seed=3)
    b = _group_batch(I, n, V, st, R_, T, seed=11)
    cap = _captioner(w, V, st, False)
    cap.ragged_unroll = True
    labels = torch.from_numpy(b['senti_labels'])
    plain = _hip_run(cap, b, n, labels)
    cap.zero_grad()
    with cap.token_logprobs(), cap.row_counts(sorted(b['lengths'], reverse=True)):
        tlp = cap(_dev(b['fc_feats']), _dev(b['att_feats']), _dev(b['cpt_words']), _dev(b['captions']), labels.to(DEV), 0.0,
                  mode='xe', captions_per_image=n)
    assert tuple(tlp.shape) == (I * n, T)
    xe = XECriterion()(tlp, _dev(b['captions'])[:, 1:], b['lengths'])
    (xe + torch.nn.MSELoss()(cap.cpt_feats, cap.fc_feats.detach())).backward()
    np.testing.assert_allclose(float(xe.detach()), plain[1][0], rtol=2e-6)
    for k, q in cap.named_parameters():
        if q.grad is not None:
            r = plain[2][k]
            np.testing.assert_allclose(q.grad.cpu().numpy(), r, atol=GRAD_RTOL * np.abs(r).max() + 1e-7, err_msg=k)


def test_grouped_xe_without_gradients_matches_the_float64_oracle():
    """Under torch.no_grad() (the per-step inference unroll) the grouped call returns the [I*n, T, V] log-probs of the
    oracle on the expanded inputs within the project's 1e-4, and leaves [I, E] attributes."""
    V, I, n, R_, T, st = 64, 3, 5, 6, 8, synth.TINY_SETTINGS
    w = synth.make_weights(V, st, seed=3)
    b = _group_batch(I, n, V, st, R_, T, seed=41)
    cap = _captioner(w, V, st, False)
    labels = torch.from_numpy(b['senti_labels'])
    with torch.no_grad():
        pred = cap.forward_xe(_dev(b['fc_feats']), _dev(b['att_feats']), _dev(b['cpt_words']), _dev(b['captions']),
                              labels.to(DEV), 0.0, captions_per_image=n)
    assert tuple(pred.shape) == (I * n, T, V) and tuple(cap.fc_feats.shape) == (I, st['feat_emb_dim'])
    ref = _oracle_run(w, V, b, n, labels, None, st['dropout_p'])[0]
    np.testing.assert_allclose(pred.cpu().numpy(), ref, atol=1e-4)


def test_grouped_xe_scheduled_sampling_is_finite_and_repeatable():
    """ss_prob = 0.25 in training mode under a seeded generator: finite loss and gradients, bit-identical over two
    seeded runs (parity with the repeated form is not demanded: a near-tie draw may differ between the two forms)."""
    V, I, n, R_, T, st = 64, 3, 5, 6, 8, synth.TINY_SETTINGS
    w = synth.make_weights(V, st, seed=3)
    b = _group_batch(I, n, V, st, R_, T, seed=21)
    cap = _captioner(w, V, st, True)
    labels = torch.from_numpy(b['senti_labels'])
    runs = []
    for _ in range(2):
        torch.manual_seed(1234)
        torch.cuda.manual_seed_all(1234)
        runs.append(_hip_run(cap, b, n, labels, ss_prob=0.25))
    assert all(np.isfinite(x) for x in runs[0][1])
    for k, gk in runs[0][2].items():
        assert np.isfinite(gk).all(), k
        assert np.array_equal(gk, runs[1][2][k]), k
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


def test_zz_report_the_measured_ratios():
    """Prints the worst err_kernel / max(err32, 2^-23 max|ref|) per output of this file's kernel tests (pytest -s)."""
    for k in sorted(R.WORST):
        if 'group' in k:
            err, err32, ratio, name = R.WORST[k]
            print('WORST %-40s ratio %.2f  (%s)' % (k, ratio, name))
            assert ratio <= R.FACTOR
