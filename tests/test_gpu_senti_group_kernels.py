"""Two-level grouping of the decode step (isc_step_plan.senti_div / isc_rows_ext.senti_div), kernel by kernel.

Rows come as images x row_div; inside an image they come in label groups of senti_div rows.  The content-side tensors
(att_p, att_e, gate_Gc) hold one entry per image, the sentiment-side tensors (pre1, label_w, words_ids, per-row words_p /
words_e / gate_Gs) one per label group.  The design rule of the grouped scan is the test: every output of every kernel is,
per row, BIT FOR BIT what the same entry point writes for the tensors expanded to one entry per row (torch.equal).
Where the project counts launches (isc_rows_launches) the route is asserted by the counter.  pytest -m gpu."""
import ctypes as C
import gc

import pytest
import torch

import _widths as Wd
from insenticap_model_amd import Captioner, _lib, ops, synth
from insenticap_model_amd.captioner import _Pro

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
E_SHAPE = -2


def _rand(g, *shape, scale=1.0):
    return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(DEV)


def _n():
    return ops._lib.load().isc_rows_launches()


def _rep(x, n):
    return x.repeat_interleave(n, 0).contiguous()


# ------------------------------------------------------------------ isc_attn_scan_gate_fwd
def _gate_case(g, images, dc, ds, R, Mw, A, gather):
    """Random operands of one gated scan: content entries per image, sentiment entries per label group."""
    rows, groups, Vt = images * dc, images * dc // ds, 50
    t = dict(Pc=_rand(g, images, R, A), Vc=_rand(g, images, R, A), Gc=_rand(g, images, R, A),
             qa=_rand(g, rows, A), qw=_rand(g, rows, A), q2=_rand(g, groups, A), zh=_rand(g, rows, A),
             wc=_rand(g, A), ws=_rand(g, A), bc=_rand(g, 1), bs=_rand(g, 1), b_gc=_rand(g, A), b_gs=_rand(g, A),
             wg=_rand(g, A), bg=_rand(g, 1))
    if gather:
        t.update(Ps=_rand(g, Vt, A), Vs=_rand(g, Vt, A), Gs=_rand(g, Vt, A),
                 ids=torch.randint(0, Vt, (groups, Mw), generator=g).to(DEV))
    else:
        t.update(Ps=_rand(g, groups, Mw, A), Vs=_rand(g, groups, Mw, A), Gs=_rand(g, groups, Mw, A), ids=None)
    return t, rows


def _gate_run(t, rows, dc, ds, R, Mw, A, expanded):
    """One isc_attn_scan_gate_fwd launch: on the grouped tensors with the two divisors, or on their expansions."""
    if expanded:
        Pc, Vc, Gc, q2 = _rep(t['Pc'], dc), _rep(t['Vc'], dc), _rep(t['Gc'], dc), _rep(t['q2'], ds)
        ids = None if t['ids'] is None else _rep(t['ids'], ds)
        Ps, Vs, Gs = (t['Ps'], t['Vs'], t['Gs']) if ids is not None else (_rep(t['Ps'], ds), _rep(t['Vs'], ds), _rep(t['Gs'], ds))
        dc = ds = 1
    else:
        Pc, Vc, Gc, q2, ids, Ps, Vs, Gs = t['Pc'], t['Vc'], t['Gc'], t['q2'], t['ids'], t['Ps'], t['Vs'], t['Gs']
    f = torch.full((rows, A), 7.0, device=DEV)
    aC, aS, beta = torch.zeros(rows, R, device=DEV), torch.zeros(rows, Mw, device=DEV), torch.zeros(rows, 1, device=DEV)
    fp = torch.zeros(2, rows, A, dtype=torch.float16, device=DEV)
    dummy = torch.empty(rows, A, device=DEV)
    scans = [ops.scan_problem(Pc, Vc, t['qa'], t['wc'], t['bc'], dummy, aC, row_div=dc),
             ops.scan_problem(Ps, Vs, t['qw'], t['ws'], t['bs'], dummy, aS, q2=q2, row_ids=ids, row_div=ds)]
    ops.attn_scan_gate_fwd(scans, (Gc.reshape(-1, A), Gs.reshape(-1, A)), t['zh'], t['b_gc'], t['b_gs'], t['wg'], t['bg'], f,
                           beta, f_planes=fp)
    torch.cuda.synchronize()
    return f, aC, aS, beta, fp


@pytest.mark.parametrize('route', ['row_kernel', 'region_walk'])
@pytest.mark.parametrize('dc,ds', [(6, 3), (6, 1), (6, 6), (15, 5)])
def test_gated_scan_honours_one_divisor_per_scan(dc, ds, route):
    g = torch.Generator().manual_seed(100 * dc + ds)
    prev = ops.set_rows_scan_max(-1)
    try:
        if route == 'region_walk':
            ops.set_rows_scan_max(0)
        for images in (2, 3):                                   # (entry index != 0)
            for R in (7, 36, 37):
                for Mw in (10, 12):
                    for A in (32, 288):
                        for gather in (True, False):
                            t, rows = _gate_case(g, images, dc, ds, R, Mw, A, gather)
                            n0 = _n()
                            got = _gate_run(t, rows, dc, ds, R, Mw, A, expanded=False)
                            assert _n() - n0 == (1 if route == 'row_kernel' else 0)
                            ref = _gate_run(t, rows, dc, ds, R, Mw, A, expanded=True)
                            for name, a, b in zip(('f', 'alpha_c', 'alpha_s', 'beta', 'planes'), got, ref):
                                assert torch.equal(a, b), (name, images, R, Mw, A, gather)
                            assert bool(torch.isfinite(got[0]).all()) and float(got[0].abs().max()) != 7.0
    finally:
        ops.set_rows_scan_max(prev)


def test_gated_scan_refuses_rows_that_do_not_divide():
    g = torch.Generator().manual_seed(5)
    t, rows = _gate_case(g, 2, 6, 3, 7, 10, 32, True)
    f = torch.full((rows, 32), 7.0, device=DEV)
    dummy = torch.empty(rows, 32, device=DEV)
    for dc, ds in ((5, 1), (1, 5), (6, 5)):                      # 12 rows
        a = _lib.ScanGateArgs()
        keep = [_rep(t['Pc'], 6), _rep(t['Vc'], 6), _rep(t['Gc'], 6), _rep(t['q2'], 3), _rep(t['ids'], 3)]
        sc = [ops.scan_problem(keep[0], keep[1], t['qa'], t['wc'], t['bc'], dummy),
              ops.scan_problem(t['Ps'], t['Vs'], t['qw'], t['ws'], t['bs'], dummy, q2=keep[3], row_ids=keep[4])]
        for i in range(2):
            C.memmove(C.byref(a.scan[i]), C.byref(sc[i]), C.sizeof(_lib.ScanProblem))
            a.scan[i].out = None
        a.scan[0].row_div, a.scan[1].row_div = dc, ds
        a.G[0], a.G[1] = keep[2].data_ptr(), t['Gs'].data_ptr()
        a.zh, a.b_gc, a.b_gs, a.w_gate, a.f = (t['zh'].data_ptr(), t['b_gc'].data_ptr(), t['b_gs'].data_ptr(),
                                               t['wg'].data_ptr(), f.data_ptr())
        n0 = _n()
        assert _lib.load().isc_attn_scan_gate_fwd(C.byref(a), rows, ops.stream()) == E_SHAPE
        torch.cuda.synchronize()
        assert _n() == n0 and bool((f == 7.0).all())


# ------------------------------------------------------------------ isc_attn_scan_fwd: two problems, two divisors
@pytest.mark.parametrize('dc,ds', [(15, 5), (6, 1)])
def test_grouped_scan_with_two_different_divisors(dc, ds):
    """(15, 5): the content problem's groups take two chunks, 8 + 7 rows; (6, 1): a plain problem rides along."""
    g = torch.Generator().manual_seed(dc)
    for images in (2, 3):
        for R, Mw, A, gather in ((7, 10, 32, True), (36, 12, 288, False), (37, 10, 288, True)):
            t, rows = _gate_case(g, images, dc, ds, R, Mw, A, gather)
            outs = []
            for expanded in (False, True):
                Pc, Vc, q2, ids, Ps, Vs = t['Pc'], t['Vc'], t['q2'], t['ids'], t['Ps'], t['Vs']
                c, s = dc, ds
                if expanded:
                    Pc, Vc, q2 = _rep(Pc, dc), _rep(Vc, dc), _rep(q2, ds)
                    ids = None if ids is None else _rep(ids, ds)
                    if ids is None:
                        Ps, Vs = _rep(Ps, ds), _rep(Vs, ds)
                    c = s = 1
                v, sv = torch.zeros(rows, A, device=DEV), torch.zeros(rows, A, device=DEV)
                aC, aS = torch.zeros(rows, R, device=DEV), torch.zeros(rows, Mw, device=DEV)
                ops.attn_scan_fwd([ops.scan_problem(Pc, Vc, t['qa'], t['wc'], t['bc'], v, aC, row_div=c),
                                   ops.scan_problem(Ps, Vs, t['qw'], t['ws'], t['bs'], sv, aS, q2=q2, row_ids=ids,
                                                    row_div=s)], rows)
                torch.cuda.synchronize()
                outs.append((v, sv, aC, aS))
            for name, a, b in zip(('v', 's', 'alpha_c', 'alpha_s'), *outs):
                assert torch.equal(a, b), (name, images, R, Mw, A, gather)
            assert float(outs[0][0].abs().max()) > 0


# ------------------------------------------------------------------ the whole step
_caps = {}


@pytest.fixture(scope='module', autouse=True)
def _free_the_models():
    """The cached captioners go with the module."""
    yield
    _caps.clear()
    gc.collect()


def _cap(name):
    if name not in _caps:
        st, w, _, _ = Wd.setup(name)
        cap = Captioner(Wd.idx2word(), synth.SENTIMENT_CATEGORIES, st)
        cap.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
        _caps[name] = cap.to(DEV).eval()
    return _caps[name]


def _grouped_prologue(cap, name, images, S, rows, words_table, fused, words_per_label=False):
    """The prologue with one entry per image / per (image, label): what a shared search decodes on."""
    _, _, d, _ = Wd.setup(name)
    fc, att = Wd.cpu(d, 'fc_feats', images).to(DEV), Wd.cpu(d, 'att_feats', images).to(DEV)
    sw = Wd.cpu(d, 'senti_words', images).to(DEV)
    if words_per_label:                                          # [I, S, M]: other words under every label
        sw = torch.stack([sw.roll(s, 1) for s in range(S)], 1).contiguous()
    labels = torch.tensor([[(i + s) % 3 for s in range(S)] for i in range(images)], dtype=torch.int64, device=DEV)
    return cap._prologue(cap._p(), 'beam', fc, att, None, sw, labels, want_table='build', words_table=words_table,
                         gate_rows=rows if fused else 0, label_group=S)


def _expanded(P, rows, row_div, senti_div):
    """Every step-invariant tensor with one entry per ROW (what beam._Search builds without sharing)."""
    ci = (torch.arange(rows, device=DEV) // row_div)
    si = (torch.arange(rows, device=DEV) // senti_div)
    Pb = _Pro()
    Pb.B, Pb.R, Pb.Mw, Pb.tab = rows, P.R, P.Mw, P.tab
    for k in ('att_e3', 'att_p3'):
        setattr(Pb, k, getattr(P, k).index_select(0, ci).contiguous())
    for k in ('label_e', 'label_w', 'pre1'):
        setattr(Pb, k, getattr(P, k).index_select(0, si).contiguous())
    if P.words_ids is not None:
        Pb.words_e3, Pb.words_p3, Pb.words_ids = P.words_e3, P.words_p3, P.words_ids.index_select(0, si).contiguous()
    else:
        Pb.words_e3, Pb.words_p3 = (getattr(P, k).index_select(0, si).contiguous() for k in ('words_e3', 'words_p3'))
    if P.gate_Gc is not None:
        A = P.gate_Gc.shape[1]
        Pb.gate_Gc = P.gate_Gc.view(-1, P.R, A).index_select(0, ci).reshape(rows * P.R, A).contiguous()
        Pb.gate_Gs = P.gate_Gs if P.words_ids is not None else \
            P.gate_Gs.view(-1, P.Mw, A).index_select(0, si).reshape(rows * P.Mw, A).contiguous()
    return Pb


def _state(cap, rows, seed):
    g = torch.Generator().manual_seed(seed)
    H = cap.att_lstm.hidden_size
    return (_rand(g, 2, rows, H, scale=0.5), _rand(g, 2, rows, H, scale=0.5),
            torch.randint(4, cap.vocab_size, (rows,), generator=g).to(DEV))


@pytest.mark.parametrize('words_table', [True, False])
@pytest.mark.parametrize('name,fused', [('h_wide', True), ('h_wide', False), ('all_differ', False), ('h_768', True)])
@pytest.mark.parametrize('images,S,beam', [(2, 2, 3), (2, 3, 3), (3, 6, 1)])      # 12, 18, 18 rows; the last: a label per row
def test_general_step_on_shared_tensors_equals_the_expanded_step(images, S, beam, name, fused, words_table):
    cap = _cap(name)
    rows, row_div, senti_div = images * S * beam, S * beam, beam
    with torch.no_grad(), ops.h3_weights_scope(DEV):
        P = _grouped_prologue(cap, name, images, S, rows, words_table, fused, words_per_label=(S == 3))
        assert (P.gate_Gc is not None) == fused and P.att_e3.shape[0] == images and P.pre1.shape[0] == images * S
        assert P.label_w.shape[0] == images * S and (P.words_ids is not None) == words_table
        h0, c0, tok = _state(cap, rows, rows + S)
        outs = []
        for shared in (True, False):
            if shared:
                Pb = P
                Pb.row_div, Pb.senti_div = row_div, senti_div
            else:
                Pb = _expanded(P, rows, row_div, senti_div)
            ws = cap._alloc_step_ws(rows, Pb, 128)
            hn, cn = torch.zeros_like(h0), torch.zeros_like(c0)
            logits = torch.zeros(rows, cap.vocab_size, device=DEV)
            aC, aS, bG = torch.zeros(rows, P.R, device=DEV), torch.zeros(rows, P.Mw, device=DEV), torch.zeros(rows, 1, device=DEV)
            n0 = _n()
            cap._step(cap._p(), Pb, ws, None, h0, c0, hn, cn, aC, aS, bG, logits=logits, tok=tok)
            torch.cuda.synchronize()
            assert _n() - n0 == (1 if fused else 0)             # the fused gate scan of <= 256 rows: the row kernel
            pl = ws['_plan']
            assert (pl.row_div, pl.senti_div) == ((row_div, senti_div) if shared else (0, 0))
            outs.append((hn, cn, logits, ws['pmax'], ws['psum'], ws['pidx'], ws['f'], aC, aS, bG))
    names = ('h', 'c', 'logits', 'pmax', 'psum', 'pidx', 'f', 'alpha_c', 'alpha_s', 'beta')
    for k, a, b in zip(names, *outs):
        assert torch.equal(a, b), (k, float((a.float() - b.float()).abs().max()))
    assert float(outs[0][2].abs().max()) > 0 and bool(torch.isfinite(outs[0][2]).all())


def _ext(cap, beam, last, cand, row_div, senti_div):
    x = _lib.RowsExt()
    x.stats_tile, x.beam = ops.rows_stats_tile(cap.vocab_size), beam
    x.pad_id, x.sos_id, x.unk_id, x.mask_special, x.decoding_constraint = cap.pad_id, cap.sos_id, cap.unk_id, 1, 1
    x.last_word, x.cand_val, x.cand_idx = last.data_ptr(), cand[0].data_ptr(), cand[1].data_ptr()
    x.row_div, x.senti_div = row_div, senti_div
    return x


@pytest.mark.parametrize('words_table', [False, True])
@pytest.mark.parametrize('name', ['h_wide', 'h_768'])
@pytest.mark.parametrize('S,beam,senti_div', [(2, 3, 3), (2, 4, 4), (8, 1, 1)])      # (6, 3), (8, 4), (8, 1)
def test_few_row_step_on_shared_tensors_equals_the_expanded_step(S, beam, senti_div, name, words_table):
    cap = _cap(name)
    rows = row_div = S * beam
    V = cap.vocab_size
    with torch.no_grad(), ops.h3_weights_scope(DEV):
        P = _grouped_prologue(cap, name, 1, S, rows, words_table, True)
        assert cap._rows_step_ok(rows, P) and P.att_e3.shape[0] == 1 and P.pre1.shape[0] == S
        h0, c0, tok = _state(cap, rows, 31 * rows + senti_div)
        src = torch.randint(0, rows, (rows,), generator=torch.Generator().manual_seed(rows)).to(DEV)
        tw = ops.rows_stats_tile(V)
        outs = []
        for shared in (True, False):
            Pb = P if shared else _expanded(P, rows, row_div, senti_div)
            ws = cap._alloc_step_ws(rows, Pb, tw)
            n_tile = ws['pmax'].shape[1]
            cand = (torch.zeros(rows, n_tile, 8, device=DEV), torch.zeros(rows, n_tile, 8, dtype=torch.int32, device=DEV))
            x = _ext(cap, beam, tok, cand, row_div if shared else 0, senti_div if shared else 0)
            x.src_row = src.data_ptr()
            hn, cn = torch.zeros_like(h0), torch.zeros_like(c0)
            aC, aS, bG = torch.zeros(rows, P.R, device=DEV), torch.zeros(rows, P.Mw, device=DEV), torch.zeros(rows, 1, device=DEV)
            n0 = _n()
            cap._step(cap._p(), Pb, ws, None, h0, c0, hn, cn, aC, aS, bG, tok=tok, rows_ext=x)
            torch.cuda.synchronize()
            assert _n() - n0 == 5
            outs.append((hn, cn, ws['pmax'], ws['psum'], ws['pidx'], cand[0], cand[1], ws['f'], aC, aS, bG))
    names = ('h', 'c', 'pmax', 'psum', 'pidx', 'cand_val', 'cand_idx', 'f', 'alpha_c', 'alpha_s', 'beta')
    for k, a, b in zip(names, *outs):
        assert torch.equal(a, b), (k, float((a.float() - b.float()).abs().max()))
    assert float(outs[0][0].abs().max()) > 0


def test_shape_refusals_launch_nothing():
    """rows % row_div, row_div % senti_div, pair_rows_c with row_div: ISC_E_SHAPE from both step entry points, the outputs
    untouched and nothing counted as launched."""
    cap = _cap('h_wide')
    rows = 6
    lib = _lib.load()
    with torch.no_grad(), ops.h3_weights_scope(DEV):
        P = _grouped_prologue(cap, 'h_wide', 1, 2, rows, False, True)
        P.row_div, P.senti_div = 6, 3
        h0, c0, tok = _state(cap, rows, 3)
        for few in (False, True):
            ws = cap._alloc_step_ws(rows, P, ops.rows_stats_tile(cap.vocab_size) if few else 128)
            n_tile = ws['pmax'].shape[1]
            cand = (torch.zeros(rows, n_tile, 8, device=DEV), torch.zeros(rows, n_tile, 8, dtype=torch.int32, device=DEV))
            x = _ext(cap, 3, tok, cand, 6, 3) if few else None
            hn, cn = torch.full_like(h0, 7.0), torch.full_like(c0, 7.0)
            logits = torch.full((rows, cap.vocab_size), 7.0, device=DEV)
            cap._step(cap._p(), P, ws, None, h0, c0, hn, cn, logits=logits, tok=tok, rows_ext=x)     # a good call fills the plan
            torch.cuda.synchronize()
            assert not bool((hn == 7.0).any())
            pl = ws['_plan']
            for k in ('pmax', 'psum'):
                ws[k].fill_(7.0)
            for row_div, senti_div, pair in ((4, 2, 0), (5, 0, 0), (6, 4, 0), (6, 5, 0), (6, -1, 0), (6, 3, 2), (6, 0, 3)):
                hn.fill_(7.0), cn.fill_(7.0), logits.fill_(7.0)
                bad = type(pl).from_buffer_copy(pl)
                bad.pair_rows_c = pair
                if pair:
                    bad.gate_Gc = bad.gate_Gs = None
                    bad.s = bad.v + 4 * pair * bad.E
                n0 = _n()
                if few:
                    xb = type(x).from_buffer_copy(x)
                    xb.row_div, xb.senti_div = row_div, senti_div
                    rc = lib.isc_rows_step_fwd(C.byref(bad), C.byref(xb), ops.stream())
                else:
                    bad.row_div, bad.senti_div = row_div, senti_div
                    rc = lib.isc_step_fwd(C.byref(bad), ops.stream())
                torch.cuda.synchronize()
                assert rc == E_SHAPE, (few, row_div, senti_div, pair, rc)
                assert _n() == n0
                for t in (hn, cn, logits, ws['pmax'], ws['psum']):
                    assert bool((t == 7.0).all()), (few, row_div, senti_div, pair)
