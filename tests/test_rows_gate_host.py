"""The few-row step's gate on the host (no GPU, nothing is issued): isc_rows_step_supported may not promise a step that one
of its five launches then refuses, and the Python gates in front of it (Captioner._rows_step_ok, Captioner._rows_vocab_ok,
beam._few_rows) may not send the kernels a shape the library turns away.

The defect this pins: the predicate accepted every 512 < H <= 1024 with 8192 < V <= 16384 (and, with no bound on H at
all, H > 1024 with V > 4096), shapes whose classifier tile the fifth launch cannot hold (J = 8 / ceil(H / 256) column
groups x 4 passes x 4 lane groups < the tile's columns): a captioner with rnn_hid_dim = 768 and 10000 words raised
ISC_E_SHAPE from isc_rows_step_fwd after four launches had been issued.  The launches and the predicate now take their
geometry from one set of host functions (csrc/rows.hip), exported as the pure predicates swept here."""
import ctypes as C
import types

import pytest

from insenticap_model_amd import Captioner, _lib, beam, ops

HS = list(range(4, 1537, 4))
VS = [4096, 4100, 8192, 8196, 12288, 12292, 16384, 16388]
FAKE = 4096          # a non-null "pointer": the predicate tests pointers for presence and reads none


def _plan(rows, H, A, V, R=7, Mw=5, tab=True):
    p = _lib.StepPlan()
    p.rows, p.H, p.E, p.A, p.W, p.V, p.R, p.Mw = rows, H, A, A, A, V, R, Mw
    p.att_e = p.words_e = p.gate_Gc = p.gate_Gs = FAKE
    if tab:
        p.tab = FAKE
    return p


def _launches_accept(lib, rows, H, A, V, tab):
    """The five launches' own conditions, one by one, as rows_step issues them."""
    return (lib.isc_rows_lstm_supported(rows, H, H, 0 if tab else A, H) == 1       # att-LSTM: h_lang (, xt), h_att
            and lib.isc_rows_linear_supported(rows, H, 3 * A) == 1                 # h2att, h2word, the gate's h-term
            and lib.isc_rows_lstm_supported(rows, H, A, H, H) == 1                 # lang-LSTM: f, h_att, h_lang
            and lib.isc_rows_vocab_supported(rows, V, H) == 1)


def _vocab_rule(V, K):
    """The classifier's rule restated from the kernel's geometry: a tile of tw columns is held as J waves x NP <= 4 passes x
    4 lane groups, J = min(4, 8 / S) with S = min(8, ceil(K / 256)) K-slices in flight."""
    tw = min(64, max(16, 4 * ((V // 4 + 255) // 256)))
    S = min(8, -(-K // 256))
    J = min(max(8 // S, 1), 4, -(-tw // 4))
    return -(-K // 256) <= 12 and -(-(-(-tw // 4)) // J) <= 4


@pytest.mark.parametrize('A', [4, 260, 512])
def test_supported_implies_every_launch_accepts(A):
    lib = _lib.load()
    seen = {0: 0, 1: 0}
    for tab in (True, False):
        for H in HS:
            for V in VS:
                for rows in (1, 8):
                    ok = lib.isc_rows_step_supported(C.byref(_plan(rows, H, A, V, tab=tab)))
                    seen[ok] += 1
                    if ok:
                        assert _launches_accept(lib, rows, H, A, V, tab), (rows, H, A, V, tab)
                        assert V <= 16384
                    assert ok == lib.isc_rows_shape_supported(rows, H, A, A, A, V, 7, 5, int(tab))
    assert seen[0] > 1000 and seen[1] > 1000


def test_the_classifier_predicate_is_the_kernels_geometry():
    lib = _lib.load()
    for K in HS + [2048, 2308, 3072, 3076]:
        for V in VS[:-1] + [1, 300, 4095, 10000]:
            for M in (1, 5, 8):
                assert lib.isc_rows_vocab_supported(M, V, K) == int(_vocab_rule(V, K)), (M, V, K)
    for bad in ((0, 300, 64), (9, 300, 64), (1, 0, 64), (1, 300, 0), (1, 300, 66)):
        assert lib.isc_rows_vocab_supported(*bad) == 0


def test_the_shapes_of_the_defect_and_the_bound_on_h():
    lib = _lib.load()
    sup = lambda H, V, A=32, tab=True, rows=5: lib.isc_rows_step_supported(C.byref(_plan(rows, H, A, V, tab=tab)))
    for H in (516, 768, 1024):
        for V in (8196, 10000, 16384):
            assert sup(H, V) == 0 and lib.isc_rows_vocab_supported(5, V, H) == 0
        assert sup(H, 8192) == 1 and sup(H, 300) == 1
    assert sup(512, 10000) == 1 and sup(512, 16384) == 1 and sup(512, 16388) == 0     # the default shape keeps the path
    # H > 1024: one column group, V <= 4096; the lang-LSTM's slices (ceil(E / 256) + 2 ceil(H / 256) <= 12) end at H = 1280
    assert sup(1028, 4096) == 1 and sup(1028, 4100) == 0
    assert sup(1280, 300) == 1 and sup(1280, 300, A=260, tab=False) == 1 and sup(1280, 300, A=512, tab=False) == 1
    assert sup(1284, 300) == 0 and sup(1284, 300, A=4) == 0 and sup(1536, 300) == 0
    # the scan's own limits and the row count
    assert sup(64, 300, A=516) == 0 and sup(64, 300, rows=9) == 0 and sup(64, 300, rows=0) == 0
    assert lib.isc_rows_step_supported(C.byref(_plan(5, 64, 32, 300, R=0))) == 0
    assert lib.isc_rows_step_supported(None) == 0


def _stub(H, A, V):
    cap = types.SimpleNamespace(settings=dict(feat_emb_dim=A, att_hid_dim=A, word_emb_dim=A, rnn_hid_dim=H), vocab_size=V,
                                ROWS_STEP_MAX=Captioner.ROWS_STEP_MAX, ROWS_STEP_MAX_H=Captioner.ROWS_STEP_MAX_H)
    cap._rows_vocab_ok = lambda: Captioner._rows_vocab_ok(cap)
    return cap


@pytest.mark.parametrize('A', [32, 260])
def test_python_gates_agree_with_the_c_predicate(A):
    """On the sweep: Captioner._rows_step_ok is isc_rows_step_supported up to ROWS_STEP_MAX_H = 1024 (the widest LSTM the
    searches send there; beyond it the Python gate keeps the general kernels although the kernels would take V <= 4096);
    it never accepts what the library refuses.  _rows_vocab_ok and beam._few_rows are the classifier's predicate."""
    lib = _lib.load()
    assert not ops.TIMER.armed and ops.TIMER.arm_step is None
    for tab in (True, False):
        P = types.SimpleNamespace(gate_Gc=object(), gate_Gs=object(), tab=object() if tab else None)
        for H in HS:
            for V in VS:
                cap = _stub(H, A, V)
                c_ok = lib.isc_rows_step_supported(C.byref(_plan(5, H, A, V, tab=tab))) == 1
                py_ok = bool(Captioner._rows_step_ok(cap, 5, P))
                assert py_ok == (c_ok and H <= 1024), (H, A, V, tab)
                v_ok = bool(cap._rows_vocab_ok())
                assert v_ok == (V <= 16384 and lib.isc_rows_vocab_supported(1, V, H) == 1), (H, V)
                assert bool(beam._few_rows(cap, 1, 5)) == v_ok and not beam._few_rows(cap, 2, 5)
    assert not Captioner._rows_step_ok(_stub(768, 32, 10000), 5, P) and Captioner._rows_step_ok(_stub(768, 32, 8192), 5, P)


def test_route_log_reads_without_a_device():
    """isc_rows_routes: reading touches no device; with nothing launched it reports what has been recorded (0 here or
    whatever earlier tests of the process launched) and writes at most that many records."""
    total, recs = ops.rows_routes(16)
    assert total >= 0 and len(recs) == min(total, 16)
    assert _lib.load().isc_rows_routes(None, 0) == total
