"""CPU-only checks: the C-ABI library loads and exports every symbol include/insenticap_hip.h
declares (no compute calls without a GPU), the ctypes structs match the C layout, the host
mirror keeps the reference's API surface, and the product fails loudly without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from insenticap_model_amd import Captioner, XECriterion, _build, _lib, synth

HEADER = os.path.join(ROOT, 'include', 'insenticap_hip.h')


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(isc_[a-z0-9_]+)\s*\(', src)))


def test_library_builds_and_exports_every_declared_symbol():
    path = _build.build()
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    names = declared_functions()
    assert len(names) >= 24
    for n in names:
        assert hasattr(lib, n), 'missing export: ' + n
    # the binding table covers exactly the declared entry points
    assert sorted(_lib.SIGNATURES) == names
    lib2 = _lib.load()
    assert lib2.isc_target_arch() == b'gfx950'
    assert lib2.isc_abi_version() >= 1


def test_no_kernel_spills_or_uses_scratch():
    """A runtime-indexed register array silently moves to scratch memory and halves GEMM speed
    (seen once in this repo): every kernel must keep its arrays in registers."""
    rep = _build.resource_report()
    assert len(rep) >= 25
    for k, r in rep.items():
        assert r.get('scratch', 0) == 0, (k, r)
        assert r.get('vgpr_spill', 0) == 0, (k, r)
    gemm = [r for k, r in rep.items() if 'gemm_kernel' in k]
    assert gemm and all(r['occupancy'] >= 2 for r in gemm)   # 2 workgroups per CU (the LDS limit)


def _code_objects(path, tmp):
    """The gfx950 code objects of a fat shared library: the clang offload bundles of its .hip_fatbin section."""
    import struct
    fat = os.path.join(tmp, 'fat.bin')
    subprocess.check_call(['/opt/rocm/lib/llvm/bin/llvm-objcopy', '-O', 'binary', '--only-section=.hip_fatbin', path, fat])
    raw = open(fat, 'rb').read()
    magic, out, pos = b'__CLANG_OFFLOAD_BUNDLE__', [], 0
    while True:
        i = raw.find(magic, pos)
        if i < 0:
            return out
        q = i + len(magic)
        n, = struct.unpack_from('<Q', raw, q)
        q += 8
        for _ in range(n):
            off, size, tl = struct.unpack_from('<QQQ', raw, q)
            q += 24
            if b'gfx950' in raw[q:q + tl] and size:
                out.append(raw[i + off:i + off + size])
            q += tl
        pos = i + len(magic)


def test_kernarg_warm_up_reads_stay_inside_the_kernarg_segment(tmp_path):
    """csrc/common.h rows_kernarg_warm touches one dword per 64-byte line of the argument struct in one batch.  A kernel
    without hidden arguments has a kernarg segment of exactly sizeof(struct) bytes: a load past it is out of bounds (it
    faulted once, in a B = 1024 training graph, when a segment ended where its mapping ended).  Checked on the SHIPPED
    code objects: every run of >= 4 scalar loads into one and the same register ends inside the segment."""
    import re
    cos = _code_objects(_build.LIB_PATH, str(tmp_path))
    assert len(cos) >= 4
    runs = 0
    for n, co in enumerate(cos):
        f = str(tmp_path / ('k%d.co' % n))
        open(f, 'wb').write(co)
        notes = subprocess.check_output(['/opt/rocm/lib/llvm/bin/llvm-readelf', '--notes', f]).decode()
        size = {}
        for m in re.finditer(r'\.kernarg_segment_size:\s*(\d+).*?\.name:\s*(\S+)', notes, re.S):
            size[m.group(2)] = int(m.group(1))
        dis = subprocess.check_output(['/opt/rocm/lib/llvm/bin/llvm-objdump', '-d', '--mcpu=gfx950', f]).decode()
        cur, run = None, []

        def close():
            nonlocal runs
            if len(run) >= 4:
                runs += 1
                assert cur in size, cur
                assert max(run) + 4 <= size[cur], (cur, size[cur], [hex(x) for x in run])
            run.clear()
        last = None
        for line in dis.splitlines():
            m = re.match(r'^[0-9a-f]+ <(\S+)>:', line)
            if m:
                close()
                cur, last = m.group(1), None
                continue
            m = re.match(r'\s+s_load_dword (s\d+), (s\[\d+:\d+\]), (0x[0-9a-f]+|\d+)\s', line)
            if m and (m.group(1), m.group(2)) == last:
                run.append(int(m.group(3), 0))
            else:
                close()
                if m:
                    run.append(int(m.group(3), 0))
            last = (m.group(1), m.group(2)) if m else None
        close()
    assert runs >= 20           # the GEMM / scan / rows kernels carry the warm-up


def test_ctypes_struct_layout_matches_c(tmp_path):
    """Compile a tiny C program against the header and compare sizeof/offsetof with ctypes."""
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "insenticap_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(isc_seg), sizeof(isc_linear_problem), sizeof(isc_lstm_problem),
         sizeof(isc_scan_problem), sizeof(isc_rollout_step));
  printf("%zu %zu %zu %zu\n", offsetof(isc_linear_problem, bias0), offsetof(isc_linear_problem, C),
         offsetof(isc_linear_problem, accumulate), sizeof(isc_scan_bwd_problem));
  printf("%zu %zu %zu\n", offsetof(isc_lstm_problem, c_prev), offsetof(isc_scan_problem, out),
         offsetof(isc_rollout_step, xt_next));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(isc_step_plan), offsetof(isc_step_plan, tok_stride),
         offsetof(isc_step_plan, out_scale), offsetof(isc_step_plan, pidx), sizeof(isc_step_bwd_plan),
         offsetof(isc_step_bwd_plan, dbg_rows));
  printf("%zu %zu %zu %zu %zu\n", offsetof(isc_step_plan, words_ids_ld), offsetof(isc_lstm_problem, h_lo),
         offsetof(isc_scan_problem, row_ids_ld), sizeof(isc_beam_merge_args), offsetof(isc_beam_merge_args, live));
  return 0;
}
'''
    cfile, exe = str(tmp_path / 'layout.c'), str(tmp_path / 'layout')      # nothing is written into the tree
    open(cfile, 'w').write(prog)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), cfile, '-o', exe])
    out = subprocess.check_output([exe]).decode().split()
    got = [int(x) for x in out]
    L = _lib
    exp = [ctypes.sizeof(L.Seg), ctypes.sizeof(L.LinearProblem), ctypes.sizeof(L.LstmProblem),
           ctypes.sizeof(L.ScanProblem), ctypes.sizeof(L.RolloutStep),
           L.LinearProblem.bias0.offset, L.LinearProblem.C.offset, L.LinearProblem.accumulate.offset,
           ctypes.sizeof(L.ScanBwdProblem),
           L.LstmProblem.c_prev.offset, L.ScanProblem.out.offset, L.RolloutStep.xt_next.offset,
           ctypes.sizeof(L.StepPlan), L.StepPlan.tok_stride.offset, L.StepPlan.out_scale.offset,
           L.StepPlan.pidx.offset, ctypes.sizeof(L.StepBwdPlan), L.StepBwdPlan.dbg_rows.offset,
           L.StepPlan.words_ids_ld.offset, L.LstmProblem.h_lo.offset, L.ScanProblem.row_ids_ld.offset,
           ctypes.sizeof(L.BeamMergeArgs), L.BeamMergeArgs.live.offset]
    assert got == exp


def test_argument_validation_without_a_gpu():
    """Bad arguments are rejected on the host before anything touches the device."""
    lib = _lib.load()
    assert lib.isc_linear_fwd(None, 1, None) == -1
    p = _lib.LinearProblem()
    assert lib.isc_linear_fwd(ctypes.byref(p), 0, None) == -2
    assert lib.isc_linear_fwd(ctypes.byref(p), 1, None) == -2         # nseg == 0
    p.nseg = 1
    assert lib.isc_linear_fwd(ctypes.byref(p), 1, None) == -1         # null segment pointers
    assert lib.isc_attn_scan_fwd(None, 1, 4, None) == -1
    assert lib.isc_vocab_fwd(None, 0, None, 0, None, 1, 1, 32, None, 0, None, None, None, None, None, None, 0, None) == -1
    assert lib.isc_gemm_bwd(ctypes.byref(p), 1, 7, None) == -2        # unknown layout
    assert lib.isc_colsum(None, 0, 1, 1, None, 0, None, 0, None) == -1


def test_f32_launch_counter_kinds_without_a_gpu():
    """isc_f32_launches: kinds 0-6 exist and read 0 or more, any other kind answers -1; reading touches no device."""
    lib = _lib.load()
    assert lib.isc_f32_launches(-1) == -1 and lib.isc_f32_launches(7) == -1
    assert all(lib.isc_f32_launches(k) >= 0 for k in range(7))
    from insenticap_model_amd import ops
    assert ops.f32_launches(7) == -1 and ops.f32_launches(6) >= 0


def test_h3_kernel_launch_counter_kinds_without_a_gpu():
    """isc_h3_kernel_launches: kinds 0-16 exist and read 0 or more, any other kind answers -1; reading touches no device."""
    lib = _lib.load()
    assert lib.isc_h3_kernel_launches(-1) == -1 and lib.isc_h3_kernel_launches(17) == -1
    assert all(lib.isc_h3_kernel_launches(k) >= 0 for k in range(17))
    from insenticap_model_amd import ops
    assert ops.H3_KINDS == 17 and ops.h3_kernel_launches(17) == -1 and ops.h3_kernel_launches(16) >= 0


def make(V=64, st=synth.TINY_SETTINGS):
    return Captioner(synth.make_idx2word(V), synth.SENTIMENT_CATEGORIES, st)


def test_state_dict_matches_reference_layout():
    cap = make()
    shapes = synth.param_shapes(64, synth.TINY_SETTINGS)
    sd = cap.state_dict()
    assert list(sd.keys()) == list(shapes.keys())          # names AND registration order
    for k, v in sd.items():
        assert tuple(v.shape) == shapes[k], k
    assert len(sd) == 40
    # full-size model: 22,063,379 parameters
    full = synth.param_shapes(10000, synth.DEFAULT_SETTINGS)
    assert sum(int(np.prod(s)) for s in full.values()) == 22063379


def test_special_ids_and_api_surface():
    cap = make()
    assert (cap.pad_id, cap.sos_id, cap.eos_id, cap.unk_id, cap.neu_idx) == (0, 1, 2, 3, 2)
    assert cap.vocab_size == 64
    for name in ('forward_xe', 'forward_seq2seq', 'forward_rl', 'sample', 'sample_batch', 'init_hidden',
                 'get_optim_criterion'):
        assert callable(getattr(cap, name))
    # vocabulary without <SOS>: sos/eos fall back to <PAD> exactly like the reference (captioner.py:127-128)
    cap2 = Captioner(['<PAD>', '<UNK>', 'a', 'b'] + ['w%d' % i for i in range(28)], ['positive', 'negative', 'neutral'],
                     synth.TINY_SETTINGS)
    assert cap2.sos_id == cap2.pad_id == cap2.eos_id == 0
    optim, xe, mse = cap.get_optim_criterion(4e-4)
    assert isinstance(optim, torch.optim.Adam) and isinstance(xe, XECriterion) and isinstance(mse, torch.nn.MSELoss)
    assert optim.param_groups[0]['lr'] == 4e-4 and optim.param_groups[0]['betas'] == (0.9, 0.999)


def test_unsupported_dims_are_rejected():
    st = dict(synth.TINY_SETTINGS, rnn_hid_dim=48)
    with pytest.raises(ValueError):
        make(st=st)
    st = dict(synth.TINY_SETTINGS, word_emb_dim=64)
    with pytest.raises(ValueError):
        make(st=st)


def test_product_fails_loudly_on_cpu():
    """No CPU fallback: calling the model with CPU parameters raises instead of computing."""
    cap = make().eval()
    d = synth.make_inputs(2, 64, synth.TINY_SETTINGS, regions=6, seq_len=4, seed=0)
    t = lambda k: torch.from_numpy(d[k])
    with torch.no_grad():
        with pytest.raises(_lib.HipLibraryError):
            cap(t('fc_feats'), t('att_feats'), t('cpt_words'), t('senti_words'), t('senti_labels'), 4, 1, mode='rl')
        with pytest.raises(_lib.HipLibraryError):
            cap(t('fc_feats'), t('att_feats'), t('cpt_words'), t('captions'), t('senti_labels'), mode='xe')
        with pytest.raises(_lib.HipLibraryError):
            cap.sample(t('fc_feats')[0], t('att_feats')[0])


def test_missing_library_is_an_error(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libinsenticap_hip.so')
    with pytest.raises(_lib.HipLibraryError):
        _lib.load()


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under insenticap_model_amd/ may reference it."""
    pkg = os.path.join(ROOT, 'insenticap_model_amd')
    for fn in os.listdir(pkg):
        if fn.endswith('.py'):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), fn


def test_attention_weight_attributes_resolve_lazily():
    """cont_weights / senti_weights / cont_senti_weights: set per call without a host read; the executed-step
    count of a roll-out (the reference's early `break`) is taken from the `alive` counters only on access."""
    import torch
    from insenticap_model_amd import Captioner, synth
    cap = Captioner(synth.make_idx2word(64), synth.SENTIMENT_CATEGORIES, synth.TINY_SETTINGS)
    assert cap.cont_weights == [] and cap.senti_weights == [] and cap.cont_senti_weights == []
    B, T, R, M = 3, 5, 4, 2
    aC, aS, bG = torch.rand(B, T, R), torch.rand(B, T, M), torch.rand(B, T)
    cap._set_weights(aC, aS, bG, T)                                  # teacher-forced unrolls: all T steps
    assert cap.cont_weights.shape == (B, T * R) and cap.senti_weights.shape == (B, T * M)
    assert torch.equal(cap.cont_senti_weights, bG)
    alive = torch.tensor([3, 2, 1, 0, 0, 0], dtype=torch.int32)      # no row unfinished after step 2 -> 3 steps ran
    cap._set_weights(aC, None, None, alive)
    assert cap.cont_weights.shape == (B, 3 * R) and torch.equal(cap.cont_weights, aC[:, :3].reshape(B, -1))
    assert cap.senti_weights == [] and cap.cont_senti_weights == []
    cap.cont_weights = []                                            # plain assignment still works (beam search)
    assert cap.cont_weights == []


def test_beam_merge_vectorised_equals_list_version():
    """beam.py: the numpy candidate merge (many images) must reproduce the reference-style Python merge step by step -
    gather indices, fed tokens, final ids and fp64 scores - including ties, early <EOS> and images that finish."""
    import numpy as np
    from insenticap_model_amd.beam import _ListMerge, _VectorMerge
    rng = np.random.default_rng(5)
    n_img, beam, T, sos, eos = 7, 3, 9, 1, 2
    rows = n_img * beam
    a, b = _ListMerge(n_img, beam, sos, eos), _VectorMerge(n_img, beam, T, sos, eos)
    for t in range(T):
        ti = rng.integers(2, 7, size=(rows, beam)).astype(np.int64)           # small vocabulary: <EOS> (2) is frequent
        tv = -rng.integers(1, 4, size=(rows, beam)).astype(np.float32) * 0.5     # few distinct values: many ties
        tv.sort(axis=1)
        tv = tv[:, ::-1].copy()                                                # top-k comes sorted, best first
        la, ga = np.full(rows, sos, dtype=np.int64), np.zeros(rows, dtype=np.int64)
        lb, gb = la.copy(), ga.copy()
        if t > 0:
            la[:] = last_prev
            lb[:] = last_prev
        live_a = a.step(t, ti, tv, la, ga)
        live_b = b.step(t, ti, tv, lb, gb)
        assert live_a == live_b, t
        assert (ga == gb).all() and (la == lb).all(), t
        last_prev = la.copy()
        if not live_a:
            break
    ra, rb = a.result(), b.result()
    assert ra == rb
