"""CPU-only checks of float16 region features: the feature stores write / re-open them with the dtype kept and refuse
values float16 cannot hold, the collates keep float16 batches float16 (mixed batches become fp32), and `isc_seg.a_f16`
sits where `_pad` sat, in the header and in the ctypes mirror."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from insenticap_model_amd import _lib, data


def _array(n=5, shape=(3, 8), seed=0):
    return (np.random.RandomState(seed).randn(n, *shape) * 3).astype(np.float32)


def test_feature_store_keeps_float16(tmp_path):
    fns, arr = ['a', 'b', 'c', 'd', 'e'], _array()
    path = data.FeatureStore.write(str(tmp_path / 'att16'), fns, arr, dtype=np.float16)
    st = data.FeatureStore(path)
    assert st.array.dtype == np.float16 and st['c'].dtype == np.float16
    assert os.path.getsize(path) - 128 == arr.nbytes // 2         # half the bytes behind the .npy header
    for i, fn in enumerate(fns):
        np.testing.assert_array_equal(st[fn], arr[i].astype(np.float16))
    # torch's spelling of the dtype is taken too
    st2 = data.FeatureStore(data.FeatureStore.write(str(tmp_path / 'att16t'), fns, arr, dtype=torch.float16))
    np.testing.assert_array_equal(st2.array, arr.astype(np.float16))


def test_feature_store_default_is_still_fp32(tmp_path):
    fns, arr = ['a', 'b', 'c', 'd', 'e'], _array()
    st = data.FeatureStore(data.FeatureStore.write(str(tmp_path / 'att32'), fns, arr))
    assert st.array.dtype == np.float32 and st['a'].dtype == np.float32
    np.testing.assert_array_equal(st['e'], arr[4])
    # ... also for an array that comes as float16
    st = data.FeatureStore(data.FeatureStore.write(str(tmp_path / 'att32b'), fns, arr.astype(np.float16)))
    assert st.array.dtype == np.float32


def test_feature_store_refuses_what_float16_cannot_hold(tmp_path):
    fns, arr = ['a', 'b', 'c', 'd', 'e'], _array()
    arr[3, 1, 2] = 70000.0
    arr[1, 0, 0] = -66000.0
    with pytest.raises(ValueError, match='70000'):                # names the largest |x|
        data.FeatureStore.write(str(tmp_path / 'bad'), fns, arr, dtype=np.float16)
    assert not os.path.exists(str(tmp_path / 'bad.npy'))          # nothing was stored
    data.FeatureStore.write(str(tmp_path / 'ok32'), fns, arr)     # fp32 holds it
    arr[3, 1, 2], arr[1, 0, 0] = 65504.0, -65504.0                # the largest float16: fine
    st = data.FeatureStore(data.FeatureStore.write(str(tmp_path / 'edge'), fns, arr, dtype=np.float16))
    assert float(st['d'][1, 2]) == 65504.0
    with pytest.raises(ValueError):
        data.FeatureStore.write(str(tmp_path / 'bf'), fns, arr, dtype=np.float64)


def _img(fn, caps, dtype, seed):
    r = np.random.RandomState(seed)
    return fn, r.randn(8).astype(dtype), r.randn(3, 8).astype(dtype), caps, [5, 6], [20, 21]


def _datasets(dt_a, dt_b):
    a, b = _img('a', [[1, 5, 6, 2], [1, 7, 8, 9, 2]], dt_a, 1), _img('b', [[1, 4, 2]], dt_b, 2)
    return {'caption': [(x[0], x[1], x[2], x[3], x[4]) for x in (a, b)],
            'rl_fact': [(x[0], x[3], x[1], x[2], x[4], x[5]) for x in (a, b)],
            'rl_senti': [(x[0], x[1], x[2], x[4], x[5], 1) for x in (a, b)]}


def _feats_of(name, out):
    return (out[1], out[2])


@pytest.mark.parametrize('name', ['caption', 'rl_fact', 'rl_senti'])
def test_collates_keep_float16(name):
    random.seed(0)
    f = data.create_collate_fn(name, pad_index=0, max_seq_len=6, num_concepts=3, num_sentiments=3)
    ds16, ds32 = _datasets(np.float16, np.float16)[name], _datasets(np.float32, np.float32)[name]
    random.seed(0)
    fc16, att16 = _feats_of(name, f(ds16))
    random.seed(0)
    fc32, att32 = _feats_of(name, f(ds32))
    assert fc16.dtype == torch.float16 and att16.dtype == torch.float16
    assert fc32.dtype == torch.float32 and att32.dtype == torch.float32          # today's behaviour
    assert fc16.shape == fc32.shape and att16.shape == att32.shape
    assert torch.equal(fc16, fc32.half()) and torch.equal(att16, att32.half())   # same rows, same order


def test_scs_collate_has_no_features_and_is_unchanged():
    f = data.create_collate_fn('scs', max_seq_len=6, num_concepts=2, num_sentiments=3)
    (caps, lengths), cpts, sentis, ids = f([([1, 9, 2], [5, 6, 7], [8], 1), ([1, 3, 4, 5, 2], [5], [8, 9, 9, 9], 0)])
    assert caps.dtype == torch.int64 and ids.tolist() == [0, 1]


def test_dedup_collate_gives_a_float16_row_gather():
    f = data.create_collate_fn('caption', pad_index=0, max_seq_len=6, num_concepts=3, dedup=True)
    plain = data.create_collate_fn('caption', pad_index=0, max_seq_len=6, num_concepts=3)
    ds = _datasets(np.float16, np.float16)['caption']
    out, ref = f(ds), plain(ds)
    assert isinstance(out[1], data.RowGather) and isinstance(out[2], data.RowGather)
    assert out[1].base.dtype == torch.float16 and out[2].base.dtype == torch.float16
    assert out[2].dense().dtype == torch.float16 and torch.equal(out[2].dense(), ref[2])
    assert torch.equal(out[1].dense(), ref[1])


@pytest.mark.parametrize('name', ['caption', 'rl_fact', 'rl_senti'])
def test_mixed_dtype_batch_becomes_fp32(name):
    random.seed(0)
    f = data.create_collate_fn(name, pad_index=0, max_seq_len=6, num_concepts=3, num_sentiments=3)
    fc, att = _feats_of(name, f(_datasets(np.float16, np.float32)[name]))
    assert fc.dtype == torch.float32 and att.dtype == torch.float32
    fc, att = _feats_of(name, f(_datasets(np.float64, np.float64)[name]))      # any other dtype: fp32, as ever
    assert fc.dtype == torch.float32 and att.dtype == torch.float32


def test_seg_a_f16_sits_where_pad_sat(tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "insenticap_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(isc_seg), offsetof(isc_seg, K), offsetof(isc_seg, a_f16),
         offsetof(isc_seg, A_hi), sizeof(((isc_seg *)0)->a_f16), sizeof(isc_linear_problem));
  return 0;
}
'''
    cfile, exe = str(tmp_path / 'layout.c'), str(tmp_path / 'layout')
    open(cfile, 'w').write(prog)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), cfile, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    S = _lib.Seg
    assert got == [ctypes.sizeof(S), S.K.offset, S.a_f16.offset, S.A_hi.offset, S.a_f16.size,
                   ctypes.sizeof(_lib.LinearProblem)]
    # the old `_pad`: the int32 behind K, in front of the plane pointers - sizes and every other offset as before
    assert got[:5] == [48, 24, 28, 32, 4]
    assert [n for n, _ in S._fields_] == ['A', 'W', 'lda', 'ldw', 'K', 'a_f16', 'A_hi', 'A_lo']
    assert _lib.Seg().a_f16 == 0                                  # default: fp32 rows, today's behaviour


def test_new_entry_points_are_declared_and_bound():
    for name in ('isc_linear_f16_native', 'isc_h3_f16a_launches', 'isc_f16_to_f32', 'isc_f16_convert_launches'):
        assert name in _lib.SIGNATURES
        assert name in open(os.path.join(ROOT, 'include', 'insenticap_hip.h')).read()
    lib = _lib.load()
    assert lib.isc_h3_f16a_launches() >= 0 and lib.isc_f16_convert_launches() >= 0
    # argument checks come before any launch (no device needed)
    assert lib.isc_f16_to_f32(None, 8, None, 8, 1, 8, None) == -1
    assert lib.isc_linear_f16_native(None, 1, None) == 0
    pr = _lib.LinearProblem()
    pr.nseg, pr.M, pr.N = 1, 8, 32
    pr.seg[0].A, pr.seg[0].W, pr.seg[0].lda, pr.seg[0].ldw, pr.seg[0].K, pr.seg[0].a_f16 = 4096, 8192, 32, 32, 32, 1
    lp = _lib.LstmProblem()
    lp.nseg, lp.M, lp.H = 1, 8, 32
    lp.seg[0].A, lp.seg[0].W, lp.seg[0].lda, lp.seg[0].ldw, lp.seg[0].K, lp.seg[0].a_f16 = 4096, 8192, 32, 32, 32, 1
    assert lib.isc_lstm_fwd(ctypes.byref(lp), None) == -2         # ISC_E_SHAPE: never halfs read as floats
    arr = (_lib.LinearProblem * 1)(pr)
    pr.C = 4096
    arr = (_lib.LinearProblem * 1)(pr)
    assert lib.isc_gemm_bwd(arr, 1, 0, None) == -2
    arr[0].seg[0].lda = 36                                        # lda % 8 != 0: ISC_E_ALIGN from the forward entry
    assert lib.isc_linear_fwd(arr, 1, None) == -3
