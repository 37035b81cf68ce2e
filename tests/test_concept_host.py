"""The concept detector's Python surface on the CPU (the torch path): helper_nets.ConceptDetector / MultiLabelClsLoss
against the fixture the reference wrote (tests/golden/concept.npz, ref_concept_checkpoint_tiny.ckpt), the checkpoint round
trip, the concept collate and dataset, data.SentimentWordTable.lookup against the restatement (tests/_concept_ref.py -
a hand restatement of preprocess.py:288-301: preprocess.py cannot be imported where the fixture is made), the error
cases, the table cap and tag_concepts."""
import os

import numpy as np
import pytest
import torch

import _concept_ref as R
from conftest import GOLDEN_DIR
from insenticap_model_amd import FusedClampAdam, _lib, checkpoint, clip_gradient, data, ops
from insenticap_model_amd.helper_nets import ConceptDetector, MultiLabelClsLoss

SETTINGS = {'fc_feat_dim': 64, 'concept_mid_him': 32, 'dropout_p': 0.0}
IDX2CONCEPT = ['cpt%d' % i for i in range(20)]


def _model(g):
    m = ConceptDetector(IDX2CONCEPT, SETTINGS)
    m.load_state_dict({k: torch.from_numpy(g['sd/' + k]) for k in R.NAMES})
    return m


def test_names_outputs_and_the_sample_triple_equal_the_reference(golden):
    g = golden('concept')
    m = _model(g)
    assert list(m.state_dict()) == list(R.NAMES)
    assert isinstance(m.output[4], torch.nn.Dropout) and isinstance(m.output[5], torch.nn.Linear)
    feats = torch.from_numpy(g['feats'])
    m.eval()
    assert not m.native_active(feats)                        # CPU tensors: the torch path
    with torch.no_grad():
        assert torch.equal(m(feats), torch.from_numpy(g['probs']))
    out, concepts, scores = m.sample(feats, 5)
    assert torch.equal(out, torch.from_numpy(g['probs']))
    assert concepts == [[IDX2CONCEPT[i] for i in row] for row in g['sample_idx'].tolist()]
    assert torch.equal(scores, torch.from_numpy(g['sample_scores']))
    m.set_vocabulary({c: 100 + i for i, c in enumerate(IDX2CONCEPT)})
    idx, sc, words = m.sample_device(feats, 5)
    assert np.array_equal(idx.numpy(), g['sample_idx']) and np.array_equal(words.numpy(), g['sample_idx'] + 100)
    assert torch.equal(sc, scores)


def test_loss_gradients_and_two_steps_equal_the_reference(golden):
    """The drop-in form of train_cpt.py:79-89 on the torch path.  FusedClampAdam's update is a device kernel, so the two
    steps here go through torch.optim.Adam with the package's clip_gradient; the fused step is held to the same numbers
    on the device (tests/test_gpu_concept.py)."""
    g = golden('concept')
    m = _model(g)
    opt, crit = m.get_optim_criterion(float(g['hyper'][0]))
    assert isinstance(opt, FusedClampAdam) and isinstance(crit, MultiLabelClsLoss)
    opt = torch.optim.Adam(m.parameters(), lr=float(g['hyper'][0]))
    feats, targets = torch.from_numpy(g['feats']), torch.from_numpy(g['targets'])
    m.train()
    for it in (1, 2):
        loss = crit(m(feats), targets)
        assert abs(float(loss.detach()) - g['loss'][it - 1]) <= 1e-6 * g['loss'][it - 1]
        opt.zero_grad()
        loss.backward()
        for k, p in m.named_parameters():
            ref = g['grad%d/%s' % (it, k)]
            assert np.abs(p.grad.numpy() - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-9, (it, k)
        clip_gradient(opt, float(g['hyper'][1]))
        opt.step()
    for k, v in m.state_dict().items():
        assert np.abs(v.numpy() - g['after2/' + k]).max() <= 1e-6, k


def test_checkpoint_round_trip_and_the_reference_written_file(golden, tmp_path):
    g = golden('concept')
    ref_file = os.path.join(GOLDEN_DIR, 'ref_concept_checkpoint_tiny.ckpt')
    m, epoch, lr = checkpoint.load_concept_checkpoint(ref_file)
    assert epoch == 1 and lr is None and m.idx2concept == IDX2CONCEPT
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), g['after2/' + k]), k
    opt = torch.optim.Adam(m.parameters(), lr=1.0)
    _, _, lr = checkpoint.load_concept_checkpoint(ref_file, m, opt, settings=SETTINGS, idx2concept=IDX2CONCEPT,
                                                  dataset_name='tiny')
    assert lr == float(g['hyper'][0]) and int(opt.state_dict()['state'][0]['step']) == 2
    with pytest.raises(AssertionError):
        checkpoint.load_concept_checkpoint(ref_file, m, dataset_name='other')
    path = checkpoint.save_concept_checkpoint(str(tmp_path), 3, m, opt, SETTINGS, IDX2CONCEPT, 'tiny', 0.5, 0.25)
    assert os.path.basename(path).startswith('model_3_0.5000_0.2500_')
    chk = torch.load(path, weights_only=False)
    assert sorted(chk) == ['dataset_name', 'epoch', 'idx2concept', 'model', 'optimizer', 'settings']    # train_cpt.py:140-147
    m2, epoch2, _ = checkpoint.load_concept_checkpoint(path)
    assert epoch2 == 3 and all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))


def test_concept_collate_dataset_and_loader(golden):
    g = golden('concept')
    fns = [str(x) for x in g['collate_fns']]
    store = {fn: g['feats'][i] for i, fn in enumerate(fns)}
    img_concepts = {fn: [int(j) for j in np.nonzero(g['targets'][i])[0]] for i, fn in enumerate(fns)}
    ds = data.ConceptDataset(store, img_concepts, 20)
    assert len(ds) == 6 and ds[0][2].dtype == np.int16
    out_fns, fc, cpts = data.concept_collate_fn([ds[i] for i in range(6)])
    assert list(out_fns) == fns and fc.dtype == torch.float32 and cpts.dtype == torch.int64
    assert np.array_equal(fc.numpy(), g['collate_fc']) and np.array_equal(cpts.numpy(), g['targets'])
    loader = data.get_concept_dataloader(store, img_concepts, 20, batch_size=4, shuffle=False)
    batches = list(loader)
    assert [len(b[0]) for b in batches] == [4, 2] and np.array_equal(batches[1][2].numpy(), g['targets'][4:])


def _table_case():
    rng = np.random.default_rng(5)
    idx2concept = ['c%d' % i for i in range(12)]
    words = ['w%d' % i for i in range(30)]
    word2idx = {w: 4 + i for i, w in enumerate(words)}
    sd = {}
    for i, c in enumerate(idx2concept):
        if i % 4 == 3:
            continue                                        # concepts without a list
        n = int(rng.integers(0, 9))
        sd[c] = [[words[int(rng.integers(0, 30))], float(rng.integers(1, 5)) / 4.0] for _ in range(n)]     # ties on purpose
    return idx2concept, word2idx, sd


def test_sentiment_word_table_lookup_equals_the_restatement():
    idx2concept, word2idx, sd = _table_case()
    table = data.SentimentWordTable(sd, word2idx, idx2concept)
    lists = [[(word2idx[w], s) for w, s in sd.get(c, [])] for c in idx2concept]
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 12, size=(40, 5))
    names = [[idx2concept[c] for c in row] for row in rows]
    for n_out in (1, 10, 20):
        ref = R.senti_words(rows, lists, n_out, 0)
        assert np.array_equal(table.lookup_tensor(names, n_out, 0).numpy(), ref)
    got = table.lookup(names)
    assert all(len(x) <= 20 for x in got) and got[0] == [int(x) for x in R.senti_words(rows[:1], lists, 20, -1)[0] if x >= 0]
    assert table.lookup([['not a concept'], []]) == [[], []]


def test_key_and_value_errors():
    idx2concept, word2idx, sd = _table_case()
    m = ConceptDetector(idx2concept, SETTINGS)
    with pytest.raises(KeyError):
        m.set_vocabulary({c: i for i, c in enumerate(idx2concept[:-1])})       # a concept the vocabulary lacks
    with pytest.raises(KeyError):
        data.SentimentWordTable({'c0': [['unknown word', 1.0]]}, word2idx, idx2concept)
    feats = torch.zeros(2, 64)
    for bad in (0, 13, 17, -1):                              # 12 concepts: num in [1, 12]
        with pytest.raises(ValueError):
            m.sample(feats, bad)
        with pytest.raises(ValueError):
            m.sample_device(feats, bad)
    with pytest.raises(ValueError):
        data.SentimentWordTable(sd, word2idx).forward(torch.zeros(1, 5, dtype=torch.int64))      # no idx2concept
    from insenticap_model_amd import Detector, synth
    det = Detector(synth.make_idx2word(40), 8, synth.SENTIMENT_CATEGORIES, {'cap_lr': 1e-4},
                   dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS))
    with pytest.raises(ValueError):
        det.sample(torch.zeros(64), torch.zeros(4, 64))      # sentis_tensor=None and no table
    with pytest.raises(ValueError):
        det.set_concept_detector(m)                          # no vocabulary yet
    assert 'concept_detector' not in dict(det.named_modules()) and not any('concept' in k for k in det.state_dict())


def test_the_table_cap_is_rejected_not_truncated():
    cap = _lib.load().isc_senti_words_cap()
    assert cap == ops.SENTI_WORDS_CAP == 1024
    word2idx = {'w%d' % i: i for i in range(300)}
    at_cap = {'c0': [['w%d' % (i % 300), 1.0] for i in range(cap // 4)]}
    table = data.SentimentWordTable(at_cap, word2idx, ['c0', 'c1'], num_concepts=4)        # 4 x 256 = the cap: fine
    assert table.max_list == cap // 4
    with pytest.raises(ValueError):
        data.SentimentWordTable(at_cap, word2idx, ['c0', 'c1'], num_concepts=5)
    over = {'c0': [['w%d' % (i % 300), 1.0] for i in range(cap // 4 + 1)]}
    with pytest.raises(ValueError):
        data.SentimentWordTable(over, word2idx, ['c0', 'c1'], num_concepts=4)
    assert ops.senti_words_pack_check([0, 5, 5, 9], 16) == 5
    # the host form has no cap
    assert len(data.SentimentWordTable(over, word2idx).lookup([['c0']])[0]) == 20


def test_tag_concepts_dictionary(golden):
    g = golden('concept')
    m = _model(g)
    fns = [str(x) for x in g['collate_fns']]
    store = {fn: g['feats'][i] for i, fn in enumerate(fns)}
    tags = data.tag_concepts(m, store, 5, batch=4)
    assert list(tags) == fns
    assert tags == {fn: [IDX2CONCEPT[j] for j in g['sample_idx'][i]] for i, fn in enumerate(fns)}


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """No device is touched: the checks run on the host and return before the first launch."""
    import ctypes as C
    lib = _lib.load()
    buf = (C.c_char * 4096)()
    p = C.addressof(buf) // 16 * 16 + 16                     # any aligned non-null address: never dereferenced
    head = lambda B, Cn, num, ld=None, logits=p, words=None, table=None, hits=None, targets=None: lib.isc_concept_head(
        logits, Cn if ld is None else ld, B, Cn, num, None, p, p, table, words, targets, 0, hits, None, None)
    assert head(2, 20, 0) == head(2, 20, 17) == head(2, 5, 6) == head(0, 20, 1) == head(2, 0, 1) == -2      # ISC_E_SHAPE
    assert head(2, 20, 5, ld=19) == -2
    assert head(2, 20, 5, logits=None) == -1 and head(2, 20, 5, words=p) == -1 and head(2, 20, 5, hits=p) == -1
    assert lib.isc_concept_loss(p, 20, 2, 20, p, 0, 1.0, p, 8, p, None, None) == -4                         # workspace
    assert lib.isc_concept_loss(p, 20, 2, 20, None, 0, 1.0, p, 64, p, None, None) == -1
    assert lib.isc_concept_loss_workspace_bytes(80) == 80 * 16
    words = lambda num, longest, n_out: lib.isc_senti_words_from_concepts(p, num, 3, num, 10, p, p, p, longest, n_out, 0,
                                                                          p, None)
    assert words(5, 205, 10) == words(17, 1, 10) == words(5, 10, 21) == words(5, 10, 0) == -2
    assert lib.isc_concept_workspace_bytes(4, 64, 32, 20) > 0
    assert lib.isc_concept_workspace_bytes(4, 48, 32, 20) == lib.isc_concept_workspace_bytes(4, 64, 40, 20) == 0
    q = _lib.ConceptProblem()
    assert lib.isc_concept_fwd(C.byref(q), None) == -1 and lib.isc_concept_fwd(None, None) == -1
    for name in ('feats', 'w0', 'b0', 'w2', 'b2', 'w5', 'b5', 'workspace'):
        setattr(q, name, p)
    q.B, q.F, q.H, q.C, q.num, q.feats_ld, q.workspace_bytes = 4, 48, 32, 20, 5, 48, 1 << 30
    assert lib.isc_concept_fwd(C.byref(q), None) == -2       # fc_feat_dim % 32 != 0
    q.F, q.feats_ld, q.num = 64, 64, 21
    assert lib.isc_concept_fwd(C.byref(q), None) == -2       # num > C
    q.num, q.workspace_bytes = 5, 64
    assert lib.isc_concept_fwd(C.byref(q), None) == -4


def test_concept_problem_layout_matches_c(tmp_path):
    import ctypes
    import subprocess
    from conftest import ROOT
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "insenticap_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(isc_concept_problem), offsetof(isc_concept_problem, feats_f16),
         offsetof(isc_concept_problem, w0), offsetof(isc_concept_problem, workspace_bytes),
         offsetof(isc_concept_problem, splitk_ws_floats), offsetof(isc_concept_problem, words));
  printf("%d %d %d\n", ISC_CONCEPT_MAX_NUM, ISC_SENTI_WORDS_CAP, ISC_SENTI_WORDS_MAX_OUT);
  return 0;
}
'''
    cfile, exe = str(tmp_path / 'layout.c'), str(tmp_path / 'layout')
    open(cfile, 'w').write(prog)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), cfile, '-o', exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    P = _lib.ConceptProblem
    assert got == [ctypes.sizeof(P), P.feats_f16.offset, P.w0.offset, P.workspace_bytes.offset, P.splitk_ws_floats.offset,
                   P.words.offset, _lib.CONCEPT_MAX_NUM, _lib.SENTI_WORDS_CAP, _lib.SENTI_WORDS_MAX_OUT]
