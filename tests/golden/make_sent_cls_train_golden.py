#!/usr/bin/env python3
"""Generator of tests/golden/sent_cls_train.npz and tests/golden/ref_sent_cls_checkpoint_tiny.ckpt.  Runs only where the
upstream reference is mounted (INSENTICAP_REFERENCE, default /root/reference): it imports the reference's
`SentenceSentimentClassifier` (models/sent_senti_cls.py - it needs only torch) and its 'senti_sents' collate
(dataloader.py:123-134) *unmodified* and records what they compute at tiny widths.  The fixture holds tensors, names and
numbers - no reference source, bytecode or pickled class.

    python tests/golden/make_sent_cls_train_golden.py

From this project it takes only the deterministic weight generator (insenticap_model_amd.synth.make_module_weights(shapes,
52, gain=6.0)) and the input draw of tests/_sent_cls_train_ref.py (draw_inputs / find_seed: the first input seed >= 7 whose
ReLU pre-activations keep clear of zero), so that the tests can rebuild the same inputs.
`dataloader.py` imports h5py at module level, which may be absent; only its Dataset classes touch it.  As
make_golden.py::case_collate does, the module is imported with an empty module object registered as `h5py`; the items handed
to the collate are built the way SentiSentDataset.__getitem__ builds them ((label, np.array(ids))).
`train_sent_senti_cls_rnn.py` cannot be imported (its option parser and tqdm at import time), so the corpus split of its
lines 69-95 is NOT recorded: data.build_senti_sents_sets restates it by hand and tests/test_sent_cls_data_host.py holds it
to the split worked out independently on sentence positions.

Recorded (W = H = 32, V = 64, k = 3, B = 37, L = 8, dropout_p = 0, lr 4e-4, grad_clip 0.1):
  sd/<name>          the state_dict at the start           tokens [37, 8], lens [37], labels [37], seed
  loss [2]           CrossEntropyLoss in front of step 1 and 2          grad1/<name> (before the clamp)
  after2/<name>      parameters after two clip_gradient + Adam steps
  collate_*          five (label, ids) items through the reference's collate at max_seq_len = 6, pad_index = 0"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('INSENTICAP_REFERENCE', '/root/reference')
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.modules.setdefault('h5py', types.ModuleType('h5py'))

from models.sent_senti_cls import SentenceSentimentClassifier  # noqa: E402  (reference)
import dataloader as ref_dl  # noqa: E402  (reference)
from insenticap_model_amd import synth  # noqa: E402
import _sent_cls_train_ref as R  # noqa: E402

SETTINGS = {'word_emb_dim': 32, 'rnn_hid_dim': 32, 'dropout_p': 0.0}
V, K, B, L, LR, CLIP = 64, 3, 37, 8, 4e-4, 0.1
CATEGORIES = ['positive', 'negative', 'neutral']


def clamp_gradients(optim, clip):
    """train_sent_senti_cls_rnn.py:24-28."""
    for group in optim.param_groups:
        for prm in group['params']:
            if prm.grad is not None:
                prm.grad.data.clamp_(-clip, clip)


def main():
    idx2word = synth.make_idx2word(V)
    model = SentenceSentimentClassifier(idx2word, CATEGORIES, SETTINGS)
    shapes = {n: tuple(v.shape) for n, v in model.state_dict().items()}
    w = synth.make_module_weights(shapes, 52, gain=6.0)
    model.load_state_dict({n: torch.from_numpy(v) for n, v in w.items()})
    out = {'sd/' + k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    seed = R.find_seed(w, V, B, L, K)
    tokens, lens, labels = R.draw_inputs(seed, V, B, L, K)
    out.update(tokens=tokens, lens=np.asarray(lens, dtype=np.int64), labels=labels, seed=np.asarray([seed]))

    model.train()
    optimizer, criterion = model.get_optim_and_crit(LR)
    losses = []
    for step in (1, 2):
        pred, _ = model(torch.from_numpy(tokens), lens)
        loss = criterion(pred, torch.from_numpy(labels))
        losses.append(float(loss.detach()))
        optimizer.zero_grad()
        loss.backward()
        if step == 1:
            for k, p in model.named_parameters():
                out['grad1/' + k] = p.grad.detach().numpy().copy()
        clamp_gradients(optimizer, CLIP)
        optimizer.step()
    out['loss'] = np.asarray(losses, dtype=np.float64)
    for k, v in model.state_dict().items():
        out['after2/' + k] = v.detach().numpy().copy()
    out['hyper'] = np.asarray([LR, CLIP], dtype=np.float64)

    # five items through the reference's collate: unsorted lengths, two equal ones (stable order), one beyond max_seq_len
    rng = np.random.default_rng(20)
    item_lens = [3, 9, 5, 5, 1]
    items = [(int(rng.integers(0, K)), np.array(rng.integers(4, V, n))) for n in item_lens]
    out['collate_in_labels'] = np.asarray([it[0] for it in items], dtype=np.int64)
    out['collate_in_ids'] = np.asarray([np.pad(it[1], (0, 9 - len(it[1])), constant_values=-1) for it in items])
    sentis, (caps_tensor, lengths) = ref_dl.create_collate_fn('senti_sents', pad_index=0, max_seq_len=6)(list(items))
    out['collate_labels'] = sentis.numpy().copy()
    out['collate_caps'] = caps_tensor.numpy().copy()
    out['collate_lengths'] = np.asarray(lengths, dtype=np.int64)

    np.savez_compressed(os.path.join(HERE, 'sent_cls_train.npz'), **out)
    # the checkpoint as train_sent_senti_cls_rnn.py:178-187 lays it out, written by the reference's own objects
    ckpt = os.path.join(HERE, 'ref_sent_cls_checkpoint_tiny.ckpt')
    torch.save({'epoch': 1, 'model': model.state_dict(), 'optimizer': optimizer.state_dict(), 'settings': SETTINGS,
                'idx2word': idx2word, 'sentiment_categories': CATEGORIES, 'dataset_name': 'tiny', 'corpus_type': 'part'},
               ckpt)
    print('sent_cls_train: seed %d, %d arrays, %d bytes; checkpoint %d bytes; losses %r' % (
        seed, len(out), os.path.getsize(os.path.join(HERE, 'sent_cls_train.npz')), os.path.getsize(ckpt), losses))


if __name__ == '__main__':
    main()
