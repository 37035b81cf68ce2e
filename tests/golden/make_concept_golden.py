#!/usr/bin/env python3
"""Generator of tests/golden/concept.npz and tests/golden/ref_concept_checkpoint_tiny.ckpt.  Runs only where the upstream
reference is mounted (INSENTICAP_REFERENCE, default /root/reference): it imports the reference's `ConceptDetector`,
`MultiLabelClsLoss` (models/concept_detector.py) and its 'concept' collate (dataloader.py:111-115) *unmodified* and
records what they compute at tiny widths.  Nothing of this project is imported: the fixture holds tensors, names and
numbers - no reference source, bytecode or pickled class.

    python tests/golden/make_concept_golden.py

`dataloader.py` imports h5py at module level, which may be absent; only its Dataset classes touch it.  As
make_golden.py::case_collate does, the module is imported with an empty module object registered as `h5py`; the items
handed to the collate are built the way ConceptDataset.__getitem__ builds them (an int16 0/1 vector per image).
`preprocess.py` cannot be imported here (nltk, skimage and its option parser at import time), so the sentiment-word
aggregation of preprocess.py:288-301 is NOT recorded: tests/_concept_ref.py restates it by hand.

Recorded (fc 64 / mid 32 / 20 concepts, 6 images, dropout_p = 0, lr 1e-2, grad_clip 0.1):
  sd/<name>             the state_dict at the start, by name          feats [6, 64]
  probs [6, 20]         forward(feats)                                 sample_idx [6, 5], sample_scores [6, 5] (sample, num=5)
  targets [6, 20]       the collate's 0/1 matrix (int64)               collate_fc [6, 64], collate_fns
  loss [2]              MultiLabelClsLoss in front of step 1 and 2     grad1/<name>, grad2/<name> (before the clamp)
  after2/<name>         parameters after two clip_gradient + Adam steps"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('INSENTICAP_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
sys.modules.setdefault('h5py', types.ModuleType('h5py'))

from models.concept_detector import ConceptDetector, MultiLabelClsLoss  # noqa: E402,F401  (reference)
import dataloader as ref_dl  # noqa: E402  (reference)

SETTINGS = {'fc_feat_dim': 64, 'concept_mid_him': 32, 'dropout_p': 0.0}
C, B, NUM, LR, CLIP = 20, 6, 5, 1e-2, 0.1


def clamp_gradients(optim, clip):
    """What train_cpt.py does between backward and step: every gradient clamped elementwise to +-clip, in place."""
    for group in optim.param_groups:
        for prm in group['params']:
            if prm.grad is not None:
                prm.grad.data.clamp_(-clip, clip)


def main():
    torch.manual_seed(20)
    rng = np.random.default_rng(20)
    idx2concept = ['cpt%d' % i for i in range(C)]
    model = ConceptDetector(idx2concept, SETTINGS)
    with torch.no_grad():                                   # wider logits than the default init gives: distinct top-5
        for p in model.parameters():
            p.mul_(3.0)
    out = {}
    for k, v in model.state_dict().items():
        out['sd/' + k] = v.detach().numpy().copy()

    # items as ConceptDataset.__getitem__ builds them, through the reference's collate
    items = []
    for i in range(B):
        cpts_idx = sorted(int(x) for x in rng.choice(C, size=int(rng.integers(1, 6)), replace=False))
        vec = np.zeros(C, dtype=np.int16)
        vec[cpts_idx] = 1
        items.append(('img%d.jpg' % i, rng.random(SETTINGS['fc_feat_dim'], dtype=np.float32) * 2.0, vec))
    fns, fc_feats, targets = ref_dl.create_collate_fn('concept')(items)
    out['collate_fns'] = np.asarray(fns)
    out['collate_fc'] = fc_feats.numpy().copy()
    out['targets'] = targets.numpy().copy()
    out['feats'] = np.stack([it[1] for it in items])

    model.eval()
    with torch.no_grad():
        out['probs'] = model(fc_feats).numpy().copy()
        probs, concepts, scores = model.sample(fc_feats, num=NUM)
    out['sample_idx'] = np.asarray([[idx2concept.index(c) for c in row] for row in concepts], dtype=np.int64)
    out['sample_scores'] = scores.numpy().copy()

    model.train()
    optimizer, criterion = model.get_optim_criterion(LR)
    losses = []
    for step in (1, 2):
        pred = model(fc_feats)
        loss = criterion(pred, targets)
        losses.append(float(loss))
        optimizer.zero_grad()
        loss.backward()
        for k, p in model.named_parameters():
            out['grad%d/%s' % (step, k)] = p.grad.detach().numpy().copy()
        clamp_gradients(optimizer, CLIP)
        optimizer.step()
    out['loss'] = np.asarray(losses, dtype=np.float64)
    for k, v in model.state_dict().items():
        out['after2/' + k] = v.detach().numpy().copy()
    out['hyper'] = np.asarray([LR, CLIP, NUM], dtype=np.float64)

    np.savez_compressed(os.path.join(HERE, 'concept.npz'), **out)
    # the checkpoint as train_cpt.py:140-147 lays it out, written by the reference's own objects (torch.save's format)
    torch.save({'epoch': 1, 'model': model.state_dict(), 'optimizer': optimizer.state_dict(), 'settings': SETTINGS,
                'idx2concept': idx2concept, 'dataset_name': 'tiny'},
               os.path.join(HERE, 'ref_concept_checkpoint_tiny.ckpt'))
    print('concept: %d arrays, %d bytes; checkpoint %d bytes; losses %r' % (
        len(out), os.path.getsize(os.path.join(HERE, 'concept.npz')),
        os.path.getsize(os.path.join(HERE, 'ref_concept_checkpoint_tiny.ckpt')), losses))
    p = out['probs']
    srt = -np.sort(-p, axis=1)
    print('smallest gap among the top %d probabilities: %.3g' % (NUM + 1, np.min(srt[:, :NUM] - srt[:, 1:NUM + 1])))


if __name__ == '__main__':
    main()
