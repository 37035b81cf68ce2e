#!/usr/bin/env python3
"""Generator of tests/golden/sw/reward.npz.  Runs only where the upstream reference is mounted (INSENTICAP_REFERENCE,
default /root/reference): it imports the reference's `self_critical.utils.get_senti_words_reward` *unmodified* and records
what it returns.  The fixture holds token ids, labels, the lexicons as arrays and the reference's results - no reference
source, bytecode or pickle.

    python tests/golden/make_sw_golden.py

Per case c<k>: c<k>_tok int64 [B, T], c<k>_labels int64 [B], c<k>_dims int64 [2] = (V, n_labels), the lexicon as
c<k>_lex_label / c<k>_lex_word int64 [E] and c<k>_lex_weight float64 [E] (an entry per word; every label 0 .. n_labels - 1
has a dict, possibly empty), c<k>_rewards float64 [B, T] and the accur_w members as c<k>_acc_label / c<k>_acc_word int64
[M], sorted.  `n_cases` int64 [1].

  c0  three labels, label 1 with an EMPTY lexicon; word 5 in the lexicons of labels 0 and 2 with different weights; the
      weights are powers of 0.9 formed by repeated multiplication in Python; rows end in <EOS> (2) with further words -
      lexicon words among them - behind it.
  c1  the lexicon holds the <PAD> id 0, the rows are padded with it behind <EOS>: every pad position is paid ("nothing is
      masked").
  c2  T = 1."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('INSENTICAP_REFERENCE', '/root/reference')
sys.path.insert(0, REF)

from self_critical.utils import get_senti_words_reward  # noqa: E402  (reference)

PAD, SOS, EOS = 0, 1, 2


def powers(base, n):
    out, x = [], 1.0
    for _ in range(n):
        out.append(x)
        x *= base
    return out


def case0():
    V, T, B = 30, 12, 24
    p = powers(0.9, 9)
    lex = {0: {5: p[0], 7: p[1], 11: p[4], 29: p[8]}, 1: {}, 2: {5: p[3], 6: p[2], 12: p[7], 3: p[5]}}
    rng = np.random.default_rng(41)
    tok = rng.integers(3, V, size=(B, T))
    for i in range(B):                                     # <EOS> somewhere, the draws behind it stay as they are
        tok[i, rng.integers(1, T)] = EOS
    tok[0, :] = 5                                          # every position the shared word
    tok[1, -3:] = (EOS, 5, 7)                              # lexicon words behind <EOS>
    labels = rng.integers(0, 3, size=B)
    labels[:3] = (2, 0, 1)
    return V, 3, lex, tok, labels


def case1():
    V, T, B = 17, 7, 9
    lex = {0: {PAD: 0.5, 4: 1.0}, 1: {9: 0.9 * 0.9}}
    rng = np.random.default_rng(42)
    tok = rng.integers(3, V, size=(B, T))
    for i in range(B):
        n = rng.integers(1, T)
        tok[i, n] = EOS
        tok[i, n + 1:] = PAD
    return V, 2, lex, tok, rng.integers(0, 2, size=B)


def case2():
    V, B = 8, 5
    lex = {0: {3: 1.0, 4: 0.9}}
    return V, 1, lex, np.asarray([[3], [4], [5], [0], [3]]), np.zeros(B, dtype=np.int64)


def main():
    out = {}
    cases = [case0(), case1(), case2()]
    for k, (V, n_labels, lex, tok, labels) in enumerate(cases):
        tok, labels = tok.astype(np.int64), labels.astype(np.int64)
        rewards, accur_w = get_senti_words_reward(torch.from_numpy(tok), torch.from_numpy(labels), lex)
        assert rewards.shape == tok.shape and rewards.dtype == np.float64
        entries = [(lab, w, x) for lab in sorted(lex) for w, x in sorted(lex[lab].items())]
        acc = sorted((int(lab), int(w)) for lab, ws in accur_w.items() for w in ws)
        c = 'c%d_' % k
        out[c + 'tok'], out[c + 'labels'] = tok, labels
        out[c + 'dims'] = np.asarray([V, n_labels], dtype=np.int64)
        out[c + 'lex_label'] = np.asarray([e[0] for e in entries], dtype=np.int64)
        out[c + 'lex_word'] = np.asarray([e[1] for e in entries], dtype=np.int64)
        out[c + 'lex_weight'] = np.asarray([e[2] for e in entries], dtype=np.float64)
        out[c + 'rewards'] = rewards
        out[c + 'acc_label'] = np.asarray([a[0] for a in acc], dtype=np.int64)
        out[c + 'acc_word'] = np.asarray([a[1] for a in acc], dtype=np.int64)
        print('case %d: %s rows, %d paid positions, %d words used' % (k, tok.shape, int((rewards != 0).sum()), len(acc)))
    out['n_cases'] = np.asarray([len(cases)], dtype=np.int64)
    os.makedirs(os.path.join(HERE, 'sw'), exist_ok=True)
    path = os.path.join(HERE, 'sw', 'reward.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
