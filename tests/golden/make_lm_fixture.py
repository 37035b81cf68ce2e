#!/usr/bin/env python3
"""Generator of tests/golden/lm/reward.npz.  Runs only where the upstream reference is mounted (INSENTICAP_REFERENCE,
default /root/reference): it imports the reference's `self_critical.utils.get_lm_reward` *unmodified* and hands it, as
`lms`, objects with KenLM's `score(sentence)` / `perplexity(sentence)` interface that answer from the fp64 restatement
of tests/_lm_ref.py (no KenLM or SRILM binary is available: the fixture pins the reference's reward FORMULA - string
normalisation, label lookup, sign, repetition over T - not those programs' numbers).  The fixture holds token ids, the
seeds of the three random models and the reference's results - no reference source, bytecode or pickle.

    python tests/golden/make_lm_fixture.py

sample / greedy int32 [B, T], labels int32 [B], seeds int32 [3]; sign float64 [B, T]: what get_lm_reward returns (its
active line); ppl_diff float64 [B, T]: its commented alternative, `perplexity(greedy) - perplexity(sample)`, evaluated
with the same objects and repeated over T as the function repeats its scores."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('INSENTICAP_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

from self_critical.utils import _array_to_str, get_lm_reward  # noqa: E402  (reference)

import _lm_ref as R  # noqa: E402

V, SOS, EOS, B, T = 40, 1, 2, 48, 12
SEEDS = (81, 82, 83)


class RestatedLM:
    """kenlm.Model's two calls over a sentence of ids: <s> in front, every word scored, then </s>."""

    def __init__(self, seed):
        self.grams = R.random_lm(seed, V, 3, with_unk=True)
        self.order, self.table, _ = R.parse_arpa(R.write_arpa(self.grams), V)

    def score(self, sentence):
        return R.score_row(self.table, self.order, [int(w) for w in sentence.split()], V, SOS, EOS, 'word', True)[0]

    def perplexity(self, sentence):
        words = len(sentence.split()) + 1
        return 10.0 ** (-self.score(sentence) / words)


def main():
    lms = {i: RestatedLM(s) for i, s in enumerate(SEEDS)}
    rng = np.random.default_rng(80)
    labels = rng.integers(0, 3, size=B)
    sample = np.stack([R.walk_rows(lms[int(l)].grams, 1, T, V, SOS, EOS, seed=1000 + i)[0] for i, l in enumerate(labels)])
    greedy = np.stack([R.walk_rows(lms[int(l)].grams, 1, T, V, SOS, EOS, seed=2000 + i)[0] for i, l in enumerate(labels)])
    greedy[::6] = sample[::6]                              # equal captions: sign 0
    sign = get_lm_reward(torch.from_numpy(sample), torch.from_numpy(greedy), torch.from_numpy(labels), SOS, EOS, lms)
    diff = np.asarray([lms[int(l)].perplexity(_array_to_str(g, SOS, EOS)) - lms[int(l)].perplexity(_array_to_str(s, SOS, EOS))
                       for s, g, l in zip(sample, greedy, labels)])
    assert sign.shape == (B, T) and set(np.unique(sign)) == {-1.0, 0.0, 1.0}
    out = dict(sample=sample.astype(np.int32), greedy=greedy.astype(np.int32), labels=labels.astype(np.int32),
               seeds=np.asarray(SEEDS, dtype=np.int32), sign=sign.astype(np.float64),
               ppl_diff=np.repeat(diff[:, None], T, 1).astype(np.float64))
    path = os.path.join(HERE, 'lm', 'reward.npz')
    np.savez_compressed(path, **out)
    print('lm reward: sign counts', {v: int((sign[:, 0] == v).sum()) for v in (-1.0, 0.0, 1.0)}, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
