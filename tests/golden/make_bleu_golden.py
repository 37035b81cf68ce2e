#!/usr/bin/env python3
"""Generator of tests/golden/bleu.npz.  Runs only where the upstream reference is mounted (INSENTICAP_REFERENCE, default
/root/reference): it imports the reference's `self_critical.bleu.bleu.Bleu` *unmodified*, hands it the captions as the
strings utils._array_to_str writes, and records what it returns.  Nothing of this project is imported: the fixture
holds the token ids of two sets and the reference's results for them - no reference source, bytecode or pickle.

    python tests/golden/make_bleu_golden.py

Per set `name`: name/hyps int32 [N, T] raw roll-out rows (row r belongs to image r % I), the I images' references
flattened (name/ref_tokens, name/ref_cap_off, name/ref_img_off), name/scores float64 [N, 4] - the four per-sentence
lists as columns - and name/corpus float64 [4].
  small: 6 images built by hand with the edge rows of the scorer among 36 rows, T = 12;
  cfg5:  512 images x 5 references, 1024 rows, T = 20, V = 10 000, seeded random ids."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('INSENTICAP_REFERENCE', '/root/reference')
sys.path.insert(0, REF)

from self_critical.bleu.bleu import Bleu  # noqa: E402  (reference)

PAD, SOS, EOS = 0, 1, 2


def _words(arr):
    """utils._array_to_str as a list of ids."""
    arr = [int(x) for x in arr]
    if arr[0] == SOS:
        arr = arr[1:]
    out = []
    for w in arr:
        if w == EOS:
            break
        out.append(w)
    return out + [EOS]


def _row(words, T, eos=True):
    row = [int(w) for w in words][:T]
    if eos and len(row) < T:
        row.append(EOS)
    return row + [PAD] * (T - len(row))


def make_small():
    T = 12
    rng = np.random.default_rng(17)
    long_a = [int(x) for x in rng.integers(4, 30, size=40)]
    long_b = long_a[5:30] + [int(x) for x in rng.integers(4, 30, size=20)]
    refs = [
        [[SOS, 4, 5, 6, 7, EOS], [SOS, 4, 5, 8, EOS], [SOS, 9, 4, 5, 6, 7, 10, EOS]],
        [[SOS, 11, 12, 13, EOS]],                                           # one reference
        [[SOS, 7, 7, 5, EOS], [SOS, 7, 7, 7, 6, EOS], [SOS, 5, 6, EOS]],    # one word twice and three times
        [[SOS, 4, 5, 6, EOS], [SOS, 4, 5, 6, 7, 8, EOS]],                   # lengths 4 and 6: a tie for testlen 5
        [[SOS] + long_a + [EOS], [SOS] + long_b + [EOS]],                   # > 128 distinct n-grams
        [[4, 5, 6, 7, 8, 9, 10, 11], [SOS, 0, 65534, 0, EOS]],              # no <SOS> / <EOS>; ids 0 and 65534
    ]
    rows = [
        # image 0
        _row([4, 5, 6, 7], T), _row([SOS, 4, 5, 6, 7], T), _row([4, 5, 8, 6, 7, 10], T), _row([], T),
        _row([20, 21, 22], T), _row([4, 5, 6, 7, 9, 4, 5, 6, 7, 10, 4, 5], T, eos=False),
        # image 1
        _row([11, 12, 13], T), _row([11, 12], T), _row([11, 12, 13, 14], T), _row([SOS, 13, 12, 11], T),
        _row([11], T), _row([], T),
        # image 2: clipping by the max over the references
        _row([7] * 5, T), _row([7] * 12, T, eos=False), _row([7, 7, 5], T), _row([7, 7, 7, 6], T),
        _row([5, 7, 7, 7, 7], T), _row([6, 5, 7], T),
        # image 3: testlen 5 ties 4 against 6 (the shorter wins), ratios below, at and above 1
        _row([4, 5, 6, 7], T), _row([4, 5, 6], T), _row([4, 5], T), _row([4, 5, 6, 7, 8], T),
        _row([4, 5, 6, 7, 8, 9], T), _row([SOS, 4, 5, 6, 7], T),
        # image 4
        _row(long_a[:11], T), _row(long_a[5:17], T, eos=False), _row(long_b[20:29], T), _row(long_a[30:40], T),
        _row([SOS] + long_a[:11], T, eos=False), _row(long_b[-6:], T),
        # image 5
        _row([4, 5, 6, 7, 8, 9, 10, 11], T), _row([0, 65534, 0], T), _row([65534, 0, 65534, 0], T),
        _row([SOS, 0, 0, 0], T), _row([4, 5, 6, 0, 65534], T), _row([9, 10, 11], T),
    ]
    hyps = np.asarray(rows, dtype=np.int64).reshape(6, 6, T).transpose(1, 0, 2).reshape(36, T)      # row r: image r % 6
    return hyps, refs


def make_cfg5():
    I, R, T, V = 512, 5, 20, 10000
    rng = np.random.default_rng(2005)
    refs = [[[SOS] + [int(x) for x in rng.integers(4, V, size=int(rng.integers(5, 19)))] + [EOS] for _ in range(R)]
            for _ in range(I)]
    hyps = np.zeros((2 * I, T), dtype=np.int64)
    for r in range(2 * I):
        base = refs[r % I][int(rng.integers(0, R))][1:-1]
        words = [w if rng.random() < 0.75 else int(rng.integers(4, V)) for w in base]
        kind = r % 6
        if kind == 1:                                   # a leading <SOS>
            words = [SOS] + words
        if kind == 2:                                   # no <EOS>: the row is full
            words = (words * 4)[:T]
        if kind == 3:                                   # shorter than every reference
            words = words[:3]
        hyps[r] = _row(words, T, eos=kind != 2)
    return hyps, refs


def main():
    out = {}
    for name, (hyps, refs) in (('small', make_small()), ('cfg5', make_cfg5())):
        I = len(refs)
        gts = {i: [' '.join(str(w) for w in _words(c)) for c in refs[i]] for i in range(I)}
        res = [{'image_id': r % I, 'caption': [' '.join(str(w) for w in _words(row))]} for r, row in enumerate(hyps)]
        corpus, lists = Bleu(4).compute_score(gts, res)
        assert len(lists) == 4 and all(len(x) == len(hyps) for x in lists)
        out[name + '/hyps'] = hyps.astype(np.int32)
        out[name + '/ref_tokens'] = np.asarray([w for caps in refs for c in caps for w in c], dtype=np.int32)
        out[name + '/ref_cap_off'] = np.cumsum([0] + [len(c) for caps in refs for c in caps]).astype(np.int32)
        out[name + '/ref_img_off'] = np.cumsum([0] + [len(caps) for caps in refs]).astype(np.int32)
        out[name + '/scores'] = np.asarray(lists, dtype=np.float64).T.copy()
        out[name + '/corpus'] = np.asarray(corpus, dtype=np.float64)
        print(name, hyps.shape, 'corpus', corpus, 'BLEU-4 min / max', min(lists[3]), max(lists[3]))
    np.savez_compressed(os.path.join(HERE, 'bleu.npz'), **out)
    print('bleu: %d arrays, %d bytes' % (len(out), os.path.getsize(os.path.join(HERE, 'bleu.npz'))))


if __name__ == '__main__':
    main()
