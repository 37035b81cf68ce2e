"""Cases shared by test_senti_beam_host.py (CPU) and test_gpu_senti_beam.py: one image of a width set of tests/_widths.py
captioned under each sentiment label by the oracle's beam search (decoding_constraint 1, T steps, the image's sentiment
words).  The CPU file asserts what the GPU file rests on: fp32 and fp64 oracle agree on every id sequence, the three
labels give three different results per image (a wrong label index cannot pass), and the final scores of neighbouring
beams are further apart than MARGIN."""
import torch

import _widths as Wd

WIDTH_SETS = ('h_wide', 'all_differ', 'h_768')
IMAGES = (0, 1, 2)
LABELS = (0, 1, 2)
BEAMS = (2, 3)
MARGIN = 2e-3
T = Wd.T
_cache = {}


def oracle(name, image, label, beam, dtype=torch.float64):
    """(captions, scores, ids) of the oracle's beam search of `image` under sentiment `label`; cached."""
    key = (name, image, label, beam, dtype)
    if key not in _cache:
        from oracle import captioner_oracle as O
        st, w, d, _ = Wd.setup(name)
        with torch.no_grad():
            _cache[key] = O.beam_search(O.to_params(w, dtype=dtype), Wd.oracle_ids(), Wd.idx2word(),
                                        Wd.cpu(d, 'fc_feats', dtype=dtype)[image], Wd.cpu(d, 'att_feats', dtype=dtype)[image],
                                        Wd.cpu(d, 'senti_words')[image], torch.tensor([label]), beam, 1, T)
    return _cache[key]


def rotated_labels(n_images, n_labels=len(LABELS)):
    """[I, S] labels, the order rotated per image: the group index differs from the label id."""
    return torch.tensor([[(i + s) % len(LABELS) for s in range(n_labels)] for i in range(n_images)], dtype=torch.int64)
