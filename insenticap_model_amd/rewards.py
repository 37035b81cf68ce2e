"""Rewards and the RL criterion of the reference (self_critical/utils.py), host side of the RL step.

* `RewardCriterion` (utils.py:169-177) - masked REINFORCE loss on [B,T] tensors.
* `get_ciderd_scorer` / `get_self_critical_reward` (utils.py:38-83) - same signatures and return
  values as the reference, computed by the native, multi-threaded CIDEr-D library
  (include/insenticap_cider.h) instead of the pure-Python scorer (~1,240 hypotheses/s/core there,
  the first wall of the RL step once decoding is fast: SURVEY 8(a-19)).
* `get_cls_reward` (utils.py:120-151) - sentence-sentiment-classifier reward.
* `DeviceCiderD` / `get_self_critical_reward_device` - the same CIDEr-D scores formed on the device
  (isc_cider_dev_score) from the host library's table and cooked references; opt-in (Detector.device_cider).
* `Bleu` / `DeviceBleu` / `get_bleu_scorer` - the reference's other scorer (utils.py:75-77: the per-sentence BLEU-4 list
  of self_critical/bleu) in the same library and on the device (isc_bleu_dev_score); every reward function above takes
  either scorer, CIDEr-D stays the default.
* `read_arpa` / `NgramLM` / `NgramLMSet` / `DeviceNgramLMSet`, `get_lm_reward` / `get_lm_reward_device`, `lm_perplexity` -
  the per-sentiment back-off n-gram language models: the reference's dormant LM reward (utils.py:86-100) and its `ppl`
  metric (eval_ppl.py), on the host (isc_lm_score) and on the device (isc_lm_dev_score); opt-in (Detector.lm_flag).
* `get_senti_words_reward` / `SentimentWordWeights` / `senti_word_stats` - the reference's dormant sentiment-word reward
  (utils.py:154-166) on the host and on the device (isc_sw_reward, isc_sw_decay); opt-in (Detector.senti_words_flag).
"""
import ctypes as C
import math
import os

import numpy as np
import torch
import torch.nn as nn

_HERE = os.path.dirname(os.path.abspath(__file__))
CIDER_LIB_PATH = os.path.join(_HERE, 'lib', 'libinsenticap_cider.so')
_cider = None


class RewardCriterion(nn.Module):
    """Masked REINFORCE loss: -sum(logp * mask * reward) / sum(mask) over [B,T] tensors (self_critical/utils.py:
    169-177).  `seq_logprobs` comes from Captioner.forward_rl (differentiable when sampling in train mode).  One HIP
    launch forward (isc_reward_loss_fwd: fixed-order sums, bit-repeatable) and one backward (isc_reward_loss_bwd) whose
    [B,T] result reaches the roll-out's BPTT as (drawn token, weight) pairs - no [B,T,V] gradient tensor exists."""

    def forward(self, seq_logprobs, seq_masks, reward):
        from .autograd import reward_criterion
        return reward_criterion(seq_logprobs, seq_masks, reward)


def _load_cider():
    global _cider
    if _cider is not None:
        return _cider
    if not os.path.exists(CIDER_LIB_PATH):
        raise RuntimeError('libinsenticap_cider.so not found at %s - run `python -m insenticap_model_amd._build`'
                           % CIDER_LIB_PATH)
    lib = C.CDLL(CIDER_LIB_PATH)
    i64p = C.POINTER(C.c_int64)
    lib.isc_cider_create.restype = C.c_void_p
    lib.isc_cider_create.argtypes = [i64p, i64p, i64p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_double]
    lib.isc_cider_destroy.restype = None
    lib.isc_cider_destroy.argtypes = [C.c_void_p]
    lib.isc_cider_num_images.restype = C.c_int64
    lib.isc_cider_num_images.argtypes = [C.c_void_p]
    lib.isc_cider_num_ngrams.restype = C.c_int64
    lib.isc_cider_num_ngrams.argtypes = [C.c_void_p]
    lib.isc_cider_score.restype = C.c_int
    lib.isc_cider_score.argtypes = [C.c_void_p, i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i64p, i64p,
                                    C.POINTER(C.c_double), C.c_int]
    # what the device scorer reads (DeviceCiderD)
    lib.isc_cider_params.restype = C.c_int
    lib.isc_cider_params.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double)]
    lib.isc_cider_table_capacity.restype = C.c_int64
    lib.isc_cider_table_capacity.argtypes = [C.c_void_p]
    lib.isc_cider_table_fill.restype = C.c_int
    lib.isc_cider_table_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.isc_cider_cook_size.restype = C.c_int64
    lib.isc_cider_cook_size.argtypes = [C.c_void_p, i64p, i64p, C.c_int64]
    lib.isc_cider_cook_fill.restype = C.c_int64
    lib.isc_cider_cook_fill.argtypes = [C.c_void_p, i64p, i64p, C.c_int64] + [C.c_void_p] * 5
    i32p = C.POINTER(C.c_int32)
    lib.isc_bleu_score.restype = C.c_int
    lib.isc_bleu_score.argtypes = [i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i64p, i64p, C.c_int64, C.c_int64,
                                   C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_double), i32p]
    lib.isc_bleu_cook_size.restype = C.c_int64
    lib.isc_bleu_cook_size.argtypes = [i64p, i64p, C.c_int64, C.c_int64, C.c_int64]
    lib.isc_bleu_cook_fill.restype = C.c_int64
    lib.isc_bleu_cook_fill.argtypes = [i64p, i64p, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 4
    _cider = lib
    return lib


def _flatten(caption_lists):
    """[[caps of image 0], [caps of image 1], ...] -> (tokens, cap_off, img_off) int64 arrays."""
    toks, cap_off, img_off = [], [0], [0]
    for caps in caption_lists:
        for cap in caps:
            toks.extend(int(x) for x in cap)
            cap_off.append(len(toks))
        img_off.append(len(cap_off) - 1)
    return (np.asarray(toks, dtype=np.int64), np.asarray(cap_off, dtype=np.int64),
            np.asarray(img_off, dtype=np.int64))


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _default_threads():
    """Up to 16 scoring threads, of this process's share of the host's cores (one process per GPU: LOCAL_WORLD_SIZE ranks of
    a launcher share them - eight ranks x 16 threads on a 64-core host would only queue behind each other)."""
    cores = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        local_ranks = max(1, int(os.environ.get('LOCAL_WORLD_SIZE', '1')))
    except ValueError:
        local_ranks = 1
    return max(1, min(16, cores // local_ranks))


def _flatten_cached(cache, ref_caption_lists, keys):
    """_flatten with the per-image conversion kept in `cache` under the image ids `keys`."""
    toks, lens, counts = [], [], []
    for k, caps in zip(keys, ref_caption_lists):
        c = cache.get(k)
        if c is None:
            c = (np.asarray([int(x) for cap in caps for x in cap], dtype=np.int64),
                 np.asarray([len(cap) for cap in caps], dtype=np.int64))
            cache[k] = c
        toks.append(c[0])
        lens.append(c[1])
        counts.append(len(c[1]))
    cap_off = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.int64)
    img_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return np.concatenate(toks), cap_off, img_off


class CiderD:
    """Native CIDEr-D scorer; plays the role of the reference's `CiderD(refs=...)` object
    (ciderD.py:16-48) for `get_self_critical_reward`."""

    def __init__(self, ref_caption_lists, sos_token, eos_token, n=4, sigma=6.0, n_threads=None):
        lib = _load_cider()
        toks, cap_off, img_off = _flatten(ref_caption_lists)
        self._lib = lib
        self.sos, self.eos = int(sos_token), int(eos_token)
        self._h = lib.isc_cider_create(_p(toks), _p(cap_off), _p(img_off), len(img_off) - 1, self.sos, self.eos,
                                       n, sigma)
        if not self._h:
            raise RuntimeError('isc_cider_create failed')
        self.n_threads = n_threads or _default_threads()
        self._gt_cache = {}

    def __del__(self):
        if getattr(self, '_h', None):
            self._lib.isc_cider_destroy(self._h)
            self._h = None

    @property
    def num_images(self):
        return self._lib.isc_cider_num_images(self._h)

    @property
    def num_ngrams(self):
        return self._lib.isc_cider_num_ngrams(self._h)

    def flatten_refs(self, ref_caption_lists, keys=None):
        """Flattened (tokens, cap_off, img_off) of a batch of reference lists; with `keys` (image ids)
        the per-image conversion is cached across calls (the ground truth of an image never changes)."""
        if keys is None:
            return _flatten(ref_caption_lists)
        return _flatten_cached(self._gt_cache, ref_caption_lists, keys)

    def score_arrays(self, hyps, ref_caption_lists, flat=None):
        """hyps: int64 [N,T] raw roll-out rows; ref_caption_lists[i]: list of id lists (or `flat` = a
        flatten_refs() result). -> float64 [N]."""
        hyps = np.ascontiguousarray(hyps, dtype=np.int64)
        toks, cap_off, img_off = flat if flat is not None else _flatten(ref_caption_lists)
        out = np.empty(hyps.shape[0], dtype=np.float64)
        rc = self._lib.isc_cider_score(self._h, _p(hyps), hyps.shape[0], hyps.shape[1], hyps.shape[1], _p(toks),
                                       _p(cap_off), _p(img_off), out.ctypes.data_as(C.POINTER(C.c_double)),
                                       self.n_threads)
        if rc != 0:
            raise RuntimeError('isc_cider_score failed (%d)' % rc)
        return out

    # ---- what the device scorer reads (DeviceCiderD; csrc/cider_key.h defines the key, the hash and the slot)
    def device_params(self):
        """(ref_len = log(#images), n, sigma) of the scorer."""
        ref_len, n, sigma = C.c_double(), C.c_int(), C.c_double()
        if self._lib.isc_cider_params(self._h, C.byref(ref_len), C.byref(n), C.byref(sigma)) != 0:
            raise RuntimeError('isc_cider_params failed')
        return ref_len.value, n.value, sigma.value

    def device_table(self, capacity=None):
        """The document frequencies as an open-addressing array (linear probing) of CIDER_SLOT records: key, log(max(1,
        df)); key 0 = empty.  `capacity`: a power of two above num_ngrams, default the production size (>= 2 x num_ngrams).
        ValueError when an n-gram holds an id above 65534 (a key field is 16 bits)."""
        cap = int(capacity) if capacity is not None else self._lib.isc_cider_table_capacity(self._h)
        tab = np.empty(cap, dtype=CIDER_SLOT)
        rc = self._lib.isc_cider_table_fill(self._h, tab.ctypes.data, cap)
        if rc == -3:
            raise ValueError('the device CIDEr-D table needs every token id <= %d' % CIDER_MAX_ID)
        if rc != 0:
            raise RuntimeError('isc_cider_table_fill failed (%d)' % rc)
        return tab

    def cook_refs(self, captions):
        """The captions of ONE list cooked for the device: (keys uint64 [E], vals float64 [E], ord_off int32 [C, 5], norms
        float64 [C, 4], length float64 [C]) - per caption its distinct n-grams in the scorer's first-occurrence order, grouped
        by order, with counts2vec's tf-idf values, norms and length (the host scorer's own numbers, bit for bit)."""
        toks, cap_off, _ = _flatten([captions])
        n_caps = len(cap_off) - 1
        E = self._lib.isc_cider_cook_size(self._h, _p(toks), _p(cap_off), n_caps)
        if E == -3:
            raise ValueError('the device CIDEr-D scorer needs every token id <= %d' % CIDER_MAX_ID)
        if E < 0:
            raise RuntimeError('isc_cider_cook_size failed (%d)' % E)
        keys, vals = np.empty(E, dtype=np.uint64), np.empty(E, dtype=np.float64)
        ord_off = np.empty((n_caps, 5), dtype=np.int32)
        norms, length = np.empty((n_caps, 4), dtype=np.float64), np.empty(n_caps, dtype=np.float64)
        got = self._lib.isc_cider_cook_fill(self._h, _p(toks), _p(cap_off), n_caps, keys.ctypes.data, vals.ctypes.data,
                                            ord_off.ctypes.data, norms.ctypes.data, length.ctypes.data)
        if got != E:
            raise RuntimeError('isc_cider_cook_fill failed (%d)' % got)
        return keys, vals, ord_off, norms, length

    def to_device(self, device, vocab_size):
        """The device twin of this scorer (DeviceCiderD): the table is uploaded once.  ValueError when vocab_size > 65535."""
        return DeviceCiderD(self, device, vocab_size)


CIDER_SLOT = np.dtype([('key', '<u8'), ('log_df', '<f8')])      # isc_cider_slot (csrc/cider_key.h): 16 bytes
CIDER_MAX_ID = 65534                                             # ISC_CIDER_MAX_ID: a key field holds id + 1 in 16 bits
CIDER_DEV_MAX_T = 63                                             # isc_cider_dev_score: one lane per word, L <= T + 1 <= 64


class CiderRefPack:
    """The cooked references of one batch on the device (DeviceCiderD.pack_refs): views into ONE uploaded buffer."""
    __slots__ = ('n_img', 'buffer', 'img_cap_off', 'ord_off', 'norms', 'length', 'keys', 'vals')


class DeviceCiderD:
    """CIDEr-D on the device (isc_cider_dev_score): the twin of a host `CiderD`, whose table and cooked references it reads.
    One wave per hypothesis, the host scorer's order of sums: scores agree with CiderD.score_arrays to the last bits of
    exp / sqrt / division (tests: 1e-12)."""

    def __init__(self, host, device, vocab_size):
        if int(vocab_size) > CIDER_MAX_ID + 1:
            raise ValueError('the device CIDEr-D scorer packs an id into 16 bits: vocab_size <= %d, got %d'
                             % (CIDER_MAX_ID + 1, vocab_size))
        self.host, self.device = host, torch.device(device)
        self.ref_len, self.n, self.sigma = host.device_params()
        tab = host.device_table()
        self.table = torch.from_numpy(tab.view(np.int64).reshape(-1, 2)).to(self.device)      # [capacity, 2], once
        self._cache = {}

    def pack_refs(self, ref_caption_lists, keys=None):
        """The batch's references cooked (per image, cached by `keys` - image ids - as CiderD.flatten_refs caches),
        concatenated and uploaded as one buffer through pinned memory, non-blocking.  Depends on no device result: it can be
        issued while a roll-out is still running.  An image without references raises, as the host scorer does."""
        cooked = []
        for i, caps in enumerate(ref_caption_lists):
            k = None if keys is None else keys[i]
            c = None if k is None else self._cache.get(k)
            if c is None:
                if len(caps) == 0:
                    raise RuntimeError('CIDEr-D: image %d of the batch has no reference caption' % i)
                c = self.host.cook_refs(caps)
                if k is not None:
                    self._cache[k] = c
            cooked.append(c)
        n_img = len(cooked)
        caps_per = np.asarray([len(c[4]) for c in cooked], dtype=np.int64)
        ents_per = np.asarray([len(c[0]) for c in cooked], dtype=np.int64)
        n_cap, n_ent = int(caps_per.sum()), int(ents_per.sum())
        if n_ent > 0x7fffffff:
            raise RuntimeError('CIDEr-D: more than 2^31 - 1 reference n-grams in one batch')
        ent_base = np.concatenate([[0], np.cumsum(ents_per)[:-1]])
        # one pinned buffer, every region 8-byte aligned: keys, vals, norms, length | ord_off, img_cap_off (int32)
        sizes = [8 * n_ent, 8 * n_ent, 32 * n_cap, 8 * n_cap, (20 * n_cap + 7) // 8 * 8, (4 * (n_img + 1) + 7) // 8 * 8]
        offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        host = torch.empty(offs[-1], dtype=torch.uint8)
        if self.device.type == 'cuda':
            host = host.pin_memory()
        raw = host.numpy()

        def region(j, dtype, count):
            return raw[offs[j]:offs[j] + count * np.dtype(dtype).itemsize].view(dtype)
        np.concatenate([c[0] for c in cooked], out=region(0, np.uint64, n_ent))
        np.concatenate([c[1] for c in cooked], out=region(1, np.float64, n_ent))
        np.concatenate([c[3] for c in cooked], out=region(2, np.float64, 4 * n_cap).reshape(n_cap, 4))
        np.concatenate([c[4] for c in cooked], out=region(3, np.float64, n_cap))
        ord_off = region(4, np.int32, 5 * n_cap).reshape(n_cap, 5)
        np.concatenate([c[2] for c in cooked], out=ord_off)
        ord_off += np.repeat(ent_base, caps_per).astype(np.int32)[:, None]
        img_cap = region(5, np.int32, n_img + 1)
        img_cap[0] = 0
        np.cumsum(caps_per, out=img_cap[1:])
        dev = host.to(self.device, non_blocking=True)

        def view(j, dtype, count, size):
            return dev[offs[j]:offs[j] + count * size].view(dtype)
        p = CiderRefPack()
        p.n_img, p.buffer = n_img, dev
        p.keys, p.vals = view(0, torch.int64, n_ent, 8), view(1, torch.float64, n_ent, 8)
        p.norms, p.length = view(2, torch.float64, 4 * n_cap, 8).view(n_cap, 4), view(3, torch.float64, n_cap, 8)
        p.ord_off = view(4, torch.int32, 5 * n_cap, 4).view(n_cap, 5)
        p.img_cap_off = view(5, torch.int32, n_img + 1, 4)
        return p

    def score(self, hyps, pack, row_div=1, out=None):
        """hyps: int64 [N, T] raw roll-out rows on the device, row r of image r // row_div of `pack` -> float64 [N] on the
        device.  T > 63 raises (the caller keeps the host scorer for such rows)."""
        from . import ops
        if hyps.shape[0] != pack.n_img * int(row_div):
            raise ValueError('CIDEr-D: %d rows for %d images x %d rows per image' % (hyps.shape[0], pack.n_img, row_div))
        hyps = hyps if hyps.is_contiguous() else hyps.contiguous()
        return ops.cider_dev_score(hyps, row_div, self.table, pack.img_cap_off, pack.ord_off, pack.norms, pack.length,
                                   pack.keys, pack.vals, self.n, self.sigma, self.ref_len, self.host.sos, self.host.eos,
                                   out=out)


def _bleu_corpus(stats, n=4):
    """The corpus figures of bleu_scorer.py:247-259 from the summed integer statistics, in Python floats."""
    small, tiny = 1e-9, 1e-15
    tot = [int(x) for x in np.asarray(stats, dtype=np.int64).reshape(-1, 10).sum(axis=0)]
    testlen, reflen, guess, correct = tot[0], tot[1], tot[2:6], tot[6:10]
    bleus, bleu = [], 1.
    for k in range(n):
        bleu *= float(correct[k] + tiny) / (guess[k] + small)
        bleus.append(bleu ** (1. / (k + 1)))
    ratio = (testlen + tiny) / (reflen + small)
    if ratio < 1:
        for k in range(n):
            bleus[k] *= math.exp(1 - 1 / ratio)
    return bleus


class Bleu:
    """Native BLEU scorer; plays the role of the reference's `Bleu(n)` object (self_critical/bleu/bleu.py) for
    `get_self_critical_reward`, whose reward is the per-sentence BLEU-4 list (utils.py:75-77) - here BLEU-`order`.  It
    keeps no document frequencies, hence takes no corpus.  Rows and references are normalised as the CIDEr-D scorer
    normalises them (utils._array_to_str)."""

    def __init__(self, sos_token, eos_token, n=4, order=4, n_threads=None):
        if not 1 <= int(n) <= 4 or not 1 <= int(order) <= int(n):
            raise ValueError('BLEU: 1 <= order <= n <= 4, got n = %r, order = %r' % (n, order))
        self._lib = _load_cider()
        self.sos, self.eos = int(sos_token), int(eos_token)
        self.n, self.order = int(n), int(order)
        self.n_threads = n_threads or _default_threads()
        self._gt_cache = {}

    def flatten_refs(self, ref_caption_lists, keys=None):
        """As CiderD.flatten_refs: with `keys` (image ids) the per-image conversion is cached across calls."""
        if keys is None:
            return _flatten(ref_caption_lists)
        return _flatten_cached(self._gt_cache, ref_caption_lists, keys)

    def _score(self, hyps, ref_caption_lists, flat, row_div, want_stats):
        hyps = np.ascontiguousarray(hyps, dtype=np.int64)
        toks, cap_off, img_off = flat if flat is not None else _flatten(ref_caption_lists)
        N = hyps.shape[0]
        out = np.empty((N, 4), dtype=np.float64)
        stats = np.empty((N, 10), dtype=np.int32) if want_stats else None
        rc = self._lib.isc_bleu_score(_p(hyps), N, hyps.shape[1], hyps.shape[1], _p(toks), _p(cap_off), _p(img_off),
                                      len(img_off) - 1, int(row_div), self.sos, self.eos, self.n_threads,
                                      out.ctypes.data_as(C.POINTER(C.c_double)),
                                      stats.ctypes.data_as(C.POINTER(C.c_int32)) if want_stats else None)
        if rc != 0:
            raise RuntimeError('isc_bleu_score failed (%d)' % rc)
        return out, stats

    def score4(self, hyps, ref_caption_lists, flat=None, row_div=1):
        """hyps: int64 [N,T] raw roll-out rows, row r against ref_caption_lists[r // row_div] (or `flat` = a flatten_refs()
        result) -> float64 [N,4]: the per-sentence BLEU-1 .. BLEU-4."""
        return self._score(hyps, ref_caption_lists, flat, row_div, False)[0]

    def score_arrays(self, hyps, ref_caption_lists, flat=None, row_div=1):
        """-> float64 [N]: BLEU-`order` (order 4 = the reference's reward, scores[3])."""
        return np.ascontiguousarray(self.score4(hyps, ref_caption_lists, flat, row_div)[:, self.order - 1])

    def stats(self, hyps, ref_caption_lists, flat=None, row_div=1):
        """-> int32 [N,10]: testlen, reflen, guess[0..3], correct[0..3] (bleu_scorer.py:63-86, option 'closest')."""
        return self._score(hyps, ref_caption_lists, flat, row_div, True)[1]

    def compute_score(self, gts, res):
        """The reference wrapper's call (bleu.py:24-59): gts = {image_id: [reference strings]}, res = [{'image_id': id,
        'caption': [string]}] -> (corpus BLEU-1..n, n per-sentence lists).  The strings are what utils._array_to_str
        writes - ids joined by blanks, <EOS> last and nowhere else, no leading <SOS>; anything else raises ValueError."""
        def ids(text):
            try:
                w = [int(x) for x in text.split()]
            except ValueError:
                w = None
            if not w or w[-1] != self.eos or self.eos in w[:-1] or w[0] == self.sos:
                raise ValueError('BLEU: %r is no normalised caption (ids, <EOS> = %d last)' % (text, self.eos))
            return w
        rows, refs = [], []
        for item in res:
            hypo, ref = item['caption'], gts[item['image_id']]
            assert type(hypo) is list and len(hypo) == 1 and type(ref) is list and len(ref) >= 1
            rows.append(ids(hypo[0]))
            refs.append([ids(r) for r in ref])
        hyps = np.full((len(rows), max(len(w) for w in rows)), self.eos, dtype=np.int64)
        for i, w in enumerate(rows):
            hyps[i, :len(w)] = w
        scores, stats = self._score(hyps, refs, None, 1, True)
        return _bleu_corpus(stats, self.n), [scores[:, k].tolist() for k in range(self.n)]

    def method(self):
        return 'Bleu'

    def cook_refs(self, captions):
        """The references of ONE image cooked for the device: (keys uint64 [E], counts int32 [E], ent_off int32 [5], lens
        int32 [C]) - the distinct n-grams over all captions with their largest count in one caption, grouped by order
        (within an order: captions ascending, first occurrence within a caption), and the normalised lengths."""
        toks, cap_off, _ = _flatten([captions])
        n_caps = len(cap_off) - 1
        E = self._lib.isc_bleu_cook_size(_p(toks), _p(cap_off), n_caps, self.sos, self.eos)
        if E == -3:
            raise ValueError('the device BLEU scorer needs every token id <= %d' % CIDER_MAX_ID)
        if E < 0:
            raise RuntimeError('isc_bleu_cook_size failed (%d)' % E)
        keys, counts = np.empty(E, dtype=np.uint64), np.empty(E, dtype=np.int32)
        ent_off, lens = np.empty(5, dtype=np.int32), np.empty(n_caps, dtype=np.int32)
        got = self._lib.isc_bleu_cook_fill(_p(toks), _p(cap_off), n_caps, self.sos, self.eos, keys.ctypes.data,
                                           counts.ctypes.data, ent_off.ctypes.data, lens.ctypes.data)
        if got != E:
            raise RuntimeError('isc_bleu_cook_fill failed (%d)' % got)
        return keys, counts, ent_off, lens

    def to_device(self, device, vocab_size):
        """The device twin of this scorer (DeviceBleu).  ValueError when vocab_size > 65535."""
        return DeviceBleu(self, device, vocab_size)


class BleuRefPack:
    """The cooked references of one batch on the device (DeviceBleu.pack_refs): views into ONE uploaded buffer."""
    __slots__ = ('n_img', 'buffer', 'keys', 'counts', 'ent_off', 'img_cap_off', 'lens')


class DeviceBleu:
    """BLEU on the device (isc_bleu_dev_score): the twin of a host `Bleu`, whose cooked references it reads.  One wave per
    hypothesis; the integer statistics are the host's exactly, the scores agree to the last bits of pow / exp / division
    (tests: 1e-12 relative)."""

    def __init__(self, host, device, vocab_size):
        if int(vocab_size) > CIDER_MAX_ID + 1:
            raise ValueError('the device BLEU scorer packs an id into 16 bits: vocab_size <= %d, got %d'
                             % (CIDER_MAX_ID + 1, vocab_size))
        self.host, self.device = host, torch.device(device)
        self._cache = {}

    def pack_refs(self, ref_caption_lists, keys=None):
        """The batch's references cooked (per image, cached by `keys` - image ids), concatenated and uploaded as one buffer
        through pinned memory, non-blocking, as DeviceCiderD.pack_refs does.  An image without references raises."""
        cooked = []
        for i, caps in enumerate(ref_caption_lists):
            k = None if keys is None else keys[i]
            c = None if k is None else self._cache.get(k)
            if c is None:
                if len(caps) == 0:
                    raise RuntimeError('BLEU: image %d of the batch has no reference caption' % i)
                c = self.host.cook_refs(caps)
                if k is not None:
                    self._cache[k] = c
            cooked.append(c)
        n_img = len(cooked)
        ents_per = np.asarray([len(c[0]) for c in cooked], dtype=np.int64)
        caps_per = np.asarray([len(c[3]) for c in cooked], dtype=np.int64)
        n_ent, n_cap = int(ents_per.sum()), int(caps_per.sum())
        if n_ent > 0x7fffffff:
            raise RuntimeError('BLEU: more than 2^31 - 1 reference n-grams in one batch')
        ent_base = np.concatenate([[0], np.cumsum(ents_per)[:-1]])
        # one pinned buffer, every region 8-byte aligned: keys | counts, ent_off, img_cap_off, lens (int32)

        def pad8(b):
            return (b + 7) // 8 * 8
        sizes = [8 * n_ent, pad8(4 * n_ent), pad8(20 * n_img), pad8(4 * (n_img + 1)), pad8(4 * n_cap)]
        offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        host = torch.empty(offs[-1], dtype=torch.uint8)
        if self.device.type == 'cuda':
            host = host.pin_memory()
        raw = host.numpy()

        def region(j, dtype, count):
            return raw[offs[j]:offs[j] + count * np.dtype(dtype).itemsize].view(dtype)
        np.concatenate([c[0] for c in cooked], out=region(0, np.uint64, n_ent))
        np.concatenate([c[1] for c in cooked], out=region(1, np.int32, n_ent))
        ent_off = region(2, np.int32, 5 * n_img).reshape(n_img, 5)
        np.stack([c[2] for c in cooked], out=ent_off)
        ent_off += ent_base.astype(np.int32)[:, None]
        img_cap = region(3, np.int32, n_img + 1)
        img_cap[0] = 0
        np.cumsum(caps_per, out=img_cap[1:])
        np.concatenate([c[3] for c in cooked], out=region(4, np.int32, n_cap))
        dev = host.to(self.device, non_blocking=True)

        def view(j, dtype, count, size):
            return dev[offs[j]:offs[j] + count * size].view(dtype)
        p = BleuRefPack()
        p.n_img, p.buffer = n_img, dev
        p.keys, p.counts = view(0, torch.int64, n_ent, 8), view(1, torch.int32, n_ent, 4)
        p.ent_off = view(2, torch.int32, 5 * n_img, 4).view(n_img, 5)
        p.img_cap_off, p.lens = view(3, torch.int32, n_img + 1, 4), view(4, torch.int32, n_cap, 4)
        return p

    def _launch(self, hyps, pack, row_div, order, out, stats=None):
        from . import ops
        if hyps.shape[0] != pack.n_img * int(row_div):
            raise ValueError('BLEU: %d rows for %d images x %d rows per image' % (hyps.shape[0], pack.n_img, row_div))
        hyps = hyps if hyps.is_contiguous() else hyps.contiguous()
        return ops.bleu_dev_score(hyps, row_div, pack.ent_off, pack.keys, pack.counts, pack.img_cap_off, pack.lens, order,
                                  self.host.sos, self.host.eos, out=out, stats=stats)

    def score(self, hyps, pack, row_div=1, out=None):
        """hyps: int64 [N, T] raw roll-out rows on the device, row r of image r // row_div of `pack` -> float64 [N] on the
        device: BLEU-`order` of the host scorer.  T > 63 raises (the caller keeps the host scorer for such rows)."""
        return self._launch(hyps, pack, row_div, self.host.order, out)

    def score4(self, hyps, pack, row_div=1, out=None, stats=None):
        """-> float64 [N, 4] on the device; `stats`: an int32 [N, 10] tensor to fill with the integer statistics."""
        return self._launch(hyps, pack, row_div, 0, out, stats)


def get_bleu_scorer(sos_token, eos_token, order=4):
    """The BLEU twin of get_ciderd_scorer: the reference builds `Bleu()` and reads scores[3] (utils.py:75-77)."""
    return Bleu(sos_token, eos_token, order=order)


def get_ciderd_scorer(split_captions, sos_token, eos_token):
    """utils.py:38-53: `split_captions` = {split: {fn: [[ids], ...]}}; document frequencies over all images."""
    captions = {}
    for caps in split_captions.values():
        captions.update(caps)
    return CiderD(list(captions.values()), sos_token, eos_token)


def self_critical_scores(captions, fns, ground_truth, scorer):
    """CIDEr-D (with a `Bleu`: BLEU-`order`) of one token matrix [B,T] (host ndarray) against the images' references ->
    float64 [B]: one half of get_self_critical_reward, for callers that score the sampled captions while the device still
    decodes the greedy ones."""
    if not isinstance(scorer, (CiderD, Bleu)):
        raise Exception('do not support this scorer: %s' % type(scorer))
    assert captions.shape[0] == len(fns)
    flat = scorer.flatten_refs([ground_truth[fn] for fn in fns], keys=list(fns))
    return scorer.score_arrays(captions, None, flat)


def get_self_critical_reward(sample_captions, greedy_captions, fns, ground_truth, sos_token, eos_token, scorer):
    """utils.py:56-83: CIDEr-D(sample) - CIDEr-D(greedy), repeated over T -> float64 ndarray [B,T]; with a `Bleu` the
    scores are its per-sentence BLEU-`order` (utils.py:75-77)."""
    batch_size = len(fns)
    if torch.is_tensor(sample_captions):
        sample_captions = sample_captions.cpu().numpy()
    if torch.is_tensor(greedy_captions):
        greedy_captions = greedy_captions.cpu().numpy()
    assert sample_captions.shape[0] == greedy_captions.shape[0] == batch_size
    if not isinstance(scorer, (CiderD, Bleu)):
        raise Exception('do not support this scorer: %s' % type(scorer))
    flat = scorer.flatten_refs([ground_truth[fn] for fn in fns], keys=list(fns))
    scores = scorer.score_arrays(sample_captions, None, flat) - scorer.score_arrays(greedy_captions, None, flat)
    return np.repeat(scores[:, np.newaxis], sample_captions.shape[1], 1)


def get_self_critical_reward_device(sample_captions, greedy_captions, pack, dev_scorer):
    """get_self_critical_reward on the device: token matrices [B, T] on the device, `pack` = dev_scorer.pack_refs(...) of
    the batch -> float32 [B, T] on the device: (CIDEr-D(sample) - CIDEr-D(greedy)) in fp64, rounded to float32, repeated
    over T - the host form followed by `.astype('float32')`."""
    if not isinstance(dev_scorer, (DeviceCiderD, DeviceBleu)):
        raise Exception('do not support this scorer: %s' % type(dev_scorer))
    assert sample_captions.shape == greedy_captions.shape
    scores = dev_scorer.score(sample_captions, pack) - dev_scorer.score(greedy_captions, pack)
    return scores.to(torch.float32).unsqueeze(1).repeat(1, sample_captions.shape[1])


def _check_group(n, rows, images=None):
    if isinstance(n, bool) or not hasattr(n, '__index__') or int(n) < 2:
        raise ValueError('a group reward needs n >= 2 samples per image (an integer), got %r' % (n,))
    n = int(n)
    if images is None:
        if rows % n:
            raise ValueError('n=%d: %d rows are no whole number of images' % (n, rows))
    elif rows != images * n:
        raise ValueError('n=%d: %d images need %d sampled rows (row i*n + j = sample j of image i), got %d'
                         % (n, images, images * n, rows))
    return n


def group_self_critical_scores(sample_captions, fns, ground_truth, scorer, n):
    """CIDEr-D of n sampled captions per image: `fns` / `ground_truth` per image, `sample_captions` [I*n, T] (host ndarray
    or tensor), row i*n + j = sample j of image i.  Every row is scored against ITS image's references by the native
    scorer -> float64 [I*n]."""
    if torch.is_tensor(sample_captions):
        sample_captions = sample_captions.cpu().numpy()
    n = _check_group(n, sample_captions.shape[0], len(fns))
    return self_critical_scores(sample_captions, [fn for fn in fns for _ in range(n)], ground_truth, scorer)


def group_advantages(scores, n):
    """Self-critical advantages with the image's other samples as the baseline, float64 [I*n] -> float64 [I*n]:
    adv[i,j] = scores[i,j] - (sum over k != j, k ascending, of scores[i,k]) / (n - 1).  The additions run in that order
    (isc_group_reward forms the same bits on the device)."""
    scores = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
    n = _check_group(n, scores.shape[0])
    s = scores.reshape(-1, n)
    adv = np.empty_like(s)
    for j in range(n):
        acc = np.zeros(s.shape[0], dtype=np.float64)
        for k in range(n):
            if k != j:
                acc = acc + s[:, k]
        adv[:, j] = s[:, j] - acc / np.float64(n - 1)
    return adv.reshape(-1)


def get_group_self_critical_reward(sample_captions, fns, ground_truth, scorer, n):
    """The fact reward of the grouped RL iteration: CIDEr-D(sample) minus the mean CIDEr-D of the image's other n - 1
    samples, repeated over T unmasked as utils.py:83 repeats the score -> float64 ndarray [I*n, T].  This is the host
    form (and the reference) of what isc_group_reward builds on the device from the uploaded scores."""
    scores = group_self_critical_scores(sample_captions, fns, ground_truth, scorer, n)
    T = sample_captions.shape[1]
    return np.repeat(group_advantages(scores, n)[:, np.newaxis], T, 1)


def get_cls_reward(sample_captions, sample_masks, greedy_captions, greedy_masks, senti_labels, sent_senti_cls,
                   sample_lens=None, on_device=False):
    """utils.py:120-151: 1[classifier(sample) == label] x per-token squeeze-excite weights, zero-padded
    to T. `sent_senti_cls` is the frozen helper net (helper_nets.SentenceSentimentClassifier).
    `sample_lens` (host ints) skips the device->host read of the mask sums - or a device tensor [B]: the classifier then
    runs over all T columns and needs no host value at all (the launches can be enqueued before the roll-out has
    finished); `on_device=True` returns the [B,T] float tensor without a host round trip (the trainer adds it to the
    CIDEr reward on the device)."""
    training = sent_senti_cls.training
    if sample_lens is None:
        sample_lens = list(sample_masks.sum(dim=-1).type(torch.int).cpu().numpy())
    sent_senti_cls.eval()
    max_len = sample_captions.shape[1]
    with torch.no_grad():
        native = getattr(sent_senti_cls, 'native', False) and sent_senti_cls.native_active(sample_captions)
        if native:      # the native forward's head kernel writes 1[pred == label] x weights itself, zero-padded to T
            sample_scores = sent_senti_cls.forward_native(sample_captions, sample_lens, labels=senti_labels,
                                                          pad_to=max_len)[3]
    if native:
        sent_senti_cls.train(training)
        return sample_scores if on_device else sample_scores.cpu().numpy()
    with torch.no_grad():
        sample_preds, sample_att_weights = sent_senti_cls(sample_captions, sample_lens)
        sample_preds = sample_preds.softmax(dim=-1).argmax(dim=-1)
        sample_preds = (sample_preds == senti_labels).type_as(sample_att_weights).unsqueeze(1)
        sample_scores = (sample_preds * sample_att_weights).detach()
    sent_senti_cls.train(training)
    if on_device:
        return torch.nn.functional.pad(sample_scores, (0, max_len - sample_scores.shape[1]))
    sample_scores = sample_scores.cpu().numpy()
    return np.pad(sample_scores, ((0, 0), (0, max_len - sample_scores.shape[1])))


# ------------------------------------------------------------------------------------------------ n-gram language models
# The per-sentiment ARPA models of the reference (preprocess.py:426-466): its `ppl` metric (eval_ppl.py) and its LM reward
# (self_critical/utils.py:86-100).  DESIGN.md "Per-sentiment n-gram language models" holds the definition; the slot, the
# special ids and the probe are csrc/lm_slot.h; host scorer isc_lm_score (csrc/lm.cpp), device isc_lm_dev_score.
LM_SLOT = np.dtype([('key', '<u8'), ('logp', '<f4'), ('backoff', '<f4')])      # isc_lm_slot: 16 bytes
LM_MAX_VOCAB = CIDER_MAX_ID - 3          # <s>, </s>, <unk> = V, V + 1, V + 2 and "no word" = V + 3 must fit a key field
LM_MAX_ORDER = 4
LM_DEV_MAX_T = 62                        # isc_lm_dev_score: T + 2 scored positions in 64 lanes
_LM_SPECIALS = ('<s>', '</s>', '<unk>')
_LM_LIB_TYPED = False


def _load_lm():
    global _LM_LIB_TYPED
    lib = _load_cider()
    if not _LM_LIB_TYPED:
        lib.isc_lm_table_capacity.restype = C.c_int64
        lib.isc_lm_table_capacity.argtypes = [C.c_int64]
        lib.isc_lm_table_fill.restype = C.c_int
        lib.isc_lm_table_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        lib.isc_lm_score.restype = C.c_int
        lib.isc_lm_score.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        _LM_LIB_TYPED = True
    return lib


def _check_lm_vocab(vocab_size):
    V = int(vocab_size)
    if not 1 <= V <= LM_MAX_VOCAB:
        raise ValueError('an n-gram language model packs an id into 16 bits and adds four ids of its own: 1 <= vocab_size '
                         '<= %d, got %d' % (LM_MAX_VOCAB, V))
    return V


def read_arpa(path_or_text, vocab_size, word2idx=None):
    """An ARPA file (a path, or its text: anything holding a newline) of order <= 4 -> {'order', 'ids': [int64 [n_k, k]
    per order k], 'logp': [float32 [n_k]], 'backoff': [float32 [n_k]], 'dropped': n}.  Every decimal is read as a Python
    float and rounded once to float32; a missing back-off weight is +0.0.  Words map through `word2idx` when given (the
    word-level *_w.sri files), else as decimal ids (the *_id.kenlm.arpa files); <s>, </s>, <unk> take the ids V, V + 1,
    V + 2.  An n-gram holding a word outside the vocabulary is dropped and counted.  ValueError: vocab_size > 65531, an
    order above 4, a malformed line."""
    V = _check_lm_vocab(vocab_size)
    if '\n' in path_or_text:
        text = path_or_text
    else:
        with open(path_or_text) as f:
            text = f.read()
    special = {w: V + j for j, w in enumerate(_LM_SPECIALS)}
    ids, logp, backoff, dropped, k = {}, {}, {}, 0, 0
    for no, line in enumerate(text.splitlines(), 1):
        line = line.strip()
        if not line or line == '\\data\\' or line.startswith('ngram '):
            continue
        if line == '\\end\\':
            break
        if line.startswith('\\'):
            if not line.endswith('-grams:') or not line[1:-7].isdigit():
                raise ValueError('ARPA line %d: %r' % (no, line))
            k = int(line[1:-7])
            if not 1 <= k <= LM_MAX_ORDER:
                raise ValueError('ARPA: order %d (an n-gram key has %d fields)' % (k, LM_MAX_ORDER))
            ids.setdefault(k, []), logp.setdefault(k, []), backoff.setdefault(k, [])
            continue
        parts = line.split()
        if k < 1 or len(parts) not in (k + 1, k + 2):
            raise ValueError('ARPA line %d: %r is no %d-gram entry' % (no, line, k))
        row = []
        for w in parts[1:k + 1]:
            i = special.get(w)
            if i is None:
                i = word2idx.get(w) if word2idx is not None else (int(w) if w.isdigit() else None)
                if i is not None and not 0 <= int(i) < V:
                    i = None
            if i is None:
                break
            row.append(int(i))
        if len(row) < k:
            dropped += 1
            continue
        ids[k].append(row)
        logp[k].append(float(parts[0]))
        backoff[k].append(float(parts[k + 1]) if len(parts) == k + 2 else 0.0)
    if not ids:
        raise ValueError('ARPA: no n-gram section')
    order = max(ids)
    with np.errstate(over='ignore'):
        return {'order': order, 'dropped': dropped,
                'ids': [np.asarray(ids.get(k, []), dtype=np.int64).reshape(-1, k) for k in range(1, order + 1)],
                'logp': [np.asarray(logp.get(k, []), dtype=np.float64).astype(np.float32) for k in range(1, order + 1)],
                'backoff': [np.asarray(backoff.get(k, []), dtype=np.float64).astype(np.float32)
                            for k in range(1, order + 1)]}


class NgramLM:
    """One back-off model: `order`, `vocab_size`, its n-grams as csrc/cider_key.h keys (`keys` uint64 [n], the oldest
    word in field 0) with `logp` / `backoff` float32 [n], `n_dropped` (n-grams of the file with a word outside the
    vocabulary) and `has_unk`."""

    def __init__(self, order, vocab_size, keys, logp, backoff, n_dropped=0):
        self.order, self.vocab_size = int(order), _check_lm_vocab(vocab_size)
        if not 1 <= self.order <= LM_MAX_ORDER:
            raise ValueError('n-gram language model: 1 <= order <= %d, got %d' % (LM_MAX_ORDER, self.order))
        self.keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self.logp = np.ascontiguousarray(logp, dtype=np.float32)
        self.backoff = np.ascontiguousarray(backoff, dtype=np.float32)
        assert self.keys.ndim == 1 and self.keys.shape == self.logp.shape == self.backoff.shape
        self.n_dropped = int(n_dropped)
        self.has_unk = bool((self.keys == np.uint64(self.vocab_size + 3)).any())      # the unigram key of <unk>: id + 1

    @classmethod
    def from_arpa(cls, path_or_text, vocab_size, word2idx=None):
        a = read_arpa(path_or_text, vocab_size, word2idx)
        keys = []
        for k, ids in enumerate(a['ids'], 1):
            key = np.zeros(len(ids), dtype=np.uint64)
            for j in range(k):
                key |= (ids[:, j] + 1).astype(np.uint64) << np.uint64(16 * j)
            keys.append(key)
        return cls(a['order'], vocab_size, np.concatenate(keys), np.concatenate(a['logp']), np.concatenate(a['backoff']),
                   a['dropped'])

    def __len__(self):
        return len(self.keys)

    def table(self, capacity=None):
        """The model as an open-addressing array of LM_SLOT records (isc_lm_table_fill).  `capacity`: a power of two above
        the number of n-grams, default the production size (>= 2 x).  ValueError: a bad capacity, a duplicate n-gram."""
        lib = _load_lm()
        cap = int(capacity) if capacity is not None else lib.isc_lm_table_capacity(len(self))
        tab = np.empty(max(cap, 0), dtype=LM_SLOT)
        rc = lib.isc_lm_table_fill(self.keys.ctypes.data, self.logp.ctypes.data, self.backoff.ctypes.data, len(self),
                                   tab.ctypes.data, cap)
        if rc == -2:
            raise ValueError('n-gram language model: capacity %d is no power of two above %d n-grams' % (cap, len(self)))
        if rc in (-3, -5):
            raise ValueError('n-gram language model: %s' % ('an empty n-gram' if rc == -3 else 'an n-gram occurs twice'))
        if rc != 0:
            raise RuntimeError('isc_lm_table_fill failed (%d)' % rc)
        return tab


def _eos_mode(mode):
    if mode not in ('word', 'end'):
        raise ValueError("eos_mode is 'word' (the <EOS> id is a word, then </s>: the id files) or 'end' (the <EOS> becomes "
                         "</s>: the word files), got %r" % (mode,))
    return 0 if mode == 'word' else 1


class NgramLMSet:
    """The models of all sentiment labels in ONE slot array: `lms_by_label` = {label: NgramLM} (labels 0 .. n - 1) or a
    list.  `eos_mode` / `unk_as_word`: see isc_lm_score; `sos` / `eos`: the caption ids <SOS> / <EOS> that `score`
    normalises rows with (they can also be given per call).  `capacities`: per label, a tighter table than the default."""

    def __init__(self, lms_by_label, vocab_size, eos_mode='word', unk_as_word=True, sos=None, eos=None, capacities=None,
                 n_threads=None):
        self.vocab_size = _check_lm_vocab(vocab_size)
        if isinstance(lms_by_label, dict):
            if sorted(lms_by_label) != list(range(len(lms_by_label))):
                raise ValueError('NgramLMSet: the labels must be 0 .. n - 1, got %r' % sorted(lms_by_label))
            lms = [lms_by_label[l] for l in range(len(lms_by_label))]
        else:
            lms = list(lms_by_label)
        if not lms or not all(isinstance(m, NgramLM) for m in lms):
            raise ValueError('NgramLMSet takes at least one NgramLM per label')
        if any(m.vocab_size != self.vocab_size for m in lms):
            raise ValueError('NgramLMSet: every model must be loaded with vocab_size = %d' % self.vocab_size)
        self.lms = lms
        self.eos_mode, self._eos_mode = eos_mode, _eos_mode(eos_mode)
        self.unk_as_word = bool(unk_as_word)
        self.sos, self.eos = sos, eos
        self.n_threads = n_threads or _default_threads()
        caps = capacities if capacities is not None else [None] * len(lms)
        caps = [caps[l] for l in range(len(lms))]
        tabs = [m.table(c) for m, c in zip(lms, caps)]
        self.slots = np.concatenate(tabs)
        self.lm_capacity = np.asarray([len(t) for t in tabs], dtype=np.int64)
        self.lm_off = np.concatenate([[0], np.cumsum(self.lm_capacity)[:-1]]).astype(np.int64)
        self.lm_order = np.asarray([m.order for m in lms], dtype=np.int32)

    def __len__(self):
        return len(self.lms)

    def _ids(self, sos, eos):
        sos = self.sos if sos is None else sos
        eos = self.eos if eos is None else eos
        if sos is None or eos is None:
            raise ValueError('NgramLMSet: the <SOS> / <EOS> ids are not set (constructor or call)')
        return int(sos), int(eos)

    def score(self, hyps, labels=None, sos=None, eos=None, tok_logp=False):
        """hyps int64 [N, T] raw rows (ndarray or tensor), labels [N] or None (model 0) -> (score float64 [N] (log10),
        n_scored int32 [N], n_oov int32 [N]) and, with tok_logp, the values per position float64 [N, T + 2].  The host
        scorer (isc_lm_score), up to 16 threads."""
        sos, eos = self._ids(sos, eos)
        if torch.is_tensor(hyps):
            hyps = hyps.cpu().numpy()
        if torch.is_tensor(labels):
            labels = labels.cpu().numpy()
        hyps = np.ascontiguousarray(hyps, dtype=np.int64)
        N, T = hyps.shape
        if labels is not None:
            labels = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
            if labels.shape[0] != N:
                raise ValueError('NgramLMSet.score: %d labels for %d rows' % (labels.shape[0], N))
        score = np.empty(N, dtype=np.float64)
        ns, no = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int32)
        tok = np.empty((N, T + 2), dtype=np.float64) if tok_logp else None
        if N:
            rc = _load_lm().isc_lm_score(hyps.ctypes.data, N, T, labels.ctypes.data if labels is not None else None,
                                         len(self.lms), self.slots.ctypes.data, len(self.slots), self.lm_off.ctypes.data,
                                         self.lm_capacity.ctypes.data, self.lm_order.ctypes.data, self.vocab_size,
                                         self._eos_mode, int(self.unk_as_word), sos, eos, score.ctypes.data,
                                         ns.ctypes.data, no.ctypes.data, tok.ctypes.data if tok_logp else None,
                                         self.n_threads)
            if rc != 0:
                raise RuntimeError('isc_lm_score failed (%d)' % rc)
        return (score, ns, no, tok) if tok_logp else (score, ns, no)

    def to_device(self, device):
        """The device twin (DeviceNgramLMSet): the slot array is uploaded once."""
        return DeviceNgramLMSet(self, device)


class DeviceNgramLMSet:
    """The models on the device (isc_lm_dev_score): the twin of a host `NgramLMSet`, whose slot array it holds.  One wave
    per row; the scores equal the host scorer's in bits."""

    def __init__(self, host, device):
        self.host, self.device = host, torch.device(device)
        self.slots = torch.from_numpy(host.slots.view(np.int64).reshape(-1, 2)).to(self.device)      # [slots, 2], once
        self.lm_off = torch.from_numpy(host.lm_off).to(self.device)
        self.lm_capacity = torch.from_numpy(host.lm_capacity).to(self.device)
        self.lm_order = torch.from_numpy(host.lm_order).to(self.device)

    def score(self, hyps, labels=None, out=None, tok_logp=None, n_scored=None, n_oov=None, sos=None, eos=None):
        """hyps int64 [N, T] on the device (T <= 62), labels int64 [N] on the device or None -> (score float64 [N],
        n_scored int32 [N], n_oov int32 [N]) on the device; `out` / `n_scored` / `n_oov`: tensors to fill; `tok_logp`: a
        float64 [N, T + 2] tensor to fill with the values per position.  One launch, nothing read back."""
        from . import ops
        sos, eos = self.host._ids(sos, eos)
        hyps = hyps if hyps.is_contiguous() else hyps.contiguous()
        if labels is not None:
            labels = labels if labels.is_contiguous() else labels.contiguous()
        return ops.lm_dev_score(hyps, labels, self.slots, self.lm_off, self.lm_capacity, self.lm_order,
                                self.host.vocab_size, self.host._eos_mode, self.host.unk_as_word, sos, eos, out=out,
                                n_scored=n_scored, n_oov=n_oov, tok_logp=tok_logp)


def _lm_form(form):
    if form not in ('sign', 'ppl_diff'):
        raise ValueError("the LM reward is 'sign' or 'ppl_diff', got %r" % (form,))
    return form


def get_lm_reward(sample_captions, greedy_captions, senti_labels, sos_token, eos_token, lms, form='sign'):
    """utils.py:86-100 with `lms` an NgramLMSet -> float64 ndarray [B, T].  'sign': the reference's active line,
    sign(score(greedy) - score(sample)); 'ppl_diff': its commented alternative, ppl(greedy) - ppl(sample) with the
    per-sentence ppl = 10 ** (-score / n_scored).  The value is repeated over the T columns."""
    _lm_form(form)
    if not isinstance(lms, NgramLMSet):
        raise Exception('do not support these language models: %s' % type(lms))
    if torch.is_tensor(sample_captions):
        sample_captions = sample_captions.cpu().numpy()
    if torch.is_tensor(greedy_captions):
        greedy_captions = greedy_captions.cpu().numpy()
    if torch.is_tensor(senti_labels):
        senti_labels = senti_labels.cpu().numpy()
    assert sample_captions.shape[0] == greedy_captions.shape[0] == len(senti_labels)
    s, s_n, _ = lms.score(sample_captions, senti_labels, sos_token, eos_token)
    g, g_n, _ = lms.score(greedy_captions, senti_labels, sos_token, eos_token)
    if form == 'sign':
        scores = np.sign(g - s)
    else:
        with np.errstate(divide='ignore', invalid='ignore'):
            scores = 10.0 ** (-g / g_n) - 10.0 ** (-s / s_n)
    return np.repeat(scores[:, np.newaxis], sample_captions.shape[1], 1)


def get_lm_reward_device(sample_captions, greedy_captions, senti_labels, dev_lms, form='sign'):
    """get_lm_reward on the device: token matrices [B, T] and labels [B] on the device -> float32 [B, T] on the device, the
    host form followed by `.astype('float32')`; no token is copied to the host."""
    _lm_form(form)
    if not isinstance(dev_lms, DeviceNgramLMSet):
        raise Exception('do not support these language models: %s' % type(dev_lms))
    assert sample_captions.shape == greedy_captions.shape
    s, s_n, _ = dev_lms.score(sample_captions, senti_labels)
    g, g_n, _ = dev_lms.score(greedy_captions, senti_labels)
    if form == 'sign':
        scores = torch.sign(g - s)
    else:
        scores = torch.pow(10.0, -g / g_n.to(torch.float64)) - torch.pow(10.0, -s / s_n.to(torch.float64))
    return scores.to(torch.float32).unsqueeze(1).repeat(1, sample_captions.shape[1])


def lm_perplexity(scores, n_scored, n_oov, labels, n_labels=None):
    """The corpus figures per label from the read-back rows, summed on the host in float64 in row order:
    {label: {'ppl': 10 ** (-sum score / sum n_scored), 'ppl1': the same without the sentence ends in the denominator
    (sum n_scored - sentences), 'logprob', 'sentences', 'words' (= sum n_scored - sentences), 'oovs'}} - SRILM's `ppl` and
    `ppl1`.  Rows of a label outside the set (n_scored -1) are left out.  A label without a scored position: ppl nan."""
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    n_scored, n_oov = np.asarray(n_scored).reshape(-1), np.asarray(n_oov).reshape(-1)
    labels = np.zeros(len(scores), dtype=np.int64) if labels is None else np.asarray(labels).reshape(-1)
    out = {}
    for lab in (range(int(n_labels)) if n_labels is not None else sorted(set(int(x) for x in labels))):
        total, count, sent, oov = 0.0, 0, 0, 0
        for r in np.nonzero(labels == lab)[0]:
            if n_scored[r] < 0:
                continue
            total += float(scores[r])
            count += int(n_scored[r])
            oov += int(n_oov[r])
            sent += 1
        out[lab] = {'ppl': 10.0 ** (-total / count) if count > 0 else float('nan'),
                    'ppl1': 10.0 ** (-total / (count - sent)) if count - sent > 0 else float('nan'),
                    'logprob': total, 'sentences': sent, 'words': count - sent, 'oovs': oov}
    return out


# ---- the sentiment-word reward (utils.py:154-166) ---------------------------------------------------------------------
def get_senti_words_reward(sample_captions, senti_labels, sentiment_words):
    """utils.py:154-166 as it stands: sample_captions int [B, T] (tensor or ndarray), senti_labels [B], sentiment_words
    {label id: {word id: weight}} -> (float64 ndarray [B, T], accur_w).  Position (i, j) is paid the weight of its word
    where the word is in the lexicon of row i's label - EVERY position, also those behind <EOS> and <PAD> ids the lexicon
    happens to hold: nothing is masked here (RewardCriterion masks).  accur_w: defaultdict(set) {label id: the words that
    were paid}.  A label without an entry raises KeyError, as the reference does."""
    from collections import defaultdict
    if torch.is_tensor(sample_captions):
        sample_captions = sample_captions.cpu().numpy()
    sample_captions = np.asarray(sample_captions)
    rewards = np.zeros(sample_captions.shape, dtype=float)
    accur_w = defaultdict(set)
    for i in range(sample_captions.shape[0]):
        senti_id = int(senti_labels[i])
        words = sentiment_words[senti_id]
        for j, w in enumerate(sample_captions[i]):
            if w in words:
                rewards[i, j] = words[w]
                accur_w[senti_id].add(w)
    return rewards, accur_w


class SentimentWordWeights:
    """The lexicon of the sentiment-word reward as a dense table: `weights` float64 [n_labels, V] and `state` uint8
    [n_labels, V] - 0 = not in the lexicon, 1 = in it, 2 = in it and used since the last decay.  Membership is the state,
    never "weight != 0": a weight may be 0.0 or negative.  On a device the reward and the decay are isc_sw_reward /
    isc_sw_decay; a table in host memory serves from_dict / to_dict and the host statement of the decay."""

    def __init__(self, weights, state):
        assert weights.dtype == torch.float64 and weights.dim() == 2 and state.dtype == torch.uint8
        assert state.shape == weights.shape and weights.device == state.device
        self.weights, self.state = weights.contiguous(), state.contiguous()

    n_labels = property(lambda self: self.weights.shape[0])
    vocab_size = property(lambda self: self.weights.shape[1])
    device = property(lambda self: self.weights.device)

    @classmethod
    def from_dict(cls, sentiment_words, vocab_size, n_labels, device=None):
        """{label id: {word id: weight}} -> the table.  A label of [0, n_labels) without an entry is an EMPTY lexicon here
        (the host function raises KeyError for it; the kernel pays such rows nothing); a label outside [0, n_labels) or a
        word id outside [0, vocab_size) raises ValueError."""
        V, n_labels = int(vocab_size), int(n_labels)
        if V < 1 or n_labels < 1:
            raise ValueError('SentimentWordWeights: vocab_size and n_labels must be >= 1')
        weights = np.zeros((n_labels, V), dtype=np.float64)
        state = np.zeros((n_labels, V), dtype=np.uint8)
        for lab, words in sentiment_words.items():
            if not 0 <= int(lab) < n_labels:
                raise ValueError('SentimentWordWeights: label %r is outside [0, %d)' % (lab, n_labels))
            for w, weight in words.items():
                if not 0 <= int(w) < V:
                    raise ValueError('SentimentWordWeights: word id %r of label %r is outside [0, %d)' % (w, lab, V))
                weights[int(lab), int(w)] = float(weight)
                state[int(lab), int(w)] = 1
        table = cls(torch.from_numpy(weights), torch.from_numpy(state))
        return table if device is None else table.to(device)

    def to(self, device):
        from . import ops
        device = torch.device(device)
        if device.type == 'cuda':                          # (through pinned memory: the host does not wait for the queue)
            return SentimentWordWeights(ops.upload(self.weights, torch.float64, device),
                                        ops.upload(self.state, torch.uint8, device))
        return SentimentWordWeights(self.weights.to(device), self.state.to(device))

    def to_dict(self):
        """{label id: {word id: Python float}} over every label of the table, the word ids ascending."""
        w, s = self.weights.cpu().numpy(), self.state.cpu().numpy()
        return {lab: {int(i): float(w[lab, i]) for i in np.nonzero(s[lab])[0]} for lab in range(self.n_labels)}

    def update_dict(self, sentiment_words):
        """Writes the table's weights into the entries `sentiment_words` already has, in place (one copy of `weights`)."""
        w = self.weights.cpu().numpy()
        for lab, words in sentiment_words.items():
            for k in words:
                words[k] = float(w[int(lab), int(k)])
        return sentiment_words

    def reward(self, tok, labels, flag=0.0, reward_io=None, accumulate=False, reward64=None, row_hits=None, mark=True):
        """isc_sw_reward on device rows tok int64 [N, T] / labels int64 [N] -> reward_io float32 [N, T] (allocated when
        None and not accumulating: the reward itself, (float)w).  See ops.sw_reward."""
        from . import ops
        if reward_io is None and not accumulate:
            reward_io = torch.empty(tok.shape, dtype=torch.float32, device=tok.device)
        ops.sw_reward(tok, labels, self.weights, self.state, flag, reward_io, accumulate, reward64, row_hits, mark)
        return reward_io

    def mark(self, accur_w):
        """The host statement of the marks: accur_w {label id: words} as get_senti_words_reward returns it."""
        if self.weights.is_cuda:
            raise ValueError('SentimentWordWeights.mark is the host statement; on the device isc_sw_reward marks')
        s = self.state.numpy()
        for lab, words in accur_w.items():
            for w in words:
                if s[int(lab), int(w)]:
                    s[int(lab), int(w)] = 2

    def decay(self, factor):
        """weights *= factor where state == 2 and those states back to 1: isc_sw_decay on the device, numpy in host memory
        (float64 either way: the bits of the reference's `w *= 0.9`)."""
        if self.weights.is_cuda:
            from . import ops
            ops.sw_decay(self.weights, self.state, factor)
            return self
        w, s = self.weights.numpy(), self.state.numpy()
        used = s == 2
        w[used] = w[used] * float(factor)
        s[used] = 1
        return self


def senti_word_stats(captions, labels, weights):
    """How far the captions use the lexicon: captions int64 [N, T] and labels int64 [N] on the device of `weights` (a
    SentimentWordWeights) -> {label: {'captions', 'with_word' (captions with at least one lexicon word), 'hits' (positions
    paid), 'distinct' (lexicon words used)}} over the table's labels.  isc_sw_reward on a scratch copy of the state, no
    reward written; rows of a label outside the table are left out."""
    from . import ops
    captions = captions.to(torch.int64).contiguous()
    labels = labels.to(torch.int64).contiguous()
    state = (weights.state != 0).to(torch.uint8)
    hits = torch.empty(captions.shape[0], dtype=torch.int32, device=captions.device)
    ops.sw_reward(captions, labels, weights.weights, state, 0.0, None, False, None, hits, True)
    hits, labels, distinct = hits.cpu().numpy(), labels.cpu().numpy(), (state == 2).sum(dim=1).cpu().numpy()
    out = {}
    for lab in range(weights.n_labels):
        h = hits[labels == lab]
        out[lab] = {'captions': int(h.size), 'with_word': int((h > 0).sum()), 'hits': int(h.sum()),
                    'distinct': int(distinct[lab])}
    return out
