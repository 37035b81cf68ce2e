"""numpy restatement of the device CIDEr-D kernel (csrc/cider_dev.hip), for the tests.  It is driven only by what the
host library exports for the device - the open-addressing table (CiderD.device_table) and the cooked references
(CiderD.cook_refs) - and repeats the kernel's steps: packed keys (csrc/cider_key.h), the probe sequence, first-occurrence
order, sums over positions in ascending order, the zero-norm guard, references ascending.  Python floats are IEEE fp64:
apart from exp this is the host scorer's arithmetic."""
import math

import numpy as np

MASK64 = (1 << 64) - 1
MAX_ID = 65534


def pack_key(ids):
    """The key of an n-gram of order len(ids) <= 4: field j (16 bits) holds ids[j] + 1, unused fields 0."""
    assert 1 <= len(ids) <= 4 and all(0 <= int(w) <= MAX_ID for w in ids)
    key = 0
    for j, w in enumerate(ids):
        key |= (int(w) + 1) << (16 * j)
    return key


def unpack_key(key):
    out = []
    for j in range(4):
        f = (int(key) >> (16 * j)) & 0xFFFF
        if not f:
            break
        out.append(f - 1)
    return out


def hash_key(key):
    """isc_cider_hash: the splitmix64 finaliser."""
    key = int(key)
    key ^= key >> 30
    key = (key * 0xBF58476D1CE4E5B9) & MASK64
    key ^= key >> 27
    key = (key * 0x94D049BB133111EB) & MASK64
    key ^= key >> 31
    return key


def probe(table, key):
    """(log_df, slot, probes) of `key` in the CIDER_SLOT array, log_df = 0.0 and slot = -1 when absent; at most
    len(table) probes, as the kernel."""
    mask = len(table) - 1
    assert len(table) & mask == 0
    s = hash_key(key) & mask
    keys = table['key']
    for p in range(len(table)):
        k = int(keys[s])
        if k == key:
            return float(table['log_df'][s]), s, p + 1
        if k == 0:
            return 0.0, -1, p + 1
        s = (s + 1) & mask
    return 0.0, -1, len(table)


def normalise(row, sos, eos):
    """Drop a leading <SOS>, cut at the first <EOS>, append <EOS>."""
    row = [int(x) for x in row]
    i = 1 if row and row[0] == sos else 0
    out = []
    for w in row[i:]:
        if w == eos:
            break
        out.append(w)
    return out + [eos]


def cook_hyp(words, table, ref_len, n=4):
    """Per order o: the lists over the positions (keys, x, first) as the lanes of the kernel hold them, then norms [4]
    (sequential sums over the positions, + 0.0 where a position is no first occurrence) and the bigram length."""
    L = len(words)
    keys, xs, firsts, norms = [], [], [], []
    length = 0.0
    for o in range(4):
        k = o + 1
        kk = [pack_key(words[i:i + k]) if (o < n and i + k <= L) else 0 for i in range(L)]
        x, first = [0.0] * L, [False] * L
        for i in range(L):
            if not kk[i]:
                continue
            tf = float(sum(1 for j in range(L) if kk[j] == kk[i]))
            first[i] = not any(kk[j] == kk[i] for j in range(i))
            if first[i]:
                x[i] = tf * (ref_len - probe(table, kk[i])[0])
                if o == 1:
                    length += tf
        acc = 0.0
        for i in range(L):
            acc += x[i] * x[i]
        keys.append(kk), xs.append(x), firsts.append(first), norms.append(math.sqrt(acc))
    return keys, xs, firsts, norms, length


def score_rows(hyps, cooked_per_image, table, params, sos, eos, row_div=1):
    """hyps int64 [N, T]; cooked_per_image[i] = CiderD.cook_refs(captions of image i); params = CiderD.device_params();
    row r belongs to image r // row_div -> float64 [N]."""
    ref_len, n, sigma = params
    out = np.empty(len(hyps), dtype=np.float64)
    for r, row in enumerate(hyps):
        words = normalise(row, sos, eos)
        L = len(words)
        hk, hx, hfirst, hnorm, hlen = cook_hyp(words, table, ref_len, n)
        rkeys, rvals, ord_off, rnorms, rlen = cooked_per_image[r // row_div]
        score = [0.0] * 4
        for c in range(len(rlen)):
            a, b = int(ord_off[c, 0]), int(ord_off[c, 4])
            where = {int(k): float(v) for k, v in zip(rkeys[a:b], rvals[a:b])}       # (keys of different orders differ)
            delta = hlen - float(rlen[c])
            pen = math.exp(-(delta * delta) / (2 * sigma * sigma))
            for o in range(n):
                val = 0.0
                for i in range(L):
                    rv = where.get(hk[o][i], 0.0) if hk[o][i] else 0.0
                    val += (min(hx[o][i], rv) * rv) if hfirst[o][i] else 0.0
                nr = float(rnorms[c, o])
                if hnorm[o] != 0 and nr != 0:
                    val /= (hnorm[o] * nr)
                val *= pen
                score[o] += val
        s = 0.0
        for o in range(n):
            s += score[o]
        s /= float(n)
        s /= float(len(rlen))
        out[r] = s * 10.0
    return out
