"""Batch-tuple producers in front of the hot path.

* `create_collate_fn(name, ...)` - the four collate layouts the decoder path consumes, with the
  semantics of /root/reference/dataloader.py:8-109 (`caption`, `senti_corpus_with_sentis` alias `scs`,
  `rl_fact`, `rl_senti`): 5-captions-per-image expansion, stable sort by caption length (descending),
  truncation to `max_seq_len`, <PAD> filling, `lengths - 1`.  Pinned by outputs of the reference's own
  collates (tests/golden/collate.npz, written by tests/golden/make_golden.py::case_collate).
* `FeatureStore` + `CaptionDataset` / `SCSDataset` / `RLFactDataset` / `RLSentiDataset` and the four
  `get_*_dataloader` factories (dataloader.py:152-222,267-328): same constructor arguments and item tuples as
  the reference's classes, but the per-item `h5py.File(...)[fn][:]` (dataloader.py:171-178: two file opens per
  image) is replaced by one memory-mapped `[N, ...]` fp32 array + a name index, so a batch is a row gather.  The
  reference's own `.h5` feature files are taken as they are where h5py exists (`H5FeatureStore`: a path ending in
  .h5 / .hdf5 handed to a Dataset class; opened once per process) and converted once with `FeatureStore.from_h5`.
* `ConceptDataset` / `concept_collate_fn` / `get_concept_dataloader` (dataloader.py:111-115,230-245,338-345), `tag_concepts`
  (what detect_concepts.py writes) and `SentimentWordTable` (preprocess.py:280-302 on the host and on the device): the
  concept pre-stage, at the end of this file.
* `DevicePrefetcher` - pinned host staging + asynchronous H2D copies on a side HIP stream, one batch
  ahead of the consumer: at >10k captions/s the 303 KB of fp32 region features per caption
  (~3 GB/s and more) must overlap with decoding instead of serialising in front of it.
"""
import os
import random

import numpy as np
import torch
import torch.utils.data


def _pad_rows(seqs, width, pad_index, limit=None):
    out = np.full((len(seqs), width), pad_index, dtype=np.int64)
    for i, s in enumerate(seqs):
        end = min(len(s), width if limit is None else limit)
        out[i, :end] = s[:end]
    return torch.from_numpy(out)


def _caps(caps, max_seq_len, pad_index, caption_width=None):
    lengths = [min(len(c), max_seq_len) for c in caps]
    width = lengths[0]                                     # rows are sorted: lengths[0] is the maximum
    if caption_width == 'full':
        width = max_seq_len
    elif caption_width:                                    # an int m: the batch's width rounded up to a multiple of m
        width = min(max_seq_len, (width - 1 + int(caption_width) - 1) // int(caption_width) * int(caption_width) + 1)
    tensor = _pad_rows(caps, width, pad_index, limit=max_seq_len)
    return tensor, [l - 1 for l in lengths]


def _feats(xs):
    if len(xs) and hasattr(xs[0], 'row') and hasattr(xs[0], 'tensor'):     # rows of a DeviceFeatureStore: gathered on the device
        return RowGather(xs[0].tensor, torch.from_numpy(np.asarray([x.row for x in xs], dtype=np.int64)))
    # float16 items (a store written with dtype=float16) stay float16; a mixed or any other batch is fp32, as ever
    f16 = len(xs) > 0 and all(getattr(x, 'dtype', None) == np.float16 for x in xs)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(xs, dtype=np.float16 if f16 else np.float32)))


def _feature_dtype(dtype):
    """np.float32 / np.float16 for the `dtype=` of the stores (numpy or torch spelling)."""
    if dtype in (torch.float16, torch.float32):
        return np.float16 if dtype == torch.float16 else np.float32
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float16), np.dtype(np.float32)):
        raise ValueError('feature stores hold float32 or float16, not %s' % (dt,))
    return dt.type


def _as_feature(array, dtype):
    """`array` as `dtype` (np.float32 / np.float16).  A finite value that float16 would round to +-inf raises: the
    split-f16 engine's domain ends at 65504 and an inf must never be STORED silently."""
    if dtype == np.float32 or getattr(array, 'dtype', None) == np.float16:
        return np.asarray(array, dtype=dtype)
    src = np.asarray(array)
    with np.errstate(over='ignore'):
        out = src.astype(np.float16)
    bad = np.isinf(out) & np.isfinite(src)
    if bad.any():
        raise ValueError('float16 features: max |x| = %g of the values beyond 65504 would be stored as inf - scale the '
                         'features or keep float32' % float(np.abs(src[bad]).max()))
    return out


class RowGather:
    """A batch tensor whose rows repeat: `base` [U, ...] holds each distinct row once, `index` [B] says which one a batch row
    is.  The 'caption' collate makes one row per CAPTION, so an image's 6 x 6 x 2048 regions appear once per caption (4-5x):
    with `dedup=True` it hands the features over in this form - a quarter of the bytes to stack, pin and copy to the device
    - and DevicePrefetcher expands them there (index_select on its stream): the consumer sees the plain [B, ...] tensors.
    `dense()` gives the expanded tensor where it stands (host or device)."""

    def __init__(self, base, index):
        self.base, self.index = base, index

    @property
    def shape(self):
        return (self.index.shape[0],) + tuple(self.base.shape[1:])

    def _index_on(self, device):
        # (through pinned memory, asynchronously: a pageable copy to the device is stream-ordered AND blocks the host - the
        # few KB of row numbers would make every batch wait for the previous iteration's whole graph)
        if self.index.device == device:
            return self.index
        if device.type == 'cuda' and not self.index.is_cuda:
            src = self.index if self.index.is_pinned() else self.index.pin_memory()
            return src.to(device, non_blocking=True)
        return self.index.to(device)

    def dense(self):
        return self.base.index_select(0, self._index_on(self.base.device))

    def to(self, device, non_blocking=False):
        """The expanded tensor on `device` (what a consumer's `batch_tensor.to(device)` expects to get)."""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        base = self.base if self.base.device == device else self.base.to(device, non_blocking=non_blocking)
        return base.index_select(0, self._index_on(device))

    @property
    def is_cuda(self):
        return self.base.is_cuda


def create_collate_fn(name, pad_index=0, max_seq_len=17, num_concepts=5, num_sentiments=10, caption_width=None,
                      dedup=False, captions_per_image=None):
    """The reference's collate functions (dataloader.py:11-58).  `caption_width` (not in the reference): None pads a batch's
    captions to its longest one, as the reference does - every distinct longest length is then another input geometry for
    the graph-served training steps (train_graph: a capture per geometry, four kept); 'full' pads every batch to
    max_seq_len, an int m rounds the unroll length (width - 1) up to a multiple of m.  Lengths are returned unchanged and the
    criteria mask by row, so losses and gradients are those of the tight batch - the extra steps run on <PAD>.
    `dedup` ('caption' only; not in the reference): features as RowGather (each image once + a row index).
    `captions_per_image=n` ('caption' only; not in the reference): the batch of Captioner.forward_xe(...,
    captions_per_image=n) - features and `cpts` of the I images, each ONCE, in dataset order; captions image-major with
    exactly n per image, [I*n, L] (row i*n + j = caption j of image i): the first n of the image's captions, cycled from
    its first one when it has fewer (no random choice); `fns` and the lengths per caption row.  The rows are the default
    collate's rows of those captions in another order (image-major instead of sorted by length).  `dedup` has nothing
    left to do then."""
    if captions_per_image is not None:
        if (isinstance(captions_per_image, bool) or not hasattr(captions_per_image, '__index__')
                or int(captions_per_image) < 1):
            raise ValueError('captions_per_image must be an integer >= 1, got %r' % (captions_per_image,))
        if name != 'caption':
            raise ValueError('captions_per_image belongs to the caption collate, not to %r' % (name,))
        captions_per_image = int(captions_per_image)

    def caption_grouped(dataset):
        n = captions_per_image
        fns, caps = [], []
        for fn, _, _, caps_idx, _ in dataset:
            if len(caps_idx) == 0:
                raise ValueError('captions_per_image: image %r has no caption' % (fn,))
            fns += [fn] * n
            caps += [caps_idx[j % len(caps_idx)] for j in range(n)]
        lengths = [min(len(c), max_seq_len) for c in caps]
        # (_caps pads to its FIRST row's length - its rows are sorted; here the longest row may stand anywhere)
        longest = max(range(len(caps)), key=lengths.__getitem__)
        tensor, _ = _caps([caps[longest]] + caps, max_seq_len, pad_index, caption_width)
        return tuple(fns), _feats([d[1] for d in dataset]), _feats([d[2] for d in dataset]), \
            (tensor[1:], [l - 1 for l in lengths]), _pad_rows([d[4] for d in dataset], num_concepts, pad_index)

    def caption(dataset):
        rows = [(fn, fc, att, cap, cpts, u) for u, (fn, fc, att, caps_idx, cpts) in enumerate(dataset) for cap in caps_idx]
        rows.sort(key=lambda p: len(p[3]), reverse=True)          # stable, like the reference
        fns, fcs, atts, caps, cpts, img = zip(*rows)
        if dedup:           # an image's features once (RowGather); same rows after DevicePrefetcher / .dense()
            index = torch.from_numpy(np.asarray(img, dtype=np.int64))
            fc_u, att_u = _feats([d[1] for d in dataset]), _feats([d[2] for d in dataset])
            if isinstance(fc_u, RowGather):      # device-resident store: rows of rows - one gather
                fc_t, att_t = RowGather(fc_u.base, fc_u.index[index]), RowGather(att_u.base, att_u.index[index])
            else:
                fc_t, att_t = RowGather(fc_u, index), RowGather(att_u, index)
        else:
            fc_t, att_t = _feats(fcs), _feats(atts)
        return fns, fc_t, att_t, _caps(caps, max_seq_len, pad_index, caption_width), \
            _pad_rows(cpts, num_concepts, pad_index)

    def scs(dataset):
        rows = sorted(dataset, key=lambda p: len(p[0]), reverse=True)
        caps, cpts, sentis, senti_ids = zip(*rows)
        return _caps(caps, max_seq_len, pad_index, caption_width), _pad_rows(cpts, num_concepts, pad_index), \
            _pad_rows(sentis, num_sentiments, pad_index), torch.from_numpy(np.asarray(senti_ids, dtype=np.int64))

    def rl_fact(dataset):
        ground_truth, rows = {}, []
        for fn, caps_idx, fc, att, cpts, sentis in dataset:
            ground_truth[fn] = [c[:max_seq_len] for c in caps_idx]
            rows.append((fn, random.sample(caps_idx, 1)[0], fc, att, cpts, sentis))
        rows.sort(key=lambda p: len(p[1]), reverse=True)
        fns, caps, fcs, atts, cpts, sentis = zip(*rows)
        return fns, _feats(fcs), _feats(atts), _caps(caps, max_seq_len, pad_index, caption_width), \
            _pad_rows(cpts, num_concepts, pad_index), _pad_rows(sentis, num_sentiments, pad_index), ground_truth

    def rl_senti(dataset):
        fns, fcs, atts, cpts, sentis, labels = zip(*dataset)
        return fns, _feats(fcs), _feats(atts), _pad_rows(cpts, num_concepts, pad_index), \
            _pad_rows(sentis, num_sentiments, pad_index), torch.from_numpy(np.asarray(labels, dtype=np.int64))

    def senti_sents(dataset):
        # dataloader.py:123-134 (the sentence classifier's own training): (label, ids) pairs, longest first (stable), cut at
        # max_seq_len, padded to the first row -> labels [B], (caps [B, lengths[0]], lengths) - the lengths are the rows'
        # own, not minus one: the classifier reads the whole sentence
        rows = sorted(dataset, key=lambda p: len(p[1]), reverse=True)
        sentis, caps = zip(*rows)
        lengths = [min(len(c), max_seq_len) for c in caps]
        return torch.from_numpy(np.asarray(sentis, dtype=np.int64)), \
            (_pad_rows(caps, lengths[0], pad_index, limit=max_seq_len), lengths)

    table = {'caption': caption if captions_per_image is None else caption_grouped, 'scs': scs, 'senti_corpus_with_sentis': scs, 'rl_fact': rl_fact,
             'rl_senti': rl_senti, 'senti_sents': senti_sents, 'senti_image': senti_image_collate_fn}
    if name not in table:
        raise KeyError('collate %r is outside the decoder path (have: %s)' % (name, sorted(table)))
    return table[name]


class FeatureStore:
    """fn -> fp32 (or, written with dtype=np.float16, float16) feature array, backed by ONE `.npy` file opened as a memory map plus `<path>.index.json`
    ({fn: row}).  Stands where the reference passes an h5 file name (`fc_feats` / `att_feats` arguments of its
    Dataset classes, dataloader.py:164-178): `store[fn]` returns what `h5py.File(path)[fn][:]` returned there.
    A plain dict {fn: ndarray} is accepted by the datasets as well."""

    def __init__(self, path):
        import json
        self.path = path
        self.array = np.load(path, mmap_mode='r')
        with open(path + '.index.json') as f:
            self.index = json.load(f)

    @staticmethod
    def write(path, fns, array, dtype=np.float32):
        """dtype=np.float16 halves the file (and every copy behind it); a value it cannot hold raises ValueError."""
        import json
        array = np.ascontiguousarray(_as_feature(array, _feature_dtype(dtype)))
        assert len(fns) == array.shape[0] and len(set(fns)) == len(fns)
        np.save(path, array)
        if not path.endswith('.npy'):
            path = path + '.npy'
        with open(path + '.index.json', 'w') as f:
            json.dump({fn: i for i, fn in enumerate(fns)}, f)
        return path

    @classmethod
    def from_h5(cls, h5_path, npy_path, fns=None, dtype=np.float32):
        """One-off conversion of a reference feature file (an h5 dataset per image, dataloader.py:171-178) into the
        memory-mapped `.npy` + index pair; returns the opened store.  Needs h5py (H5FeatureStore says so)."""
        src = H5FeatureStore(h5_path)
        fns = list(fns if fns is not None else src.keys())
        first = src[fns[0]]
        path = npy_path if npy_path.endswith('.npy') else npy_path + '.npy'
        dtype = _feature_dtype(dtype)
        out = np.lib.format.open_memmap(path, mode='w+', dtype=dtype, shape=(len(fns),) + first.shape)
        for i, fn in enumerate(fns):            # row by row: the set does not have to fit in host memory
            out[i] = _as_feature(src[fn], dtype)
        out.flush()
        del out
        import json
        with open(path + '.index.json', 'w') as f:
            json.dump({fn: i for i, fn in enumerate(fns)}, f)
        return cls(path)

    def __getitem__(self, fn):
        return np.array(self.array[self.index[fn]])

    def __contains__(self, fn):
        return fn in self.index

    def keys(self):
        return list(self.index)

    def __len__(self):
        return len(self.index)


class H5FeatureStore:
    """fn -> fp32 feature array straight out of the reference's own feature files: one h5 dataset per image file name
    (dataloader.py:171-178 `h5py.File(path, mode='r')[fn][:]`).  A caller that hands the Dataset classes the `.h5` / `.hdf5`
    paths it handed the reference's gets this store (`_store`).  Differences to the reference's access pattern, none
    visible in what an item holds: the file is opened ONCE per process (per loader worker: the handle is dropped on
    pickling and re-opened lazily) instead of twice per item.  Needs `h5py`, imported here and nowhere else - without
    it the call raises with the one-off conversion named (`FeatureStore.from_h5`, run wherever h5py exists).
    Parity: unpinned against real h5 files in this build's image (no h5py); the tests drive it through a stand-in
    module with h5py's `File(path, 'r')[fn][:]` surface."""

    def __init__(self, path):
        self.path, self._file = path, None
        self._open()

    def _open(self):
        if self._file is None:
            try:
                import h5py
            except ImportError as e:
                raise ImportError('%r is an h5 feature file and h5py is not importable here: install h5py, or convert the '
                                  'file once with data.FeatureStore.from_h5(h5_path, npy_path) on a machine that has it '
                                  '(the .npy + index pair needs numpy only)' % (self.path,)) from e
            self._file = h5py.File(self.path, mode='r')
        return self._file

    def __getstate__(self):                     # loader workers get the path, not the open handle
        return {'path': self.path, '_file': None}

    def __getitem__(self, fn):
        return np.asarray(self._open()[fn][:], dtype=np.float32)

    def __contains__(self, fn):
        return fn in self._open()

    def __len__(self):
        return len(self._open())

    def keys(self):
        return list(self._open().keys())


class _Row:
    """What a DeviceFeatureStore hands a dataset item instead of the feature array: which row of which device tensor."""
    __slots__ = ('tensor', 'row')

    def __init__(self, tensor, row):
        self.tensor, self.row = tensor, row


class DeviceFeatureStore:
    """All features of a dataset RESIDENT ON THE DEVICE: fn -> row of one [N, ...] fp32 tensor in HBM (`dtype=torch.float16`:
    a float16 tensor, half the bytes; inference reads it as it is, training converts a batch to fp32 in front of its prologue).  The reference reads
    an image's features from an h5 file per item (dataloader.py:164-178) and a 512-image RL batch of 6 x 6 x 2048 regions is
    151 MB to read, stack, pin and copy - 55-76 ms on the host per iteration, against 22.5 ms for the iteration itself
    (tools/rl_loop_probe.py).  An MI355X has 288 GB: the 113 k training images of COCO are 34 GB at 6 x 6 regions (160 GB
    at the encoder's own 14 x 14), so the whole set is uploaded once and a batch is an index_select on the device (151 MB
    in ~50 us).  Datasets take it where they take a FeatureStore / dict; their items then carry row handles, the collates
    turn them into a RowGather over the store's tensor, and DevicePrefetcher (or RowGather.to(device) / .dense()) gives the
    consumer the plain [B, ...] tensor.  Loader workers: num_workers = 0 (a batch is a few KB of indices and captions).

        fc_store  = data.DeviceFeatureStore.from_arrays(fns, fc_array,  device)      # or .from_store(FeatureStore / dict)
        att_store = data.DeviceFeatureStore.from_arrays(fns, att_array, device)
        loader = data.get_rl_fact_dataloader(fc_store, att_store, ...)"""

    def __init__(self, index, tensor):
        self.index, self.tensor = index, tensor

    @classmethod
    def from_arrays(cls, fns, array, device, chunk_rows=4096, dtype=torch.float32):
        assert len(fns) == len(array) and len(set(fns)) == len(fns)
        device = torch.device(device)
        np_dtype = _feature_dtype(dtype)
        t_dtype = torch.float16 if np_dtype == np.float16 else torch.float32
        first = np.asarray(array[0])
        out = torch.empty((len(fns),) + first.shape, dtype=t_dtype, device=device)
        pin = torch.empty((min(chunk_rows, len(fns)),) + first.shape, dtype=t_dtype).pin_memory()
        for lo in range(0, len(fns), chunk_rows):                 # through one kept pinned chunk: no 34 GB host copy
            hi = min(lo + chunk_rows, len(fns))
            np.stack([_as_feature(array[i], np_dtype) for i in range(lo, hi)], out=pin.numpy()[:hi - lo])
            out[lo:hi].copy_(pin[:hi - lo], non_blocking=True)
            torch.cuda.current_stream(device).synchronize()       # (the chunk buffer is reused)
        return cls({fn: i for i, fn in enumerate(fns)}, out)

    @classmethod
    def from_store(cls, store, device, fns=None, dtype=torch.float32):
        store = _store(store)
        fns = list(fns if fns is not None else store.keys())
        return cls.from_arrays(fns, [store[fn] for fn in fns], device, dtype=dtype)

    def __getitem__(self, fn):
        return _Row(self.tensor, self.index[fn])

    def __contains__(self, fn):
        return fn in self.index

    def __len__(self):
        return len(self.index)


def _store(x):
    """What the Dataset classes take for `fc_feats` / `att_feats`: a path - the reference's `.h5` / `.hdf5` file
    (H5FeatureStore) or this package's `.npy` (FeatureStore) - or any fn -> array mapping (dict, DeviceFeatureStore)."""
    if isinstance(x, (str, os.PathLike)):
        x = os.fspath(x)
        return H5FeatureStore(x) if x.lower().endswith(('.h5', '.hdf5', '.hdf')) else FeatureStore(x)
    return x


def _item(x):
    """A dataset item's feature: a copy of the array (the reference reads it out of its h5 file), or the row handle of a
    device-resident store."""
    return x if isinstance(x, _Row) else np.array(x)


class SCSDataset(torch.utils.data.Dataset):
    """dataloader.py:152-161: rows (caption ids, concept ids, sentiment-word ids, sentiment id)."""

    def __init__(self, senti_corpus_with_sentis):
        self.senti_corpus_with_sentis = senti_corpus_with_sentis

    def __getitem__(self, index):
        cap, cpts, sentis, senti_id = self.senti_corpus_with_sentis[index]
        return cap, cpts, sentis, senti_id

    def __len__(self):
        return len(self.senti_corpus_with_sentis)


class CaptionDataset(torch.utils.data.Dataset):
    """dataloader.py:164-182: item = (fn, fc [F], att [...,F], captions of the image, detected concepts)."""

    def __init__(self, fc_feats, att_feats, img_captions, img_det_concepts):
        self.fc_feats, self.att_feats = _store(fc_feats), _store(att_feats)
        self.captions = list(img_captions.items())
        self.det_concepts = img_det_concepts

    def __getitem__(self, index):
        fn, caps = self.captions[index]
        return fn, _item(self.fc_feats[fn]), _item(self.att_feats[fn]), caps, self.det_concepts[fn]

    def __len__(self):
        return len(self.captions)


class RLFactDataset(torch.utils.data.Dataset):
    """dataloader.py:185-206: item = (fn, captions, fc, att, concepts, sentiment words)."""

    def __init__(self, fc_feats, att_feats, img_captions, img_det_concepts, img_det_sentiments):
        self.fc_feats, self.att_feats = _store(fc_feats), _store(att_feats)
        self.captions = list(img_captions.items())
        self.det_concepts, self.det_sentiments = img_det_concepts, img_det_sentiments

    def __getitem__(self, index):
        fn, caps = self.captions[index]
        return fn, caps, _item(self.fc_feats[fn]), _item(self.att_feats[fn]), self.det_concepts[fn], \
            self.det_sentiments[fn]

    def __len__(self):
        return len(self.captions)


class RLSentiDataset(torch.utils.data.Dataset):
    """dataloader.py:209-230: item = (fn, fc, att, concepts, sentiment words, sentiment label)."""

    def __init__(self, fc_feats, att_feats, img_det_concepts, img_det_sentiments, img_senti_labels):
        self.fc_feats, self.att_feats = _store(fc_feats), _store(att_feats)
        self.det_concepts, self.det_sentiments = img_det_concepts, img_det_sentiments
        self.img_senti_labels = img_senti_labels

    def __getitem__(self, index):
        fn, senti_label = self.img_senti_labels[index]
        return fn, _item(self.fc_feats[fn]), _item(self.att_feats[fn]), self.det_concepts[fn], \
            self.det_sentiments[fn], senti_label

    def __len__(self):
        return len(self.img_senti_labels)


def _loader(dataset, batch_size, num_workers, shuffle, collate):
    return torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers,
                                       collate_fn=collate)


def get_caption_dataloader(fc_feats, att_feats, img_captions, img_det_concepts, pad_index, max_seq_len,
                           num_concepts, batch_size, num_workers=0, shuffle=True, caption_width=None, dedup=False,
                           captions_per_image=None):
    """dataloader.py:267-278 (note max_seq_len + 1: the <SOS> column).  caption_width, dedup, captions_per_image:
    create_collate_fn."""
    return _loader(CaptionDataset(fc_feats, att_feats, img_captions, img_det_concepts), batch_size, num_workers,
                   shuffle, create_collate_fn('caption', pad_index, max_seq_len + 1, num_concepts,
                                              caption_width=caption_width, dedup=dedup,
                                              captions_per_image=captions_per_image))


def get_senti_corpus_with_sentis_dataloader(senti_corpus_with_sentis, pad_index, max_seq_len, num_concepts,
                                            num_sentiments, batch_size, num_workers=0, shuffle=True,
                                            caption_width=None):
    """dataloader.py:281-294."""
    return _loader(SCSDataset(senti_corpus_with_sentis), batch_size, num_workers, shuffle,
                   create_collate_fn('senti_corpus_with_sentis', pad_index, max_seq_len + 1,
                                     num_concepts=num_concepts, num_sentiments=num_sentiments,
                                     caption_width=caption_width))


def get_rl_fact_dataloader(fc_feats, att_feats, img_captions, img_det_concepts, img_det_sentiments, pad_index,
                           max_seq_len, num_concepts, num_sentiments, batch_size, num_workers=0, shuffle=True,
                           caption_width=None):
    """dataloader.py:297-312."""
    return _loader(RLFactDataset(fc_feats, att_feats, img_captions, img_det_concepts, img_det_sentiments),
                   batch_size, num_workers, shuffle,
                   create_collate_fn('rl_fact', pad_index=pad_index, max_seq_len=max_seq_len + 1,
                                     num_concepts=num_concepts, num_sentiments=num_sentiments,
                                     caption_width=caption_width))


def get_rl_senti_dataloader(fc_feats, att_feats, img_det_concepts, img_det_sentiments, img_senti_labels, pad_index,
                            num_concepts, num_sentiments, batch_size, num_workers=0, shuffle=True):
    """dataloader.py:315-328."""
    return _loader(RLSentiDataset(fc_feats, att_feats, img_det_concepts, img_det_sentiments, img_senti_labels),
                   batch_size, num_workers, shuffle,
                   create_collate_fn('rl_senti', pad_index=pad_index, num_concepts=num_concepts,
                                     num_sentiments=num_sentiments))


def freeze_host_objects():
    """Call once after the caption / concept dictionaries and the loaders are built.  A COCO-sized caption table is
    millions of small Python objects; every batch's collate allocates a few thousand containers, so the cyclic garbage
    collector walks ALL of them every few iterations - 20 ms pauses in front of a 22 ms RL iteration, a collate that takes
    4 ms in one epoch and 22 ms in the next (tools/pf_rl_probe.py).  gc.freeze() moves everything alive now into a
    permanent generation the collector no longer traverses (nothing is leaked: reference counting still frees it)."""
    import gc
    gc.collect()
    gc.freeze()


def _map_tensors(obj, fn):
    if torch.is_tensor(obj):
        return fn(obj)
    if isinstance(obj, RowGather):          # both parts through fn; expanded by the caller where it wants the rows
        return RowGather(fn(obj.base), fn(obj.index))
    if isinstance(obj, tuple):
        return tuple(_map_tensors(o, fn) for o in obj)
    if isinstance(obj, list) and obj and torch.is_tensor(obj[0]):
        return [_map_tensors(o, fn) for o in obj]
    return obj          # file names, length lists, ground-truth dicts stay on the host


def _expand(obj):
    if isinstance(obj, RowGather):
        return obj.dense()
    if isinstance(obj, tuple):
        return tuple(_expand(o) for o in obj)
    return obj


class DevicePrefetcher:
    """Wraps an iterable of collated batches: every tensor is staged in pinned memory and copied to
    `device` on a dedicated stream while the previous batch is being consumed."""

    def __init__(self, loader, device):
        self.loader, self.device = loader, torch.device(device)
        # a stream no other owner of this package holds: torch hands its 32 pool streams out round robin, and a prefetch
        # stream that IS a training graph's stream made every pinned-buffer wait below a wait for that graph's backward
        # pass (an RL epoch over a device-resident store: 23.9 -> 36 ms per iteration)
        from . import ops
        import weakref
        self.stream = ops.private_stream(self.device)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        weakref.finalize(self, ops.release_stream_state, idx, self.stream.cuda_stream)
        # pinned staging buffers, kept: two slots (the batch being consumed, the batch on its way) x the tensors of a
        # batch, each a byte buffer that only grows.  `tensor.pin_memory()` per batch page-locks fresh memory every time
        # here - 38 ms for the 38 MB of a 128-row batch of 6 x 6 x 2048 regions, against 4.7 ms to collate it and 4.6 ms
        # to train on it (tools/loader_probe.py)
        self._pins, self._slot = {}, 0

    def __len__(self):
        return len(self.loader)

    def _pinned(self, key, t):
        need = t.numel() * t.element_size()
        ent = self._pins.get(key)
        if ent is None or ent[0].numel() < need:
            ent = self._pins[key] = [torch.empty(max(need + need // 2, 256), dtype=torch.uint8).pin_memory(),
                                     torch.cuda.Event()]
        else:
            ent[1].synchronize()                 # the copy that last read this buffer has finished (two batches ago)
        return ent[0][:need].view(t.dtype).view(t.shape), ent[1]

    def _stage(self, batch):
        self._slot ^= 1
        n = [0]

        def put(t):
            if t.is_cuda:
                return t
            if t.is_pinned():
                return t.to(self.device, non_blocking=True)
            buf, ev = self._pinned((self._slot, n[0]), t)
            n[0] += 1
            # a plain memcpy on THIS thread: torch's copy_ of a 38 MB tensor opens an OpenMP region on every core the HOST
            # has (128) even when the process may use 16 of them, and the pool's threads then spin for a while - the next
            # batch's collate (numpy, this thread) ran 5x slower next to them (tools/pf_probe.py: 25 -> 5.7 ms)
            if t.is_contiguous() and t.dtype != torch.bool:
                np.copyto(buf.numpy(), t.numpy())
            else:
                buf.copy_(t)
            out = buf.to(self.device, non_blocking=True)
            ev.record(self.stream)
            return out
        with torch.cuda.stream(self.stream):
            return _map_tensors(batch, put)

    def __iter__(self):
        it = iter(self.loader)
        try:
            nxt = self._stage(next(it))
        except StopIteration:
            return
        while nxt is not None:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)      # batch `nxt` has landed
            cur = nxt
            _map_tensors(cur, lambda t: t.record_stream(torch.cuda.current_stream(self.device)) or t)
            # repeated rows (dedup collate, device-resident stores) are expanded HERE, on the consumer's stream: the
            # [B, ...] tensors then come out of that stream's memory pool, which the next batch reuses (expanded on the
            # prefetch stream a 512-image batch allocated 151 MB there per iteration: 23.5 -> 38.9 ms per RL iteration)
            cur = _expand(cur)
            try:
                nxt = self._stage(next(it))                                      # overlaps with the consumer
            except StopIteration:
                nxt = None
            yield cur


# ---------------------------------------------------------------------------- concept detector (dataloader.py:111-115,230-245,338-345)
def concept_collate_fn(dataset):
    """The reference's 'concept' collate (dataloader.py:111-115): items (fn, fc [F], 0/1 vector [C]) -> (fns, fc_feats
    [B, F] fp32 - float16 when every item is -, targets [B, C] int64).  (create_collate_fn keeps the decoder path's four
    names and the sentence classifier's 'senti_sents'; this one stands beside it.)"""
    fns, fcs, cpts = zip(*dataset)
    return fns, _feats(fcs), torch.from_numpy(np.asarray(cpts).astype(np.int64))


class ConceptDataset(torch.utils.data.Dataset):
    """dataloader.py:230-245: item = (fn, fc [F], int16 vector [num_cpts] with ones at the image's concept indices)."""

    def __init__(self, fc_feats, img_concepts, num_cpts):
        self.fc_feats = _store(fc_feats)
        self.concepts = list(img_concepts.items())
        self.num_cpts = num_cpts

    def __getitem__(self, index):
        fn, cpts_idx = self.concepts[index]
        cpts = np.zeros(self.num_cpts, dtype=np.int16)
        cpts[cpts_idx] = 1
        return fn, _item(self.fc_feats[fn]), cpts

    def __len__(self):
        return len(self.concepts)


def get_concept_dataloader(fc_feats, img_concepts, num_cpts, batch_size, num_workers=0, shuffle=True):
    """dataloader.py:338-345."""
    return _loader(ConceptDataset(fc_feats, img_concepts, num_cpts), batch_size, num_workers, shuffle, concept_collate_fn)


# ---------------------------------------------------------------------------- image-sentiment detector (dataloader.py:117-121,248-260,349-357)
def senti_image_collate_fn(dataset):
    """The reference's 'senti_image' collate (dataloader.py:117-121): items (fn, att [h, w, F], label) -> (fns, att_feats
    [B, h, w, F] fp32 - float16 when every item is, rows of a DeviceFeatureStore gathered on the device -, labels [B]
    int64)."""
    fns, atts, labels = zip(*dataset)
    return fns, _feats(atts), torch.from_numpy(np.asarray(labels, dtype=np.int64))


class SentiImageDataset(torch.utils.data.Dataset):
    """dataloader.py:248-260: item = (fn, att [h, w, F], sentiment label index) over [(fn, label index), ...]."""

    def __init__(self, senti_att_feats, img_senti_labels):
        self.att_feats = _store(senti_att_feats)
        self.img_senti_labels = list(img_senti_labels)

    def __getitem__(self, index):
        fn, senti_label = self.img_senti_labels[index]
        return fn, _item(self.att_feats[fn]), senti_label

    def __len__(self):
        return len(self.img_senti_labels)


def get_senti_image_dataloader(senti_att_feats, img_senti_labels, batch_size, num_workers=0, shuffle=True):
    """dataloader.py:349-357, over any of the project's feature stores (or a {fn: array} mapping)."""
    return _loader(SentiImageDataset(senti_att_feats, img_senti_labels), batch_size, num_workers, shuffle,
                   senti_image_collate_fn)


# ---------------------------------------------------------------------------- sentence classifier (dataloader.py:263-272,360-370)
class SentiSentDataset(torch.utils.data.Dataset):
    """dataloader.py:263-272: item = (sentiment id, the sentence's word ids as an array)."""

    def __init__(self, senti_sentences):
        self.senti_sentences = senti_sentences

    def __getitem__(self, index):
        senti, sent = self.senti_sentences[index]
        return senti, np.array(sent)

    def __len__(self):
        return len(self.senti_sentences)


def get_senti_sents_dataloader(senti_sentences, pad_index, max_seq_len, batch_size=80, num_workers=2, shuffle=True):
    """dataloader.py:360-370: batches of (labels [B], (caps [B, L], lengths)) for train.sent_cls_train_step."""
    return _loader(SentiSentDataset(senti_sentences), batch_size, num_workers, shuffle,
                   create_collate_fn('senti_sents', pad_index=pad_index, max_seq_len=max_seq_len))


def build_senti_sents_sets(senti_captions, word2idx, categories, val_counts=None, rng=random):
    """train_sent_senti_cls_rnn.py:69-95: the classifier's training list and validation lists from `senti_captions`
    {category: [[words, ...], ...]} (the first entry of every item is its word list).
    Per category: shuffle (rng.shuffle), the first val_counts[category] sentences are the validation set (the reference
    takes 5000 neutral and 1000 of each other category - the default), the rest train; 'positive' and 'negative' are then
    repeated int(len(neutral) / len(own)) times - whole-number oversampling.  Words become ids by
    `word2idx.get(w) or word2idx['<UNK>']` - so a word whose index is 0 becomes <UNK> too, as in the reference - plus <EOS>.
    The training list is shuffled once more.  -> (train_set [[senti_id, ids], ...], val_set {category: [[senti_id, ids], ...]})."""
    if val_counts is None:
        val_counts = {c: 5000 if c == 'neutral' else 1000 for c in senti_captions}
    caps = {}
    for senti in senti_captions:                        # (the dict's order: it is the order of the rng draws)
        caps[senti] = [c[0] for c in senti_captions[senti]]
        rng.shuffle(caps[senti])
    split = {'train': {}, 'val': {}}
    for senti in ('neutral', 'positive', 'negative'):
        split['train'][senti] = list(caps[senti][val_counts[senti]:])
        split['val'][senti] = list(caps[senti][:val_counts[senti]])
    for senti in ('positive', 'negative'):
        split['train'][senti] = split['train'][senti] * int(len(split['train']['neutral']) / len(split['train'][senti]))
    unk, eos = word2idx['<UNK>'], word2idx['<EOS>']
    to_ids = lambda cap: [word2idx.get(w, None) or unk for w in cap] + [eos]
    train_set, val_set = [], {}
    for senti_id, senti in enumerate(categories):
        train_set += [[senti_id, to_ids(cap)] for cap in split['train'][senti]]
        val_set[senti] = [[senti_id, to_ids(cap)] for cap in split['val'][senti]]
    rng.shuffle(train_set)
    return train_set, val_set


class SentimentWordTable:
    """The sentiment words of an image from its detected concepts (preprocess.py:280-302): per word the scores of the
    concepts' (word, score) lists are summed, the words sorted by sum (descending, stable), 20 kept.

    Built from the `sentiment_detector.json` mapping {concept: [[word, score], ...]} and `word2idx` (a word the
    vocabulary lacks raises KeyError, as train_rl.py:129 does).  `lookup` is the host form over concept NAMES; `forward`
    is the device kernel (isc_senti_words_from_concepts) over concept INDICES [B, num] - it needs `idx2concept`, the
    detector's index -> name list.  The kernel stages at most ops.SENTI_WORDS_CAP = 1024 candidates per image:
    `num_concepts` x the longest list above that raises ValueError here, at build time - never a silent cut."""
    KEEP = 20               # preprocess.py:301

    def __init__(self, sentiment_detector, word2idx, idx2concept=None, num_concepts=5):
        self.lists = {c: [(int(word2idx[w]), float(s)) for w, s in pairs] for c, pairs in sentiment_detector.items()}
        self.idx2concept = list(idx2concept) if idx2concept is not None else None
        self.num_concepts = int(num_concepts)
        self._csr, self._dev = None, {}
        if self.idx2concept is not None:
            off, word, score = [0], [], []
            for c in self.idx2concept:
                for w, s in self.lists.get(c, ()):
                    word.append(w)
                    score.append(s)
                off.append(len(word))
            from . import ops
            self.max_list = ops.senti_words_pack_check(off, self.num_concepts)      # ValueError beyond the cap
            self._csr = (torch.tensor(off, dtype=torch.int32), torch.tensor(word, dtype=torch.int64),
                         torch.tensor(score, dtype=torch.float64))

    def lookup(self, concept_lists):
        """[[concept name, ...] per image] -> [[vocabulary id, ...] per image], at most 20 each, best first: the pure-Python
        host form (get_img_det_sentiments followed by train_rl.py:129)."""
        out = []
        for concepts in concept_lists:
            sentis = []
            for con in concepts:
                sentis.extend(self.lists.get(con, []))
            if sentis:
                tmp = {}
                for w, s in sentis:
                    tmp[w] = tmp.get(w, 0.0) + s
                sentis = sorted(tmp.items(), key=lambda p: p[1], reverse=True)
                sentis = [w for w, _ in sentis]
            out.append(sentis[:self.KEEP])
        return out

    def lookup_tensor(self, concept_lists, n_out=10, pad_id=0):
        """`lookup` as the collates hand it on: int64 [B, n_out], filled with pad_id."""
        return _pad_rows(self.lookup(concept_lists), n_out, pad_id)

    def _on(self, device):
        device = torch.device(device)
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = tuple(x.to(device) for x in self._csr)
        return t

    def forward(self, idx, n_out=10, pad_id=0):
        """idx [B, num] int64 concept indices on the device -> int64 [B, n_out] vocabulary ids there; no host read."""
        if self._csr is None:
            raise ValueError('SentimentWordTable.forward needs idx2concept (the detector\'s index -> name list)')
        from . import ops
        if idx.shape[1] > self.num_concepts:
            ops.senti_words_pack_check(self._csr[0].tolist(), idx.shape[1])
            self.num_concepts = idx.shape[1]
        off, word, score = self._on(idx.device)
        return ops.senti_words_from_concepts(idx, off, word, score, self.max_list, n_out, pad_id)

    __call__ = forward


def tag_concepts(model, fc_store, num, batch=100, fns=None):
    """detect_concepts.py:32-43: {fn: [concept words, best first]} for every image of `fc_store` (any fn -> fc array
    mapping with keys(), or a path - see the Dataset classes), `batch` images per forward, ONE read-back per batch."""
    store = _store(fc_store)
    fns = list(store.keys()) if fns is None else list(fns)
    device = next(model.parameters()).device
    out = {}
    for i in range(0, len(fns), batch):
        cur = fns[i:i + batch]
        feats = _feats([_item(store[fn]) for fn in cur])
        feats = feats.to(device) if isinstance(feats, RowGather) else feats.to(device, non_blocking=True)
        _, concepts, _ = model.sample(feats, num)
        out.update(zip(cur, concepts))
    return out


def _image_items(images):
    """(name, uint8 array) pairs as they are; paths are decoded with PIL (RGBA and palette images become RGB, grey stays
    two-dimensional)."""
    for item in images:
        if isinstance(item, (str, os.PathLike)):
            from PIL import Image
            with Image.open(item) as im:
                if im.mode not in ('L', 'RGB'):
                    im = im.convert('RGB')
                yield os.path.basename(os.fspath(item)), np.asarray(im)
        else:
            name, array = item
            yield name, np.asarray(array)


def extract_features(encoder, images, out_dir, dtype=np.float32, att_size=14):
    """preprocess.py:23-46 (`extract_imgs_feat`) for this package: every image through `encoder` (encoder.Encoder, on
    whatever device it lives) into the two stores the datasets read - `<out_dir>/feats_fc.npy` [N, C] and
    `<out_dir>/feats_att.npy` [N, a, a, C] with their `.index.json` (FeatureStore), float32 or float16.  `images`: a
    sized collection (its len() gives N) of (name, uint8 array [H, W] / [H, W, 3] / [H, W, 4]) or of image paths; it may
    produce its items lazily.  Each image's features go straight into the memory-mapped files, as the reference writes
    per image: the host never holds more than one image's features.  Returns the two paths."""
    import json
    dtype = _feature_dtype(dtype)
    try:
        n = len(images)
    except TypeError:
        raise TypeError('extract_features: `images` must have a len() (the stores are allocated up front); pass a list '
                        'of paths or a sized dataset, not a generator')
    os.makedirs(out_dir, exist_ok=True)
    paths = (os.path.join(out_dir, 'feats_fc.npy'), os.path.join(out_dir, 'feats_att.npy'))
    names, maps = [], None
    encoder.eval()
    with torch.no_grad():
        for name, array in _image_items(images):
            if array.ndim == 3 and array.shape[-1] == 4:
                array = array[:, :, :3]
            if array.dtype != np.uint8:
                raise ValueError('extract_features: image %r is %s, not uint8' % (name, array.dtype))
            out = encoder.encode_uint8(array, att_size, want_f16=dtype == np.float16)
            feats = [t.cpu().numpy() for t in (out[2:] if dtype == np.float16 else out[:2])]
            if maps is None:                    # the first image gives the shapes
                maps = [np.lib.format.open_memmap(p, mode='w+', dtype=dtype, shape=(n,) + f.shape)
                        for p, f in zip(paths, feats)]
            if len(names) >= n:
                raise ValueError('extract_features: `images` produced more than its len() = %d items' % n)
            for m, f in zip(maps, feats):
                m[len(names)] = f
            names.append(name)
    if len(names) != n or len(set(names)) != n:
        raise ValueError('extract_features: %d items with %d distinct names from a collection of len() %d'
                         % (len(names), len(set(names)), n))
    for m, p in zip(maps or (), paths):
        m.flush()
        with open(p + '.index.json', 'w') as f:
            json.dump({fn: i for i, fn in enumerate(names)}, f)
    del maps
    return paths
