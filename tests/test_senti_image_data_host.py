"""The image-sentiment detector's data path on the CPU: data.SentiImageDataset, senti_image_collate_fn (also as
create_collate_fn('senti_image')) and get_senti_image_dataloader (reference dataloader.py:117-121, 248-260, 349-357) over
a dict, a FeatureStore file in fp32 and float16, and a device-resident store's row handles; and that a RowGather batch is
what train.senti_det_loss_with_grad accepts up to its shape check."""
import numpy as np
import pytest
import torch

from insenticap_model_amd import data

FNS = ['img_%d.jpg' % i for i in range(7)]
RNG = np.random.default_rng(12)
ATT = RNG.standard_normal((7, 2, 3, 32)).astype(np.float32)
LABELS = [[fn, int(l)] for fn, l in zip(FNS, RNG.integers(0, 3, 7))]        # train_senti.py:48-54: [fn, label index]


def _check_batches(loader, dtype, order=None):
    seen = 0
    for fns, att, labels in loader:
        B = len(fns)
        assert isinstance(fns, tuple) and tuple(att.shape) == (B, 2, 3, 32) and att.dtype == dtype
        assert labels.dtype == torch.int64 and tuple(labels.shape) == (B,)
        for fn, a, l in zip(fns, att, labels):
            i = FNS.index(fn)
            assert int(l) == LABELS[i][1]
            assert torch.equal(a, torch.from_numpy(ATT[i]).to(dtype))
            if order is not None:
                assert i == order[seen]
            seen += 1
    assert seen == 7


def test_loader_over_a_mapping_keeps_order_shapes_and_dtypes():
    loader = data.get_senti_image_dataloader(dict(zip(FNS, ATT)), LABELS, batch_size=3, shuffle=False)
    assert len(loader) == 3                                    # 3 + 3 + 1
    _check_batches(loader, torch.float32, order=list(range(7)))
    # shuffled: every image once, labels still with their images
    torch.manual_seed(1)
    _check_batches(data.get_senti_image_dataloader(dict(zip(FNS, ATT)), LABELS, batch_size=4), torch.float32)


@pytest.mark.parametrize('dtype', [np.float32, np.float16], ids=['fp32', 'f16'])
def test_loader_over_a_feature_store_file(tmp_path, dtype):
    path = data.FeatureStore.write(str(tmp_path / 'att.npy'), FNS, ATT, dtype=dtype)
    loader = data.get_senti_image_dataloader(path, LABELS, batch_size=4, shuffle=False)
    want = torch.float16 if dtype == np.float16 else torch.float32
    seen = 0
    for fns, att, labels in loader:                            # float16 items stay float16; values are the store's
        assert att.dtype == want and labels.dtype == torch.int64
        for fn, a in zip(fns, att):
            assert torch.equal(a, torch.from_numpy(ATT[FNS.index(fn)].astype(dtype)))
            seen += 1
    assert seen == 7


def test_mixed_items_collate_to_fp32_and_the_named_collate_is_the_same_function():
    items = [(FNS[0], ATT[0].astype(np.float16), 2), (FNS[1], ATT[1], 0)]
    fns, att, labels = data.create_collate_fn('senti_image')(items)
    assert data.create_collate_fn('senti_image') is data.senti_image_collate_fn
    assert fns == (FNS[0], FNS[1]) and att.dtype == torch.float32 and labels.tolist() == [2, 0]
    assert torch.equal(att[0], torch.from_numpy(ATT[0].astype(np.float16).astype(np.float32)))


def test_dataset_items_are_copies_with_the_label_index():
    store = dict(zip(FNS, ATT))
    ds = data.SentiImageDataset(store, LABELS)
    assert len(ds) == 7
    fn, att, label = ds[4]
    assert fn == FNS[4] and label == LABELS[4][1] and isinstance(att, np.ndarray) and att.dtype == np.float32
    att[:] = 0
    assert store[FNS[4]].any()                                 # the store's array is untouched


def test_device_resident_store_gives_a_row_gather_that_expands_to_the_batch():
    store = data.DeviceFeatureStore({fn: i for i, fn in enumerate(FNS)}, torch.from_numpy(ATT))     # (a host tensor here)
    loader = data.get_senti_image_dataloader(store, LABELS, batch_size=4, shuffle=False)
    fns, att, labels = next(iter(loader))
    assert isinstance(att, data.RowGather) and att.shape == (4, 2, 3, 32)
    assert torch.equal(att.dense(), torch.from_numpy(ATT[:4])) and labels.tolist() == [l for _, l in LABELS[:4]]
    # ... and the training entry point expands it before it looks at its shape: what it refuses here is the device
    from insenticap_model_amd.helper_nets import SentimentDetector
    from insenticap_model_amd import synth
    from insenticap_model_amd.train import senti_det_loss_with_grad
    st = dict(synth.TINY_SETTINGS, **synth.HELPER_SETTINGS)
    st.update(fc_feat_dim=32, sentiment_convs_num=1, sentiment_fcs_num=1, dropout_p=0.0)
    m = SentimentDetector(synth.SENTIMENT_CATEGORIES, st)
    with pytest.raises(Exception) as err:
        senti_det_loss_with_grad(m, att, labels)
    assert not isinstance(err.value, AttributeError), err.value
