"""Checkpoint and result files in the reference's formats (SURVEY 5 "Checkpoint / resume", 8(f)-4).

The captioner's 40-tensor `state_dict` and FusedClampAdam's Adam-layout optimizer state make the
files interchangeable with the reference's:
  XE stage  train_xe.py:241-254  {epoch, model, optimizer, settings, idx2word, sentiment_categories,
                                   dataset_name, corpus_type};  resume checks train_xe.py:39-56
  RL stage  train_rl.py:311-325  {epoch, model (Detector state_dict: captioner.* / senti_detector.* /
                                   sent_senti_cls.*), settings, idx2word, max_seq_len, ...}
  results   train_xe.py:230-232  result_<epoch>.json [{image_id, caption}] + result_<epoch>.txt
"""
import json
import os
import time

import torch

_META = ('settings', 'idx2word', 'sentiment_categories', 'dataset_name', 'corpus_type')


def save_xe_checkpoint(directory, epoch, captioner, optimizer, settings, idx2word, sentiment_categories,
                       dataset_name, corpus_type, train_loss=0.0, val_loss=0.0):
    chk = {'epoch': epoch, 'model': captioner.state_dict(), 'optimizer': optimizer.state_dict(),
           'settings': settings, 'idx2word': idx2word, 'sentiment_categories': sentiment_categories,
           'dataset_name': dataset_name, 'corpus_type': corpus_type}
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, 'model_%d_%.4f_%.4f_%s.pth' % (epoch, train_loss, val_loss,
                                                                  time.strftime('%m%d-%H%M')))
    torch.save(chk, path)
    return path


def save_rl_checkpoint(directory, epoch, detector, settings, idx2word, max_seq_len, sentiment_categories,
                       dataset_name, corpus_type):
    chk = {'epoch': epoch, 'model': detector.state_dict(), 'settings': settings, 'idx2word': idx2word,
           'max_seq_len': max_seq_len, 'sentiment_categories': sentiment_categories,
           'dataset_name': dataset_name, 'corpus_type': corpus_type}
    words = getattr(detector, 'sentiment_words', None)
    if getattr(detector, 'senti_words_flag', 0) != 0 and isinstance(words, dict):
        # the sentiment-word reward is on: its (decayed) weights, so that a resumed run goes on with them; otherwise the
        # file is key for key the reference's
        chk['sentiment_words'] = {int(lab): {int(w): float(v) for w, v in ws.items()} for lab, ws in words.items()}
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, 'model_%d_%s.pth' % (epoch, time.strftime('%m%d-%H%M')))
    torch.save(chk, path)
    return path


def load_sentiment_words(path):
    """The lexicon weights an RL checkpoint carries ({label id: {word id: float}}: written while the sentiment-word
    reward was on) for Detector.set_sentiment_words, or None where the file has none."""
    chk = torch.load(path, map_location=lambda s, l: s, weights_only=False)
    return chk.get('sentiment_words')


def _check_meta(chk, expected):
    for key in _META:
        if key in expected and expected[key] != chk[key]:
            raise AssertionError('%s and resume model %s are different' % (key, key))


def load_xe_checkpoint(path, captioner, optimizer=None, **expected):
    """Resume as train_xe.py:39-56 does: metadata must match, then model (+ optimizer) state is loaded.
    Returns (epoch, lr)."""
    chk = torch.load(path, map_location=lambda s, l: s, weights_only=False)
    _check_meta(chk, expected)
    captioner.load_state_dict(chk['model'])
    lr = None
    if optimizer is not None and 'optimizer' in chk:
        optimizer.load_state_dict(chk['optimizer'])
        lr = optimizer.param_groups[0]['lr']
    return chk['epoch'], lr


def load_captioner_into_detector(path, detector, **expected):
    """RL warm start (train_rl.py:58-71): the XE checkpoint's `model` goes into `detector.captioner`."""
    chk = torch.load(path, map_location=lambda s, l: s, weights_only=False)
    _check_meta(chk, expected)
    detector.captioner.load_state_dict(chk['model'])
    return chk['epoch']


def write_results(result_dir, epoch, results):
    """results: [{'image_id': fn, 'caption': str}] -> result_<epoch>.json / .txt (train_xe.py:219-232)."""
    os.makedirs(result_dir, exist_ok=True)
    with open(os.path.join(result_dir, 'result_%d.json' % epoch), 'w') as f:
        json.dump(results, f)
    with open(os.path.join(result_dir, 'result_%d.txt' % epoch), 'w') as f:
        f.write(''.join(r['caption'] + '\n' for r in results))


def save_concept_checkpoint(directory, epoch, model, optimizer, settings, idx2concept, dataset_name, train_loss=0.0,
                            val_loss=0.0):
    """The concept detector's checkpoint as train_cpt.py:140-150 writes it: {epoch, model, optimizer, settings,
    idx2concept, dataset_name} under model_<epoch>_<train loss>_<val loss>_<time>.pth."""
    chk = {'epoch': epoch, 'model': model.state_dict(), 'optimizer': optimizer.state_dict(), 'settings': settings,
           'idx2concept': idx2concept, 'dataset_name': dataset_name}
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, 'model_%d_%.4f_%.4f_%s.pth' % (epoch, train_loss, val_loss,
                                                                  time.strftime('%m%d-%H%M')))
    torch.save(chk, path)
    return path


def load_concept_checkpoint(path, model=None, optimizer=None, **expected):
    """Resume as train_cpt.py:34-47 does (`expected`: settings / idx2concept / dataset_name must equal the file's), or -
    model=None - build the detector from the file as detect_concepts.py:15-23 / test_cpt.py:11-19 do.
    Returns (model, epoch, lr); lr is None without an optimizer."""
    chk = torch.load(path, map_location=lambda s, l: s, weights_only=False)
    for key in ('settings', 'idx2concept', 'dataset_name'):
        if key in expected and expected[key] != chk[key]:
            raise AssertionError('%s and resume model %s are different' % (key, key))
    if model is None:
        from .helper_nets import ConceptDetector
        model = ConceptDetector(chk['idx2concept'], chk['settings'])
    model.load_state_dict(chk['model'])
    lr = None
    if optimizer is not None and 'optimizer' in chk:
        optimizer.load_state_dict(chk['optimizer'])
        lr = optimizer.param_groups[0]['lr']
    return model, chk['epoch'], lr


_SENT_CLS_META = ('settings', 'idx2word', 'sentiment_categories', 'dataset_name', 'corpus_type')


def save_sent_cls_checkpoint(directory, epoch, model, optimizer, settings, idx2word, sentiment_categories, dataset_name,
                             corpus_type, train_loss=0.0, acc_rate=0.0):
    """The sentence-sentiment classifier's checkpoint as train_sent_senti_cls_rnn.py:178-190 writes it: {epoch, model,
    optimizer, settings, idx2word, sentiment_categories, dataset_name, corpus_type} under
    model_<epoch>_<train loss>_<accuracy>_<time>.pth."""
    chk = {'epoch': epoch, 'model': model.state_dict(), 'optimizer': optimizer.state_dict(), 'settings': settings,
           'idx2word': idx2word, 'sentiment_categories': sentiment_categories, 'dataset_name': dataset_name,
           'corpus_type': corpus_type}
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, 'model_%d_%.4f_%.4f_%s.pth' % (epoch, train_loss, acc_rate, time.strftime('%m%d-%H%M')))
    torch.save(chk, path)
    return path


def load_sent_cls_checkpoint(path, model=None, optimizer=None, **expected):
    """Resume as train_sent_senti_cls_rnn.py:42-59 does (`expected`: settings / idx2word / sentiment_categories /
    dataset_name / corpus_type must equal the file's - AssertionError with the reference's words otherwise, which name
    the settings `opt.settings`), or - model=None - build the classifier from the file.  Returns (model, epoch, lr); lr is
    None without an optimizer."""
    chk = torch.load(path, map_location=lambda s, l: s, weights_only=False)
    for key in _SENT_CLS_META:
        if key in expected and expected[key] != chk[key]:
            raise AssertionError('%s and resume model %s are different' % ('opt.settings' if key == 'settings' else key, key))
    if model is None:
        from .helper_nets import SentenceSentimentClassifier
        model = SentenceSentimentClassifier(chk['idx2word'], chk['sentiment_categories'], chk['settings'])
    model.load_state_dict(chk['model'])
    lr = None
    if optimizer is not None and 'optimizer' in chk:
        optimizer.load_state_dict(chk['optimizer'])
        lr = optimizer.param_groups[0]['lr']
    return model, chk['epoch'], lr


def save_senti_checkpoint(directory, epoch, model, optimizer, settings, sentiment_categories, train_loss=0.0, val_loss=0.0):
    """The image-sentiment detector's checkpoint as train_senti.py:119-128 writes it: {epoch, model, optimizer, settings,
    sentiment_categories} under model_<epoch>_<train loss>_<val loss>_<time>.pth."""
    chk = {'epoch': epoch, 'model': model.state_dict(), 'optimizer': optimizer.state_dict(), 'settings': settings,
           'sentiment_categories': sentiment_categories}
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, 'model_%d_%.4f_%.4f_%s.pth' % (epoch, train_loss, val_loss, time.strftime('%m%d-%H%M')))
    torch.save(chk, path)
    return path


def load_senti_checkpoint(path, model=None, optimizer=None, **expected):
    """Resume as train_senti.py:28-40 does (`expected`: settings / sentiment_categories must equal the file's), or -
    model=None - build the detector from the file.  Returns (model, epoch, lr); lr is None without an optimizer."""
    chk = torch.load(path, map_location=lambda s, l: s, weights_only=False)
    for key in ('settings', 'sentiment_categories'):
        if key in expected and expected[key] != chk[key]:
            raise AssertionError('%s and resume model %s are different' % ('opt.settings' if key == 'settings' else key, key))
    if model is None:
        from .helper_nets import SentimentDetector
        model = SentimentDetector(chk['sentiment_categories'], chk['settings'])
    model.load_state_dict(chk['model'])
    lr = None
    if optimizer is not None and 'optimizer' in chk:
        optimizer.load_state_dict(chk['optimizer'])
        lr = optimizer.param_groups[0]['lr']
    return model, chk['epoch'], lr
