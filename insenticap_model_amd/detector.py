"""`Detector`: the RL-stage trainer wrapper of the reference (/root/reference/models/decoder.py:21-192)
on the MI355X path - same constructor, setters, `forward(data, data_type, training)` loss dictionary
and `sample(...)`.

One RL iteration = sampled roll-out (with REINFORCE gradients) + greedy roll-out (baseline) +
CIDEr-D and classifier rewards + XE pass (ss_prob 0.5) + seq2seq pass (ss_prob 0.25) + backward +
clamp(0.1) + Adam (decoder.py:65-167).  The decoder work runs on the HIP kernels through
`Captioner`; CIDEr-D runs in the native host library (or, `device_cider = True`, on the device in the
eager iterations: rewards.DeviceCiderD); the two frozen helper nets are stock PyTorch-ROCm modules
(helper_nets.py).

`rl_samples_per_image = n` > 1 (opt-in): n sampled captions per image from one grouped differentiable roll-out, the
baseline of a sample = the mean CIDEr-D of the image's other n - 1 samples (no greedy roll-out), the reward formed on
the device from the uploaded scores (isc_group_reward).
"""
from collections import defaultdict

import torch
import torch.nn as nn

from . import dp, ops
from .captioner import Captioner
from .helper_nets import SentenceSentimentClassifier, SentimentDetector
from .optim import clip_gradient
from .train import run_on_side_stream
from .ops import OutOfDomain
from .rewards import (CIDER_DEV_MAX_T, LM_DEV_MAX_T, Bleu, NgramLM, NgramLMSet, RewardCriterion, SentimentWordWeights,
                      get_bleu_scorer, get_ciderd_scorer, get_cls_reward, get_lm_reward, get_lm_reward_device,
                      get_self_critical_reward, get_self_critical_reward_device, get_senti_words_reward,
                      group_self_critical_scores, lm_perplexity)


def _helper_input(feats):
    """The stock-torch helper nets (fp32 parameters) read fp32: float16 features get an fp32 view at their call site."""
    return feats if feats.dtype == torch.float32 else feats.float()


class Detector(nn.Module):
    MAX_BATCHES_PER_CALL = 500      # decoder.py:65

    def __init__(self, idx2word, max_seq_len, sentiment_categories, lrs, settings):
        super().__init__()
        self.idx2word = idx2word
        self.pad_id = idx2word.index('<PAD>')
        self.max_seq_len = max_seq_len
        self.captioner = Captioner(idx2word, sentiment_categories, settings)
        self.senti_detector = SentimentDetector(sentiment_categories, settings)
        self.sent_senti_cls = SentenceSentimentClassifier(idx2word, sentiment_categories, settings)
        self.senti_detector.eval()
        self.sent_senti_cls.eval()
        self.cap_optim, self.cap_xe_crit, self.cap_da_crit = self.captioner.get_optim_criterion(lrs['cap_lr'])
        self.cap_rl_crit = RewardCriterion()
        self.cls_flag = 0.4
        self.seq_flag = 1.0
        self.senti_threshold = 0.7
        self.xe_ss_prob, self.seq2seq_ss_prob = 0.5, 0.25     # decoder.py:139,155 (hard-coded there)
        self.dp_arena, self.dp_group = None, None             # data-parallel training: enable_data_parallel()
        # The image sentiment detector is frozen (decoder.py:31,34: only captioner.parameters() are
        # optimised), so its label is a pure function of the image: cache it per file name instead of
        # re-running 1.7-9.2 GFLOP of convolutions per image in every RL iteration.
        self.cache_image_sentiments = True
        self._senti_cache, self._senti_cache_key = {}, None
        # 'fact' training iterations are served from HIP graphs (train_graph.RLTrainGraph: roll-outs / unrolls /
        # backward + update captured per batch geometry after two eager iterations; CIDEr-D and the classifier reward
        # between them).  False: every iteration runs the eager sequence below.
        self.train_graphs = True
        self._rl_graph = None
        # Token constraints of both roll-outs of an iteration (the sampled one and the greedy baseline): None, or a dict
        # of Captioner.forward_rl's keywords `suppress_special`, `decoding_constraint`, `min_len`.  While it is set every
        # iteration runs the eager sequence (capture under constraints is not built).
        self.rollout_constraints = None
        # Sampling controls of the TRAINING iterations' sampled roll-out: None, or a dict of Captioner.forward_rl's keywords
        # `temperature`, `top_k`, `top_p`.  A token drawn from the filtered distribution q is on-policy for q: while the
        # controls are on, the REINFORCE loss is taken on the SAMPLING log-probabilities log q(token) (differentiable:
        # isc_logsoftmax_bwd_raw_filtered), for n = 1 and for rl_samples_per_image > 1 alike; the greedy baseline and
        # evaluation are untouched, and the iteration runs the eager sequence (a graph-served filtered iteration is not
        # built).  None or all-default controls change nothing, graphs included.
        self.rollout_sampling = None
        # Sampled captions per image of a TRAINING iteration (1: the reference's iteration, sample + greedy baseline).
        # n > 1: self-critical RL on n samples per image whose baseline is the mean CIDEr-D of the image's other n - 1
        # samples - one grouped differentiable roll-out (Captioner.forward_rl captions_per_image=n: the image is not
        # repeated), no greedy roll-out, the reward built on the device from the uploaded scores (isc_group_reward).
        # Such iterations run the eager sequence; evaluation keeps the n = 1 path; not built under a process group.
        self.rl_samples_per_image = 1
        # True (opt-in): the iterations that run the eager sequence - evaluation, train_graphs = False, rollout_constraints,
        # rl_samples_per_image > 1, the exact-engine retry - take the fact reward from the device CIDEr-D scorer
        # (rewards.DeviceCiderD, isc_cider_dev_score): the token matrices are not copied to the host and the host scorer
        # is not called; grouped iterations hand the device scores straight to isc_group_reward.  The device twin of
        # `ciderd_scorer` is built on first use and rebuilt when set_ciderd_scorer replaces the host scorer; a vocabulary
        # above 65535 ids or max_seq_len > 63 warns once and keeps the host scorer.  With set_bleu_scorer the twin is a
        # rewards.DeviceBleu (isc_bleu_dev_score), everything else alike.  Graph-served iterations
        # (train_graph.RLTrainGraph) are untouched: they keep the host scorer, whose time they already hide under the
        # greedy roll-out and the XE graphs.
        self.device_cider = False
        self._cider_dev, self._cider_dev_warned = None, False
        # The reference's dormant LM reward (decoder.py:114-118, utils.py:86-100), opt-in: with lm_flag != 0 an n = 1
        # iteration adds lm_flag * get_lm_reward(...) to `rewards` - per row sign(score(greedy) - score(sample)) under the
        # n-gram model of the row's sentiment label (lm_reward_form 'sign', the reference's active line) or ppl(greedy) -
        # ppl(sample) ('ppl_diff', its commented alternative) - and logs 'lm_reward'.  Needs set_lms with the models; such
        # iterations run the eager sequence; with device_cider on the scores are formed on the device
        # (rewards.DeviceNgramLMSet, isc_lm_dev_score), otherwise by the host scorer.  0: nothing changes.
        self.lm_flag = 0.0
        self.lm_reward_form = 'sign'
        self._lms_dev, self._lms_dev_warned = None, False
        # The reference's dormant sentiment-word reward (decoder.py:120-126,174-176, utils.py:154-166), opt-in: with
        # senti_words_flag != 0 (the reference's commented value: 0.05) every iteration - 'fact' and 'senti', training and
        # evaluation, n = 1, grouped, constrained, filtered and graph-served - adds senti_words_flag * senti_words_reward
        # to `rewards` after the other terms and logs 'senti_words_reward' (a sum); at the end of the forward() call the
        # weights of the words that were paid are multiplied by senti_words_decay (1.0: no decay) and the caller's dict
        # (set_sentiment_words) is updated in place.  senti_words_form 'device': isc_sw_reward on the roll-out's token
        # matrix, the lexicon a rewards.SentimentWordWeights built lazily from the dict; 'host': the reference's function
        # on a host copy of the tokens - the yardstick, eager sequence only.  Not built under a process group.
        self.senti_words_flag = 0.0
        self.senti_words_decay = 0.9
        self.senti_words_form = 'device'
        self._sw_table = None

    def _device_sw(self, device):
        """The device table of `sentiment_words` (rewards.SentimentWordWeights): built on first use, rebuilt when
        set_sentiment_words replaced the dict object or the module moved."""
        words = self.__dict__.get('sentiment_words')
        twin = self._sw_table
        if twin is None or twin[0] is not words or twin[1] != device:
            n_labels = len(self.senti_detector.sentiment_categories)
            twin = self._sw_table = (words, device, SentimentWordWeights.from_dict(
                words, self.captioner.vocab_size, n_labels, device))
        return twin[2]

    def _device_ciderd(self, device, T):
        """The device twin of `ciderd_scorer` for rows of T tokens, or None: the flag is off, or this vocabulary / length
        is outside what the device scorer takes (warned once; the host scorer serves)."""
        if not self.device_cider or device.type != 'cuda':
            return None
        host = self.ciderd_scorer
        twin = self._cider_dev
        if twin is None or twin[0] is not host or twin[1] != device:
            try:
                twin = (host, device, host.to_device(device, self.captioner.vocab_size))
            except ValueError as e:
                twin = (host, device, None)
                self._warn_device_cider(str(e))
            self._cider_dev = twin
        if twin[2] is not None and T > CIDER_DEV_MAX_T:
            self._warn_device_cider('rows of %d tokens (the device scorer takes %d)' % (T, CIDER_DEV_MAX_T))
            return None
        return twin[2]

    def _warn_device_cider(self, why):
        if not self._cider_dev_warned:
            import warnings
            which = 'BLEU' if isinstance(self.ciderd_scorer, Bleu) else 'CIDEr-D'
            warnings.warn('device_cider: %s - the host %s scorer is used' % (why, which))
            self._cider_dev_warned = True

    @property
    def rl_samples_per_image(self):
        return self.__dict__.get('_rl_samples_per_image', 1)

    @rl_samples_per_image.setter
    def rl_samples_per_image(self, n):
        if isinstance(n, bool) or not hasattr(n, '__index__') or int(n) < 1:
            raise ValueError('rl_samples_per_image must be an integer >= 1, got %r' % (n,))
        self.__dict__['_rl_samples_per_image'] = int(n)

    @property
    def native_sentence_classifier(self):
        """True: the frozen sentence-sentiment classifier runs on the library's kernels (helper_nets.
        SentenceSentimentClassifier.native) - the classifier reward and both XE-label sites; default False: stock torch ops."""
        return bool(self.sent_senti_cls.native)

    @native_sentence_classifier.setter
    def native_sentence_classifier(self, on):
        self.sent_senti_cls.enable_native(on)

    @property
    def native_sentiment_detector(self):
        """True: the frozen image-sentiment detector runs on the library's kernels (helper_nets.SentimentDetector.native:
        implicit-GEMM convolutions on the split-f16 engine) and reads float16 features as they are - the image labels of an
        iteration and the label in front of `sample`'s beam search; default False: stock torch ops on an fp32 copy."""
        return bool(self.senti_detector.native)

    @native_sentiment_detector.setter
    def native_sentiment_detector(self, on):
        self.senti_detector.enable_native(on)

    def _detector_input(self, feats):
        """What the image detector is handed: with its native forward on, the features as they are (float16 rows are read
        natively; should the call fall to the torch code - exact-fp32 engine - the module up-casts them itself)."""
        return feats if self.senti_detector.native else _helper_input(feats)

    def enable_data_parallel(self, group=None, broadcast=True):
        """Data-parallel RL training over the ranks of `group` (default process group; backend nccl = RCCL over xGMI,
        gloo in tests).  The reference is single-device; under DP every rank runs `forward` on ITS shard of the fact /
        seq2seq batches (the caller shards the loaders), and the step becomes:
          * roll-outs, helper nets, CIDEr-D reward (document frequencies replicated) and classifier reward rank-local;
          * every loss term pre-scaled by local_count / global_count of ITS normaliser - RewardCriterion by the mask
            sum (utils.py:175), the two XECriterion terms by their token counts (captioner.py:438), the domain-align
            MSE by the row count - one 4-float all-reduce per iteration;
          * ONE sum-all-reduce of the flat 88 MB gradient arena between backward and the elementwise clamp
            (decoder.py:165-166: the clamp is nonlinear, it must see the reduced gradient), then identical
            clamp+Adam on every rank;
          * the returned dictionary holds global values (one all-reduce of the statistics per call)."""
        self.dp_group = group
        self.dp_arena = dp.GradArena(self.captioner.parameters())
        if broadcast:
            dp.broadcast_parameters(self.captioner, group=group)
        return self

    def set_ciderd_scorer(self, captions):
        self.ciderd_scorer = get_ciderd_scorer(captions, self.captioner.sos_id, self.captioner.eos_id)

    def set_bleu_scorer(self, order=4):
        """BLEU-`order` per sentence as the fact reward and metric instead of CIDEr-D (the reference's reward function
        takes either scorer through the same argument: utils.py:73-79, order 4 = its scores[3]).  The scorer is stored in
        `ciderd_scorer`, the attribute keeps its name; with device_cider on its device twin (rewards.DeviceBleu) is built."""
        self.ciderd_scorer = get_bleu_scorer(self.captioner.sos_id, self.captioner.eos_id, order)

    def set_sentiment_words(self, sentiment_words):
        self.sentiment_words = sentiment_words

    def set_lms(self, lms, eos_mode='word', unk_as_word=True):
        """The per-sentiment n-gram language models: {sentiment label: rewards.NgramLM or the path of an ARPA file over
        token ids (the reference's *_id.kenlm.arpa)} - labels 0 .. n - 1 - or a ready rewards.NgramLMSet.  Paths are read
        with the captioner's vocabulary; `eos_mode` / `unk_as_word` default to what the id files and KenLM imply.  Anything
        else is stored as it is (the reference's setter: decoder.py:52-53), and lm_flag != 0 then raises."""
        cap = self.captioner
        if isinstance(lms, dict) and lms and all(isinstance(v, (NgramLM, str)) or hasattr(v, '__fspath__')
                                                 for v in lms.values()):
            lms = NgramLMSet({k: v if isinstance(v, NgramLM) else NgramLM.from_arpa(str(v), cap.vocab_size)
                              for k, v in lms.items()}, cap.vocab_size, eos_mode, unk_as_word)
        if isinstance(lms, NgramLMSet):
            if lms.sos is None:
                lms.sos = cap.sos_id
            if lms.eos is None:
                lms.eos = cap.eos_id
        self.lms = lms
        self._lms_dev = None

    def _device_lms(self, device, T):
        """The device twin of `lms` for rows of T tokens, or None: device_cider is off, or the rows are longer than the
        device scorer takes (warned once; the host scorer serves)."""
        if not self.device_cider or device.type != 'cuda':
            return None
        if T > LM_DEV_MAX_T:
            if not self._lms_dev_warned:
                import warnings
                warnings.warn('device_cider: rows of %d tokens (the device LM scorer takes %d) - the host LM scorer is used'
                              % (T, LM_DEV_MAX_T))
                self._lms_dev_warned = True
            return None
        twin = self._lms_dev
        if twin is None or twin[0] is not self.lms or twin[1] != device:
            twin = self._lms_dev = (self.lms, device, self.lms.to_device(device))
        return twin[2]

    def caption_perplexity(self, token_rows, labels=None):
        """The corpus perplexity of caption rows under the models of `set_lms`: token_rows int [N, T] (ndarray or tensor,
        raw rows as the roll-outs and the result files hold them), labels [N] sentiment labels (None: model 0) ->
        rewards.lm_perplexity's dictionary {label: {'ppl', 'ppl1', 'logprob', 'sentences', 'words', 'oovs'}}.  Device rows
        are scored on the device where device_cider is on and they fit; the sums are taken on the host in float64."""
        lms = self.__dict__.get('lms')
        if not isinstance(lms, NgramLMSet):
            raise ValueError('Detector.caption_perplexity needs set_lms with n-gram language models')
        dev = None
        if torch.is_tensor(token_rows) and token_rows.is_cuda:
            dev = self._device_lms(token_rows.device, token_rows.shape[1])
        if dev is not None:
            lab = None if labels is None else torch.as_tensor(labels, dtype=torch.int64).to(token_rows.device)
            score, n_scored, n_oov = (x.cpu().numpy() for x in dev.score(token_rows.to(torch.int64), lab))
        else:
            score, n_scored, n_oov = lms.score(token_rows, labels)
        if torch.is_tensor(labels):
            labels = labels.cpu().numpy()
        return lm_perplexity(score, n_scored, n_oov, labels)

    def set_concept_detector(self, cd, senti_table=None, num_concepts=5, num_sentiments=10):
        """Gives the detector the pre-stage it lacked: a helper_nets.ConceptDetector (after `set_vocabulary`) and,
        optionally, a data.SentimentWordTable built with the detector's idx2concept.  With it, `tag` produces the
        cpts_tensor / sentis_tensor of images never seen before, `sample` derives the sentiment words of its image and
        `forward` tags a batch whose cpts_tensor / sentis_tensor is None.  The concept detector is frozen here and is NOT
        a registered submodule: state_dict and the RL checkpoint layout stay the reference's."""
        if cd is not None and cd._concept_word is None:
            raise ValueError('set_concept_detector: call ConceptDetector.set_vocabulary(word2idx) first')
        if senti_table is not None and senti_table.idx2concept is None:
            raise ValueError('set_concept_detector: the SentimentWordTable needs idx2concept')
        if cd is not None:
            cd.eval()
        self.__dict__['concept_detector'] = cd
        self.__dict__['senti_table'] = senti_table
        self.__dict__['num_concepts'], self.__dict__['num_sentiments'] = int(num_concepts), int(num_sentiments)
        return self

    @torch.no_grad()
    def tag(self, fc_feats):
        """fc_feats [B, F] on the device -> (cpts_tensor [B, num_concepts] int64 vocabulary ids of the detected concepts,
        sentis_tensor [B, num_sentiments] int64 ids of their sentiment words - None without a table), on the device,
        nothing read back: what the loaders take from img_det_concepts.json / img_det_sentiments.json."""
        cd = self.__dict__.get('concept_detector')
        if cd is None:
            raise ValueError('Detector.tag needs set_concept_detector')
        if next(cd.parameters()).device != fc_feats.device:
            cd.to(fc_feats.device)
        idx, _, words = cd.sample_device(fc_feats, self.num_concepts)
        table = self.__dict__.get('senti_table')
        sentis = table.forward(idx, self.num_sentiments, self.pad_id) if table is not None else None
        return words, sentis

    def forward(self, data, data_type, training):
        """data = (caption loader[, seq2seq loader]); data_type 'fact' | 'senti'. Returns the dict of
        loss sums divided by len(data) - the tuple length, as the reference does (decoder.py:178-179)."""
        if data_type not in ('fact', 'senti'):
            raise Exception('data_type(%s) is wrong!' % data_type)
        cap = self.captioner
        cap.train(training)
        # this call looks at the numerics flags at each iteration's own synchronisation point (below) instead of reducing
        # the features in front of every roll-out (Captioner._features_in_domain: a host read per new tensor)
        own_check, cap._domain_check_off = cap.__dict__.get('_domain_check_off'), True
        try:
            return self._forward(data, data_type, training)
        finally:
            cap._domain_check_off = own_check

    def _forward(self, data, data_type, training):
        cap = self.captioner
        # statistics stay on the device until the end of the call: every float(tensor) would stall the host
        # behind the whole queue (the reference reads them one by one, decoder.py:90-163)
        sums = defaultdict(float)

        def add(key, value):
            sums[key] = sums[key] + (value.detach() if torch.is_tensor(value) else value)

        device = next(self.parameters()).device
        rl_kw = dict(self.rollout_constraints or {})
        if set(rl_kw) - {'suppress_special', 'decoding_constraint', 'min_len'}:
            raise ValueError('rollout_constraints takes suppress_special / decoding_constraint / min_len, got %r'
                             % sorted(rl_kw))
        if not any(rl_kw.values()):
            rl_kw = {}                       # (all off: the unconstrained iteration, graphs included)
        rs_kw = dict(self.rollout_sampling or {})
        if set(rs_kw) - {'temperature', 'top_k', 'top_p'}:
            raise ValueError('rollout_sampling takes temperature / top_k / top_p, got %r' % sorted(rs_kw))
        tau, top_k, top_p = ops.check_sample_filter(rs_kw.get('temperature', 1.0), rs_kw.get('top_k', 0),
                                                    rs_kw.get('top_p', 1.0))
        if not training or (tau == 1.0 and not 0 < top_k < cap.vocab_size and top_p >= 1.0):
            rs_kw = {}                       # (all default: today's iteration, graphs included; evaluation: untouched)
        else:
            rs_kw = dict(temperature=tau, top_k=top_k, top_p=top_p, return_sampling_logprobs=True)
        # data-parallel branches: taken whenever DP is enabled and a process group exists - also a one-rank group
        # (shares are then exactly 1.0), so a one-GPU RCCL run crosses the code an 8-rank run does
        dist_on = self.dp_arena is not None and dp.distributed(self.dp_group)
        n_rl = self.rl_samples_per_image if training else 1      # (evaluation keeps the n = 1 path)
        lm_on = self.lm_flag != 0
        if lm_on and n_rl > 1:
            raise ValueError('lm_flag != 0 with rl_samples_per_image=%d: the LM reward compares a sample with the greedy '
                             'baseline, which a grouped iteration does not roll out' % n_rl)
        if lm_on and not isinstance(self.__dict__.get('lms'), NgramLMSet):
            raise ValueError('lm_flag != 0 needs set_lms with n-gram language models (rewards.NgramLMSet)')
        if n_rl > 1 and dist_on:
            raise ValueError('rl_samples_per_image=%d is not built for data-parallel training (a process group is '
                             'active): set it to 1' % n_rl)
        sw_on = self.senti_words_flag != 0
        sw_host = sw_on and self.senti_words_form == 'host'
        if sw_on and self.senti_words_form not in ('device', 'host'):
            raise ValueError("senti_words_form is 'device' or 'host', got %r" % (self.senti_words_form,))
        if sw_on and not isinstance(self.__dict__.get('sentiment_words'), dict):
            raise ValueError('senti_words_flag != 0 needs set_sentiment_words with the lexicon '
                             '{label id: {word id: weight}}')
        if sw_on and dist_on:
            raise ValueError('senti_words_flag != 0 is not built for data-parallel training (a process group is active): '
                             'the marks of the used words would have to be reduced across the ranks first')
        sw_table = self._device_sw(device) if sw_on and not sw_host else None
        accur_ws = defaultdict(set)                       # ('host' form: the words paid in this call, decoder.py:63)
        seq2seq_iter = iter(data[1]) if training else None
        caption_iter = iter(data[0])
        n_iter = min(self.MAX_BATCHES_PER_CALL, len(data[0]))
        if dist_on:
            # every iteration issues collectives: ranks whose loaders differ in length (or in data_type) would hang
            # inside RCCL - check once per call instead (shard with dp.shard(..., drop_last=True))
            dp.assert_same_across_ranks(n_iter * 4 + (2 if training else 0) + (data_type == 'fact'), device,
                                        self.dp_group, 'Detector.forward: iterations / data_type / training')
        for _ in range(n_iter):
            item = next(caption_iter)
            s2s_batch = None
            if training:                                  # fetched here (same loader order) so that its token
                try:                                      # count can ride in the iteration's one count all-reduce
                    s2s_batch = next(seq2seq_iter)
                except StopIteration:
                    seq2seq_iter = iter(data[1])
                    s2s_batch = next(seq2seq_iter)
            if data_type == 'fact':
                fns, fc_feats, att_feats, (caps_tensor, lengths), cpts_tensor, sentis_tensor, ground_truth = item
                caps_tensor = ops.to_device(caps_tensor, device)
            else:
                fns, fc_feats, att_feats, cpts_tensor, sentis_tensor, senti_labels = item
                senti_labels = ops.to_device(senti_labels, device)
            fc_feats, att_feats = ops.to_device(fc_feats, device), ops.to_device(att_feats, device)
            # (ops.to_device: through pinned memory, non-blocking - `x.to(device)` from pageable memory holds the host until the
            # stream gets there, i.e. until the previous iteration has finished)
            if cpts_tensor is None or sentis_tensor is None:
                # an untagged batch: concepts and sentiment words from the concept detector, on the device, ahead of the
                # iteration (graph-served or eager: both take the tensors as inputs, as before)
                t_cpts, t_sentis = self.tag(fc_feats)
                if sentis_tensor is None and t_sentis is None:
                    raise ValueError('Detector.forward: the batch carries no sentis_tensor and no SentimentWordTable is set')
                cpts_tensor = t_cpts if cpts_tensor is None else cpts_tensor
                sentis_tensor = t_sentis if sentis_tensor is None else sentis_tensor
            cpts_tensor, sentis_tensor = ops.to_device(cpts_tensor, device), ops.to_device(sentis_tensor, device)
            del item

            if data_type == 'fact' or not training:      # labels from the image sentiment detector
                senti_labels = self._image_sentiments(fns, att_feats)

            def run_iteration(exact, put):
                """One iteration (models/decoder.py:69-167).  `exact`: on the exact-fp32 GEMM engine, eagerly - the retry of
                an iteration whose roll-outs left the split-f16 operand domain (OutOfDomain is raised at the iteration's
                own synchronisation point, before anything is updated)."""
                if (training and self.train_graphs and not rl_kw and not rs_kw and n_rl == 1 and not lm_on
                        and not sw_host and device.type == 'cuda'
                        and ops.TIMER.arm_step is None and ops.graphs_allowed_here() and not exact):
                    # the same iteration from HIP graphs (train_graph.RLTrainGraph): same calls in the same order
                    from .train_graph import RLTrainGraph
                    g = self._rl_graph
                    if g is None or g.arena is not self.dp_arena or g.group is not self.dp_group or \
                            g.optim is not self.cap_optim or g.xe_crit is not self.cap_xe_crit or \
                            g.da_crit is not self.cap_da_crit:
                        # (the graph object holds its own references to the optimizer, the criteria, the arena and the
                        # group: a replaced optimizer - a new learning-rate schedule object, say - must not leave replays
                        # updating through the old one)
                        self._rl_graph = RLTrainGraph(self)
                    (s_caps, s_lengths), s_cpts, s_sentis, s_labels = s2s_batch
                    scs_dev = ((ops.to_device(s_caps, device), s_lengths), ops.to_device(s_cpts, device),
                               ops.to_device(s_sentis, device), ops.to_device(s_labels, device))
                    if data_type == 'fact':
                        def xe_senti_labels():
                            with torch.no_grad():
                                logits = self.sent_senti_cls(caps_tensor[:, 1:], lengths)[0]
                                return logits.softmax(dim=-1).argmax(dim=-1).detach()
                        if self.sent_senti_cls.training:     # (dropout draws: keep the reference's order of random numbers)
                            xe_senti_labels = xe_senti_labels()
                        # else: a callable - the graph object runs it behind its first roll-out, whose input it is not
                        stats = self._rl_graph.step(
                            (fns, fc_feats, att_feats, (caps_tensor, lengths), cpts_tensor, sentis_tensor, ground_truth),
                            scs_dev, senti_labels, xe_senti_labels)
                    else:                                    # 'senti': labelled images, no captions (decoder.py:75-78)
                        stats = self._rl_graph.step((fns, fc_feats, att_feats, cpts_tensor, sentis_tensor, senti_labels),
                                                    scs_dev, senti_labels)
                    for k, v in stats.items():
                        put(k, v)
                    return

                # sampled roll-out (graph kept in train mode) and the domain-alignment loss on its prologue
                # (grouped: n_rl rows per image, [I*n, T]; the prologue and its attributes stay per image, [I, E])
                grouped = n_rl > 1
                sampled = cap(
                    fc_feats, att_feats, cpts_tensor, sentis_tensor, senti_labels, self.max_seq_len,
                    sample_max=0, mode='rl', **(dict(captions_per_image=n_rl) if grouped else {}), **rl_kw, **rs_kw)
                sample_captions, sample_logprobs, seq_masks = sampled[:3]
                if rs_kw:           # drawn from q: the on-policy REINFORCE term is on log q(token), not on the model's log p
                    sample_logprobs = sampled[3]
                da_loss = self.cap_da_crit(cap.cpt_feats, cap.fc_feats.detach())
                # DP: each term's share of the global normaliser (mask sum, XE tokens, seq2seq tokens, rows)
                w_rl = w_xe = w_s2s = w_rows = None
                share = (lambda x, w: x * w) if dist_on else (lambda x, w: x)      # single process: graph untouched
                if dist_on:
                    n_local, n_global = dp.global_counts(
                        [seq_masks.sum(), float(sum(lengths)) if data_type == 'fact' else 0.0,
                         float(sum(s2s_batch[0][1])) if s2s_batch is not None else 0.0,
                         float(fc_feats.shape[0])], device, self.dp_group)
                    w_rl, w_xe, w_s2s, w_rows = (n_local / n_global.clamp_min(1.0)).unbind(0)
                da_loss = share(da_loss, w_rows)
                put('da_loss', da_loss)

                greedy_captions = greedy_masks = None
                if not grouped:                              # greedy baseline (grouped: the image's other samples are)
                    cap.eval()
                    with torch.no_grad():
                        greedy_captions, _, greedy_masks = cap(
                            fc_feats, att_feats, cpts_tensor, sentis_tensor, senti_labels, self.max_seq_len,
                            sample_max=1, mode='rl', **rl_kw)
                    cap.train(training)

                # The rewards need the token matrices on the host (CIDEr-D is host code).  Start their copies
                # now, enqueue the XE / seq2seq forward passes, and only then wait: the host scores the captions
                # while the device works through the two unrolls.  The order of the captioner calls - hence of
                # every random draw - is the reference's; only host-side waiting moved.
                # device_cider: CIDEr-D runs on the device instead (rewards.DeviceCiderD) - the token matrices stay where
                # they are; the batch's cooked references depend on no device result and are uploaded now, behind the
                # roll-outs already queued.  ('senti' has no CIDEr-D term: with the flag on nothing reads host tokens.)
                dev_cider = self._device_ciderd(device, sample_captions.shape[1]) if data_type == 'fact' else None
                host_tokens = dev_cider is None and not (self.device_cider and data_type != 'fact')
                # (the LM reward: on the device with device_cider where the rows fit, else from host tokens)
                dev_lms = self._device_lms(device, sample_captions.shape[1]) if lm_on else None
                host_tokens = host_tokens or (lm_on and dev_lms is None) or sw_host
                if dev_cider is not None:
                    ref_pack = dev_cider.pack_refs([ground_truth[fn] for fn in fns], keys=list(fns))
                if host_tokens:
                    host_sample = torch.empty(sample_captions.shape, dtype=sample_captions.dtype).pin_memory()
                    if not grouped:
                        host_greedy = torch.empty(greedy_captions.shape, dtype=greedy_captions.dtype).pin_memory()
                host_lens = torch.empty(seq_masks.shape[0], dtype=torch.int32).pin_memory()
                if host_tokens:
                    host_sample.copy_(sample_captions, non_blocking=True)
                    if not grouped:
                        host_greedy.copy_(greedy_captions, non_blocking=True)
                host_lens.copy_(seq_masks.sum(dim=-1).type(torch.int32), non_blocking=True)
                copied = torch.cuda.Event()
                copied.record()

                xe_loss = 0.0
                seq2seq_loss = 0.0
                from .autograd_pair import use_pair
                merged = data_type == 'fact' and training and device.type == 'cuda' and use_pair(cap, False)
                if merged:                                   # XE + seq2seq unrolls through one step chain (autograd_pair)
                    with torch.no_grad():
                        xe_senti_labels = self.sent_senti_cls(caps_tensor[:, 1:], lengths)[0]
                        xe_senti_labels = xe_senti_labels.softmax(dim=-1).argmax(dim=-1).detach()
                    (s_caps, s_lengths), s_cpts, s_sentis, s_labels = s2s_batch
                    s_caps, s_cpts = ops.to_device(s_caps, device), ops.to_device(s_cpts, device)
                    s_sentis, s_labels = ops.to_device(s_sentis, device), ops.to_device(s_labels, device)
                    with cap.token_logprobs():       # (log p(target) [B,T]: the [B,T,V] log-probs are never formed)
                        pred, pred2 = cap(fc_feats, att_feats, cpts_tensor, caps_tensor, xe_senti_labels, self.xe_ss_prob,
                                          s_caps, s_cpts, s_sentis, s_labels, self.seq2seq_ss_prob, mode='xe_seq2seq')
                    xe_loss = share(self.cap_xe_crit(pred, caps_tensor[:, 1:], lengths), w_xe)
                    put('xe_loss', xe_loss)
                    seq2seq_loss = share(self.seq_flag * self.cap_xe_crit(pred2, s_caps[:, 1:], s_lengths), w_s2s)
                    put('seq2seq_loss', seq2seq_loss)
                elif data_type == 'fact':                    # XE on the ground truth, labelled by the classifier
                    with torch.no_grad():
                        xe_senti_labels = self.sent_senti_cls(caps_tensor[:, 1:], lengths)[0]
                        xe_senti_labels = xe_senti_labels.softmax(dim=-1).argmax(dim=-1).detach()
                    with cap.token_logprobs():
                        pred = cap(fc_feats, att_feats, cpts_tensor, caps_tensor, xe_senti_labels,
                                   ss_prob=self.xe_ss_prob, mode='xe')
                    xe_loss = share(self.cap_xe_crit(pred, caps_tensor[:, 1:], lengths), w_xe)
                    put('xe_loss', xe_loss)

                if training and not merged:
                    (s_caps, s_lengths), s_cpts, s_sentis, s_labels = s2s_batch
                    s_caps, s_cpts = ops.to_device(s_caps, device), ops.to_device(s_cpts, device)
                    s_sentis, s_labels = ops.to_device(s_sentis, device), ops.to_device(s_labels, device)
                    def seq2seq_unroll():                     # 80 text-only rows: a chain of small launches that
                        with cap.token_logprobs():
                            pred = cap(s_caps, s_cpts, s_sentis, s_labels, ss_prob=self.seq2seq_ss_prob, mode='seq2seq')
                        return share(self.seq_flag * self.cap_xe_crit(pred, s_caps[:, 1:], s_lengths), w_s2s)
                    # ... overlaps with the XE unroll queued above when it runs on the side stream (forward and,
                    # through autograd, backward); same numbers either way
                    seq2seq_loss = run_on_side_stream(device, seq2seq_unroll) if device.type == 'cuda' \
                        else seq2seq_unroll()
                    put('seq2seq_loss', seq2seq_loss)

                copied.synchronize()
                if not exact and getattr(cap, 'numerics_checks', True) and ops.device_status(reset=True):
                    raise OutOfDomain()      # the roll-outs met non-finite values: nothing has been updated yet
                cls_reward = get_cls_reward(sample_captions, seq_masks, greedy_captions, greedy_masks,
                                            senti_labels.repeat_interleave(n_rl) if grouped else senti_labels,
                                            self.sent_senti_cls, sample_lens=host_lens.tolist(), on_device=True)
                if grouped:
                    # the I*n float64 CIDEr-D scores are all that is uploaded ('senti': zeros - the classifier term
                    # alone, as in the reference); baseline, advantage, the sum with the classifier term and the four
                    # logged means are formed on the device: isc_group_reward, two launches
                    if dev_cider is not None:            # (scored where the rows are: nothing is uploaded)
                        scores = dev_cider.score(sample_captions, ref_pack, row_div=n_rl)
                    elif data_type == 'fact':
                        scores = ops.upload(torch.from_numpy(group_self_critical_scores(
                            host_sample.numpy(), fns, ground_truth, self.ciderd_scorer, n_rl)), torch.float64, device)
                    else:
                        scores = torch.zeros(sample_captions.shape[0], dtype=torch.float64, device=device)
                    rewards, stats4 = ops.group_reward(scores, n_rl, cls_reward.float().contiguous(), self.cls_flag,
                                                       sample_captions.shape[1])
                    put('sample_score', stats4[0])
                    put('fact_reward', stats4[1])            # the mean advantage: 0 up to rounding by construction
                    put('cls_reward', stats4[2])
                    if not sw_on:                            # (else: from the final tensor, below)
                        put('all_rewards', stats4[3])
                elif dev_cider is not None:
                    fact_reward = get_self_critical_reward_device(sample_captions, greedy_captions, ref_pack, dev_cider)
                    put('fact_reward', share(fact_reward[:, 0].mean(), w_rows))
                elif data_type == 'fact':
                    fact_reward = get_self_critical_reward(
                        host_sample.numpy(), host_greedy.numpy(), fns, ground_truth, cap.sos_id, cap.eos_id,
                        self.ciderd_scorer)
                    fact_reward = ops.upload(fact_reward.astype('float32'), torch.float32, device)
                    put('fact_reward', share(fact_reward[:, 0].mean(), w_rows))
                else:
                    fact_reward = 0
                if not grouped:
                    put('cls_reward', share(cls_reward.mean(-1).mean(-1), w_rows))
                    rewards = fact_reward + self.cls_flag * cls_reward
                    if lm_on:
                        if dev_lms is not None:
                            lm_reward = get_lm_reward_device(sample_captions, greedy_captions, senti_labels, dev_lms,
                                                             self.lm_reward_form)
                        else:
                            lm_reward = get_lm_reward(host_sample.numpy(), host_greedy.numpy(), senti_labels, cap.sos_id,
                                                      cap.eos_id, self.lms, self.lm_reward_form)
                            lm_reward = ops.upload(lm_reward.astype('float32'), torch.float32, device)
                        put('lm_reward', lm_reward[:, 0].sum())      # (a sum, as decoder.py:118 logs it)
                        rewards = rewards + self.lm_flag * lm_reward
                if sw_on:
                    # the sentiment-word reward of the sampled rows (decoder.py:120-126), after the other terms; one torch
                    # expression on the device for both forms: the same bits
                    sw_labels = senti_labels.repeat_interleave(n_rl) if grouped else senti_labels
                    if sw_host:
                        sw_reward, accur_w = get_senti_words_reward(host_sample.numpy(), sw_labels.cpu().numpy(),
                                                                    self.sentiment_words)
                        for senti, words in accur_w.items():
                            accur_ws[senti].update(words)
                        sw_reward = ops.upload(torch.from_numpy(sw_reward).float(), torch.float32, device)
                    else:
                        sw_reward = sw_table.reward(sample_captions.contiguous(),
                                                    sw_labels.to(torch.int64).contiguous())
                    put('senti_words_reward', sw_reward.sum())       # (a sum, as decoder.py:124 logs it)
                    rewards = rewards + self.senti_words_flag * sw_reward
                    if grouped:                              # (isc_group_reward's mean was taken before this term)
                        put('all_rewards', rewards.mean(-1).mean(-1))
                if not grouped:
                    put('all_rewards', share(rewards.mean(-1).mean(-1), w_rows))
                cap_loss = share(self.cap_rl_crit(sample_logprobs, seq_masks, rewards), w_rl)
                put('cap_loss', cap_loss)

                total = cap_loss + xe_loss + da_loss + seq2seq_loss
                if training:
                    if self.dp_arena is not None:
                        self.dp_arena.zero_()
                    else:
                        self.cap_optim.zero_grad()
                    total.backward()
                    if self.dp_arena is not None:
                        self.dp_arena.all_reduce(self.dp_group)      # one 88 MB sum over xGMI, before the clamp
                    clip_gradient(self.cap_optim)            # 0.1, fused into the Adam launch
                    self.cap_optim.step()

            stats_it = []
            try:
                run_iteration(False, lambda k, v: stats_it.append((k, v)))
            except OutOfDomain:
                # features beyond |x| < 65504: the reference trains / evaluates on whatever its encoder produced
                # (models/decoder.py:86-98) - this iteration is redone on the exact-fp32 engine
                cap._warn_out_of_domain('non-finite values in a roll-out')
                del stats_it[:]
                with ops.exact_fp32_engine():
                    if self.senti_detector.native and (data_type == 'fact' or not training):
                        # the flagged batch's image labels came from the split-f16 convolutions (a non-finite logit
                        # reads `neutral`): recomputed here, on the torch path, they also replace what the label
                        # cache took from that batch
                        senti_labels = self._image_sentiments(fns, att_feats, refresh=True)
                    run_iteration(True, lambda k, v: stats_it.append((k, v)))
            for k, v in stats_it:
                add(k, v)

        if sw_on:
            # the words this call paid are paid less from now on (decoder.py:174-176: no `training` condition there)
            if sw_host:
                for senti, words in accur_ws.items():
                    for w in words:
                        self.sentiment_words[senti][w] *= self.senti_words_decay
                self._sw_table = None                    # (a device table of this dict is stale now)
            else:
                sw_table.decay(self.senti_words_decay)
                sw_table.update_dict(self.sentiment_words)       # (one small copy; the states are back to 1)

        if dist_on and sums:                             # global statistics: one small all-reduce per call
            keys = sorted(sums)                          # (same keys on every rank: data_type / training were checked)
            vec = torch.stack([torch.as_tensor(sums[k], dtype=torch.float32, device=device).reshape(()) for k in keys])
            dp.all_reduce_(vec, self.dp_group)
            sums = dict(zip(keys, vec.tolist()))
        if getattr(self.captioner, 'numerics_checks', True):
            ops.check_numerics('Detector.forward')       # (the statistics below are read by the host anyway)
        # len(data) is the length of the (loader, loader) TUPLE, as in the reference (decoder.py:178-179) - the same
        # on every rank, so globally summed statistics divide by the same number everywhere
        return {k: float(v) / len(data) for k, v in sums.items()}

    def invalidate_image_sentiments(self):
        """Forget the cached image-sentiment labels.  The cache is keyed by file name (+ the feature geometry, the
        threshold and the detector's weights): call this when the FEATURES behind a file name change - a second dataset
        that reuses names, features edited in place - or construct with cache_image_sentiments = False."""
        self._senti_cache, self._senti_cache_key = {}, None

    def _image_sentiments(self, fns, att_feats, refresh=False):
        """refresh: compute the labels anew and overwrite the cached ones (no cache hit is taken)."""
        if not self.cache_image_sentiments:
            return self.senti_detector.sample(self._detector_input(att_feats), self.senti_threshold)[0].detach()
        key = (self.senti_threshold, tuple(att_feats.shape[1:]), att_feats.dtype) + \
            tuple((q.data_ptr(), q._version) for q in self.senti_detector.parameters())
        if key != self._senti_cache_key:                 # weights reloaded / threshold changed
            self._senti_cache, self._senti_cache_key = {}, key
        cache = self._senti_cache
        if not refresh and all(fn in cache for fn in fns):
            return ops.upload([cache[fn] for fn in fns], torch.int64, att_feats.device)
        labels = self.senti_detector.sample(self._detector_input(att_feats), self.senti_threshold)[0].detach()
        for fn, lab in zip(fns, labels.tolist()):
            cache[fn] = lab
        return labels

    def sample(self, fc_feats, att_feats, sentis_tensor=None, beam_size=3, decoding_constraint=1, no_repeat_ngram=0,
               min_len=0, beam_groups=1, diversity=0.0):
        """One image: detect its sentiment, then beam search (decoder.py:182-192).  sentis_tensor=None: the image's
        sentiment words are derived on the device from its detected concepts (set_concept_detector with a table) and the
        search is queued behind them without a host read; without a table ValueError.  `no_repeat_ngram` / `min_len` /
        `beam_groups` / `diversity`: the beam search's controls (Captioner.sample_batch)."""
        self._check_groups(beam_size, beam_groups, diversity)
        self.eval()
        if sentis_tensor is None:
            if self.__dict__.get('concept_detector') is None or self.__dict__.get('senti_table') is None:
                raise ValueError('Detector.sample: sentis_tensor=None needs set_concept_detector with a SentimentWordTable')
            sentis_tensor = self.tag(fc_feats.reshape(1, -1))[1]
        att_feats = att_feats.unsqueeze(0)
        # the label stays on the device until the search is queued: the category name (a host read) is looked up behind the
        # search's own read-back instead of draining the device between the two (tools/eval_loop_probe.py)
        senti_label, _, _ = self.senti_detector.sample_device(self._detector_input(att_feats), self.senti_threshold)
        captions, _ = self.captioner.sample(fc_feats, att_feats, sentis_tensor, senti_label, beam_size,
                                            decoding_constraint, self.max_seq_len, no_repeat_ngram=no_repeat_ngram,
                                            min_len=min_len, beam_groups=beam_groups, diversity=diversity)
        return captions, self.senti_detector.names(senti_label)

    def _check_groups(self, beam_size, beam_groups, diversity):
        """`beam_groups` / `diversity` checked first thing, before the detector touches the device."""
        from .beam import check_groups
        return check_groups(self.captioner, beam_size, beam_groups, diversity)

    def sample_sentiments(self, fc_feats, att_feats, sentis_tensor=None, sentiments=None, beam_size=3,
                          decoding_constraint=1, no_repeat_ngram=0, min_len=0, beam_groups=1, diversity=0.0):
        """One image captioned under several sentiments at once: `sentiments` is a list of category names (default: all of
        the detector's sentiment_categories, in their order); the searches share the image's region tensors
        (Captioner.sample_sentiments).  The sentiment words are `sentis_tensor` or, when None, derived from the image's
        detected concepts as in `sample`; they are the image's and serve every sentiment.  Returns
        ({sentiment: captions}, detected) - `detected` is the image's own detected sentiment, as `sample` returns it.
        An unknown or repeated name, or an empty list, is a ValueError before anything touches the device."""
        self._check_groups(beam_size, beam_groups, diversity)
        cats = list(self.senti_detector.sentiment_categories)
        names = cats if sentiments is None else list(sentiments)
        if isinstance(sentiments, str) or not names:
            raise ValueError('Detector.sample_sentiments: sentiments must be a non-empty list of category names out of %r, '
                             'got %r' % (cats, sentiments))
        for s in names:
            if s not in cats:
                raise ValueError('Detector.sample_sentiments: %r is not one of the sentiment categories %r' % (s, cats))
        if len(set(names)) != len(names):
            raise ValueError('Detector.sample_sentiments: a sentiment is named twice in %r' % (names,))
        self.eval()
        if sentis_tensor is None:
            if self.__dict__.get('concept_detector') is None or self.__dict__.get('senti_table') is None:
                raise ValueError('Detector.sample_sentiments: sentis_tensor=None needs set_concept_detector with a '
                                 'SentimentWordTable')
            sentis_tensor = self.tag(fc_feats.reshape(1, -1))[1]
        att_feats = att_feats.unsqueeze(0)
        detected, _, _ = self.senti_detector.sample_device(self._detector_input(att_feats), self.senti_threshold)
        labels = ops.upload([[cats.index(s) for s in names]], torch.int64, fc_feats.device)       # [1, S]
        captions, _, _ = self.captioner.sample_sentiments(fc_feats.reshape(1, -1), att_feats, sentis_tensor.reshape(1, -1),
                                                          labels, beam_size, decoding_constraint, self.max_seq_len,
                                                          _labels_known=True, no_repeat_ngram=no_repeat_ngram,
                                                          min_len=min_len, beam_groups=beam_groups, diversity=diversity)
        return dict(zip(names, captions[0])), self.senti_detector.names(detected)

    def set_encoder(self, enc):
        """The image encoder (encoder.Encoder) behind sample_image; kept outside the module tree, as the concept detector
        is: the encoder is frozen and has its own checkpoint."""
        self.__dict__['encoder'] = enc
        return self

    def sample_image(self, image, beam_size=3, decoding_constraint=1, att_size=14, sentiments=None, no_repeat_ngram=0,
                     min_len=0, beam_groups=1, diversity=0.0):
        """One image from its pixels: uint8 [H, W, 3] / [H, W] as decoded (the normalisation is fused into the encoder's
        first kernel) or a `preprocess`ed fp32 tensor [3, H, W] -> encoder -> sample(fc, att).  The sentiment words come
        from the concept detector (set_concept_detector with a table); no host read between the encoder and the search.
        `sentiments` (a list of category names): the image is captioned under each of them instead of under its detected
        sentiment - `sample_sentiments(fc, att, None, sentiments)`, which returns ({sentiment: captions}, detected)."""
        self._check_groups(beam_size, beam_groups, diversity)
        enc = self.__dict__.get('encoder')
        if enc is None:
            raise ValueError('Detector.sample_image needs set_encoder')
        with torch.no_grad():
            if torch.is_tensor(image) and image.is_floating_point():
                fc, att = enc(image.to(enc.resnet.conv1.weight.device), att_size)
            else:
                fc, att = enc.encode_uint8(image, att_size)
        if sentiments is not None:
            return self.sample_sentiments(fc, att, None, sentiments, beam_size, decoding_constraint, no_repeat_ngram,
                                          min_len, beam_groups, diversity)
        return self.sample(fc, att, None, beam_size, decoding_constraint, no_repeat_ngram, min_len, beam_groups, diversity)
