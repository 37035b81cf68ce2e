"""insenticap_model_amd - MI355X (gfx950) native caption-decoder hot path of InSentiCap.

    from insenticap_model_amd import Captioner, XECriterion, Detector, clip_gradient
"""
import os as _os

# Kernel arguments in device memory instead of host memory: the GEMM / step entry points take ~1 KB
# argument blocks whose first (dependent) scalar loads otherwise cross PCIe - measured 18.5 -> 11 us per
# small launch on MI355X.  Read by the HIP runtime when it initialises (first HIP call), so it has to be
# in the environment before then; an explicit user setting wins.
_os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')

from .captioner import Captioner, XECriterion  # noqa: F401,E402
from .detector import Detector  # noqa: F401,E402
from .optim import FusedClampAdam, clip_gradient  # noqa: F401,E402
from .helper_nets import ConceptDetector, MultiLabelClsLoss  # noqa: F401,E402
from .encoder import Encoder  # noqa: F401,E402
from .data import SentimentWordTable, tag_concepts  # noqa: F401,E402
from .train import concept_train_step  # noqa: F401,E402
from .rewards import RewardCriterion, get_ciderd_scorer, get_cls_reward, get_self_critical_reward  # noqa: F401,E402
from .rewards import get_group_self_critical_reward, group_self_critical_scores  # noqa: F401,E402
from .rewards import Bleu, DeviceBleu, get_bleu_scorer  # noqa: F401,E402
from .rewards import NgramLM, NgramLMSet, DeviceNgramLMSet, get_lm_reward, get_lm_reward_device, lm_perplexity  # noqa: F401,E402
from .rewards import SentimentWordWeights, get_senti_words_reward, senti_word_stats  # noqa: F401,E402

__all__ = ['SentimentWordWeights', 'get_senti_words_reward', 'senti_word_stats','Captioner', 'XECriterion', 'Detector', 'FusedClampAdam', 'clip_gradient', 'RewardCriterion',
           'get_ciderd_scorer', 'get_self_critical_reward', 'get_cls_reward', 'get_group_self_critical_reward',
           'group_self_critical_scores', 'Bleu', 'DeviceBleu', 'get_bleu_scorer', 'ConceptDetector', 'MultiLabelClsLoss',
           'SentimentWordTable', 'tag_concepts', 'concept_train_step', 'NgramLM', 'NgramLMSet', 'DeviceNgramLMSet',
           'get_lm_reward', 'get_lm_reward_device', 'lm_perplexity', 'Encoder']
