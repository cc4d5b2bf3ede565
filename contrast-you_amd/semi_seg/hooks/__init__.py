from .autoencoder import AuxiliaryLayer, DenoisingAutoEncoderTrainerHook  # noqa: F401
from .consistency import ConsistencyTrainerHook  # noqa: F401
from .cc import CrossCorrelationOnLogitsHook  # noqa: F401
from .ccblock import ProjectorGeneralHook  # noqa: F401
from .creator import (create_consistency_hook, create_cross_correlation_hooks2, create_dae_hook,  # noqa: F401
                      create_differentiable_mt_hook, create_discrete_mi_consistency_hook, create_discrete_mi_hooks,
                      create_ent_min_hook, create_ict_hook, create_iid_seg_hook, create_iid_segmentation_hook,
                      create_imsat_hook, create_infonce_hooks, create_intermediate_imsat_hook, create_mixup_hook,
                      create_mt_hook, create_orthogonal_hook, create_pseudo_label_hook, create_sp_infonce_hooks,
                      create_superpixel_hooks, create_uamt_hook, feature_until_from_hooks, mt_in_hooks)
from .dmt import DifferentiableMeanTeacherTrainerHook  # noqa: F401
from .discretemi import DiscreteIMSATTrainHook, DiscreteMITrainHook  # noqa: F401
from .entmin import EntropyMinTrainerHook  # noqa: F401
from .infonce import (INFONCEHook, OnlineSuperPixelInfoNCEHook, PScheduler, SelfPacedINFONCEHook,  # noqa: F401
                      SuperPixelInfoNCEHook, region_extractor)
from .midl import IIDSegmentationTrainerHook, IMSATTrainHook  # noqa: F401
from .mixup import MixUpTrainHook  # noqa: F401
from .mt import (EMAUpdater, ICTMeanTeacherTrainerHook, MeanTeacherTrainerHook,  # noqa: F401
                 UAMeanTeacherTrainerHook)
from .orthogonal import OrthogonalTrainerHook  # noqa: F401
from .pseudolabel import PseudoLabelTrainerHook  # noqa: F401
