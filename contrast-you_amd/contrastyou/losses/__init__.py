from .contrastive import SelfPacedSupConLoss, SupConLoss1, is_normalized  # noqa: F401
from .redundancy_reduction import RedundancyCriterion  # noqa: F401
from .discreteMI import IIDLoss, IIDSegmentationLoss, IIDSegmentationSmallPathLoss, patch_generator  # noqa: F401
from .kl import KL_div, Entropy, JSD_div, EntropyPrior  # noqa: F401
from .pica_loss import PUILoss, PUISegLoss  # noqa: F401
from .dice_loss import BinaryDiceLoss, DiceLoss, make_one_hot  # noqa: F401
from .multicore_loss import GeneralOverSegmentedLoss, MultiCoreKL  # noqa: F401
from .multicore_loss import AdaptiveOverSegmentedLoss, GradientReverse, scale_grad  # noqa: F401
from .multicore_loss import StricterAdaptiveOverSegmentedLoss, StricterAdaptiveOverSegmentedLossWithMI  # noqa: F401
