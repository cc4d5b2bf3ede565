"""hook factories (semi_seg/hooks/creator.py:31-281 of the reference).  Every name the reference's `hook_creator.py`
imports from `semi_seg.hooks` exists here; the methods this project has not built are stubs with the reference's
signature that raise NotImplementedError when called."""
from __future__ import annotations

from typing import Any, Dict, List, Sequence, Union

from torch import nn

from contrastyou.arch._base import sort_arch
from contrastyou.hooks.base import CombineTrainerHook, TrainerHook
from contrastyou.utils.utils import ntuple

from .cc import CrossCorrelationOnLogitsHook
from .ccblock import (ProjectorGeneralHook, _CenterCompactnessHook, _ConsistencyHook, _CrossCorrelationHook,
                      _IMSATHook, _MIHook, _RedundancyReduction)
from .consistency import ConsistencyTrainerHook
from .discretemi import DiscreteMITrainHook, decoder_names
from .entmin import EntropyMinTrainerHook
from .infonce import INFONCEHook, SelfPacedINFONCEHook, SuperPixelInfoNCEHook
from .midl import IIDSegmentationTrainerHook
from .mt import MeanTeacherTrainerHook, UAMeanTeacherTrainerHook
from .pseudolabel import PseudoLabelTrainerHook


def get_individual_hook(*hooks):
    for h in hooks:
        assert isinstance(h, TrainerHook)
        if isinstance(h, CombineTrainerHook):
            yield from get_individual_hook(*h._hooks)  # noqa
        else:
            yield h


def mt_in_hooks(*hooks) -> bool:
    return any(isinstance(h, MeanTeacherTrainerHook) for h in get_individual_hook(*hooks))


def feature_until_from_hooks(*hooks, model) -> Union[str, None]:
    names = [h._feature_name for h in get_individual_hook(*hooks) if hasattr(h, "_feature_name")]
    if names:
        return sort_arch(names, model=model)[-1]
    return model.arch_elements[-1]


def create_consistency_hook(weight: float):
    return ConsistencyTrainerHook(name="consistency", weight=weight)


def create_mt_hook(*, model: nn.Module, weight: float, alpha: float = 0.999, weight_decay: float = 1e-5,
                   update_bn: bool = False, num_teachers: int = 1, hard_clip: bool = False):
    """config/hooks/mt.yaml (creator.py:147-151)"""
    return MeanTeacherTrainerHook(name="mt", model=model, weight=weight, alpha=alpha, weight_decay=weight_decay,
                                  update_bn=update_bn, num_teachers=num_teachers, hard_clip=hard_clip)


def create_uamt_hook(*, model: nn.Module, weight: float, alpha: float = 0.999, weight_decay: float = 1e-5,
                     update_bn: bool = False, num_teachers: int = 1, hard_clip: bool = False):
    """config/hooks/uamt.yaml (creator.py:154-158; the reference names this hook "mt" as well)"""
    return UAMeanTeacherTrainerHook(name="mt", model=model, weight=weight, alpha=alpha, weight_decay=weight_decay,
                                    update_bn=update_bn, num_teachers=num_teachers, hard_clip=hard_clip)


def create_ent_min_hook(*, weight: float = 0.001):
    """config/hooks/entmin.yaml (creator.py:170-172)"""
    return EntropyMinTrainerHook(name="entropy", weight=weight)


def create_pseudo_label_hook(*, weight: float):
    """config/hooks/pseudolabel.yaml (creator.py:188-189)"""
    return PseudoLabelTrainerHook(weight=weight, name="plab")


def _infonce_hook(*, model: nn.Module, feature_name: str, weight: float, contrast_on: str, data_name: str,
                  spatial_size: int, global_negatives: bool = False):
    return INFONCEHook(name=f"infonce/{feature_name}/{contrast_on}", model=model, feature_name=feature_name,
                       weight=weight, data_name=data_name, contrast_on=contrast_on,
                       spatial_size=(spatial_size, spatial_size), global_negatives=global_negatives)


def create_infonce_hooks(*, model: nn.Module, feature_names: Union[str, List[str]],
                         weights: Union[float, List[float]], contrast_ons: Union[str, List[str]],
                         spatial_size: Union[int, Sequence[int]] = 1, data_name: str,
                         global_negatives: bool = False):
    n = 1 if isinstance(feature_names, str) else len(feature_names)
    rep = ntuple(n)
    hooks = [_infonce_hook(model=model, feature_name=f, weight=w, contrast_on=c, data_name=data_name,
                           spatial_size=ss, global_negatives=global_negatives)
             for f, w, c, ss in zip(rep(feature_names), rep(weights), rep(contrast_ons), rep(spatial_size))]
    return CombineTrainerHook(*hooks)


def _infonce_sp_hook(*, model: nn.Module, feature_name: str, weight: float, contrast_on: str, data_name: str,
                     begin_value: float = 1e6, end_value: float = 1e6, max_epoch: int, mode: str = "soft", p=0.5,
                     correct_grad=False, global_negatives: bool = False):
    return SelfPacedINFONCEHook(name=f"spinfoce/{feature_name}/{contrast_on}", model=model, feature_name=feature_name,
                                weight=weight, data_name=data_name, contrast_on=contrast_on, mode=mode, p=p,
                                begin_value=begin_value, end_value=end_value, max_epoch=max_epoch,
                                correct_grad=correct_grad, global_negatives=global_negatives)


def create_sp_infonce_hooks(*, model: nn.Module, feature_names: Union[str, List[str]],
                            weights: Union[float, List[float]], contrast_ons: Union[str, List[str]], data_name: str,
                            begin_values: Union[float, List[float]] = 1e10,
                            end_values: Union[float, List[float]] = 1e10, mode: str, p=0.5, max_epoch: int,
                            correct_grad: Union[bool, List[bool]] = False, global_negatives: bool = False):
    """one SelfPacedINFONCEHook per feature (creator.py:122-145)"""
    n = 1 if isinstance(feature_names, str) else len(feature_names)
    rep = ntuple(n)
    hooks = [_infonce_sp_hook(model=model, feature_name=f, weight=w, contrast_on=c, data_name=data_name,
                              begin_value=b, end_value=e, max_epoch=max_epoch, mode=mode, p=p, correct_grad=g,
                              global_negatives=global_negatives)
             for f, w, c, b, e, g in zip(rep(feature_names), rep(weights), rep(contrast_ons), rep(begin_values),
                                         rep(end_values), rep(correct_grad))]
    return CombineTrainerHook(*hooks)


def _create_superpixel_hook(*, model: nn.Module, feature_name: str, weight: float, data_name: str,
                            spatial_size: int):
    return SuperPixelInfoNCEHook(name=f"infonce/{feature_name}/superpixel", model=model, feature_name=feature_name,
                                 weight=weight, data_name=data_name, contrast_on="self",
                                 spatial_size=(spatial_size, spatial_size))


def create_superpixel_hooks(*, model: nn.Module, feature_names: Union[str, List[str]],
                            weights: Union[float, List[float]], spatial_size: Union[int, Sequence[int]],
                            data_name: str):
    """creator.py:263-281"""
    n = 1 if isinstance(feature_names, str) else len(feature_names)
    rep = ntuple(n)
    hooks = [_create_superpixel_hook(model=model, feature_name=f, weight=w, data_name=data_name, spatial_size=ss)
             for f, w, ss in zip(rep(feature_names), rep(weights), rep(spatial_size))]
    return CombineTrainerHook(*hooks)


def create_discrete_mi_hooks(*, feature_names: List[str], weights: List[float], paddings: List[int],
                             model: nn.Module):
    """one DiscreteMITrainHook per feature; `paddings` lists the displacement radius of the DECODER
    features only, in order (creator.py:56-67)"""
    assert len(feature_names) == len(weights), (feature_names, weights)
    decoder_features = [f for f in feature_names if f in decoder_names]
    assert len(paddings) == len(decoder_features), (decoder_features, paddings)
    pad_gen = iter(paddings)
    paddings_ = [next(pad_gen) if f in decoder_features else None for f in feature_names]
    hooks = [DiscreteMITrainHook(name=f"discreteMI/{f.lower()}", model=model, feature_name=f, weight=w, padding=p)
             for f, w, p in zip(feature_names, weights, paddings_)]
    return CombineTrainerHook(*hooks)


def create_discrete_mi_consistency_hook(*, model: nn.Module, feature_names: Union[str, List[str]],
                                        mi_weights: Union[float, List[float]], dense_paddings: List[int] = None,
                                        consistency_weight: float):
    """config/hooks/udaiic.yaml: IIC on feature maps + output consistency (creator.py:76-90)"""
    n = 1 if isinstance(feature_names, str) else len(feature_names)
    feature_names = ntuple(n)(feature_names)
    mi_weights = ntuple(n)(mi_weights)
    n_dense = len([f for f in feature_names if f in decoder_names])
    dense_paddings = ntuple(n_dense)(dense_paddings) if n_dense else ()
    mi = create_discrete_mi_hooks(feature_names=list(feature_names), weights=list(mi_weights),
                                  paddings=list(dense_paddings), model=model)
    return CombineTrainerHook(mi, create_consistency_hook(weight=consistency_weight))


def create_iid_segmentation_hook(*, weight: float, mi_lambda: float = 1.0):
    """config/hooks/iid.yaml: IIC between the two views' segmentation outputs"""
    return IIDSegmentationTrainerHook(hook_name="midl_hook", weight=weight, mi_lambda=mi_lambda)


def create_iid_seg_hook(*, weight: float = 0.001, mi_lambda=1.0):
    """the reference's name and hook name for `create_iid_segmentation_hook` (creator.py:184-185)"""
    return IIDSegmentationTrainerHook(hook_name="iid", weight=weight, mi_lambda=mi_lambda)


def _not_built(method: str, factory: str):
    raise NotImplementedError(f"{factory}: {method} is not implemented in this project (DESIGN.md, out of scope)")


def create_differentiable_mt_hook(*, model: nn.Module, weight: float, alpha: float = 0.999,
                                  weight_decay: float = 0.000001, meta_weight=0, meta_criterion: str,
                                  method_name: str):
    _not_built("the differentiable mean teacher (semi_seg/hooks/dmt.py)", "create_differentiable_mt_hook")


def create_orthogonal_hook(*, weight: float = 0.001, model: nn.Module):
    _not_built("the orthogonal-prototype regulariser (semi_seg/hooks/orthogonal.py)", "create_orthogonal_hook")


def create_imsat_hook(*, weight: float = 0.1):
    _not_built("IMSAT on the segmentation output (semi_seg/hooks/midl.py)", "create_imsat_hook")


def create_intermediate_imsat_hook(*, feature_name: str, weight: float, num_clusters: int, cons_weight: float,
                                   model: nn.Module):
    _not_built("IMSAT on a feature map (semi_seg/hooks/discretemi.py)", "create_intermediate_imsat_hook")


def create_mixup_hook(*, weight: float, enable_bn: bool):
    _not_built("MixUp (semi_seg/hooks/mixup.py)", "create_mixup_hook")


def create_ict_hook(*, weight: float, alpha: float, weight_decay: float, update_bn: bool, model):
    _not_built("interpolation consistency training (semi_seg/hooks/mt.py)", "create_ict_hook")


def create_dae_hook(*, weight: float, num_classes: int):
    _not_built("the denoising auto-encoder prior (semi_seg/hooks/autoencoder.py)", "create_dae_hook")


def create_cross_correlation_hooks2(*, model: nn.Module, feature_name: str, num_clusters: int, head_type: str,
                                    num_subheads: int, save: bool = True, hook_params: Dict[str, Any]):
    """config section CrossCorrelationParameters (creator.py:196-239): on a feature map, a projector with the tiny
    hooks named by the keys of `hook_params`; on "Deconv_1x1", the on-logits hook"""
    project_params = {"num_clusters": num_clusters, "head_type": head_type, "normalize": False,
                      "num_subheads": num_subheads, "hidden_dim": 64}
    if "Deconv_1x1" != feature_name:
        hook = ProjectorGeneralHook(name=f"cc_{feature_name}", model=model, feature_name=feature_name,
                                    projector_params=project_params, save=save)
        for key, tiny in (("mi", _MIHook), ("cc", _CrossCorrelationHook), ("compact", _CenterCompactnessHook),
                          ("rr", _RedundancyReduction), ("imsat", _IMSATHook), ("consist", _ConsistencyHook)):
            if key in hook_params:
                hook.register_dist_hook(tiny(**hook_params[key]))
    else:
        mi_params = {"lamda": hook_params["mi"]["lamda"], "padding": hook_params["mi"]["padding"]}
        norm_params = {"power": hook_params["cc"]["diff_power"]}
        hook = CrossCorrelationOnLogitsHook(
            name=f"cc_{feature_name}", cc_weight=hook_params["cc"]["weight"], feature_name=feature_name,
            kernel_size=hook_params["cc"]["kernel_size"], projector_params=project_params, model=model,
            mi_weight=hook_params["mi"]["weight"], save=save, mi_criterion_params=mi_params, norm_params=norm_params)
    return CombineTrainerHook(hook)
