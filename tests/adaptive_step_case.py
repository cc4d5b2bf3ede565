"""Helper of tests/test_gpu_multicore_adaptive.py (not a test): training steps of a small multi-prototype U-Net under
`StricterAdaptiveOverSegmentedLoss`, the translation matrix T in a param group of its own, as `MulticoreTrainer` sets it
up.  `run_steps()` is called in the test's process; `python tests/adaptive_step_case.py <out.pt>` runs the same steps
in a fresh process under whatever CY_* switches the environment carries (cyhip.graphed reads CY_GRAPH_STEP at import)
and saves T."""
import random
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "contrast-you_amd", REPO / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

DEV = "cuda"
C_STEP, M_STEP = 4, 8
K_STEP = C_STEP * M_STEP
LR, WD = 1e-3, 1e-5
STEPS = 4  # eager probe step, captured step, two replayed steps


def step_batches():
    from test_gpu_hooks_dice import blob_batch
    g = torch.Generator().manual_seed(31)
    return blob_batch(2, 32, C_STEP, g), blob_batch(3, 32, C_STEP, g), blob_batch(2, 32, C_STEP, g, views=1)


def initial_state():
    from contrastyou.arch import UNet
    torch.manual_seed(11)
    return {k: v.clone() for k, v in UNet(input_dim=1, num_classes=K_STEP, max_channel=128).state_dict().items()}


def run_steps(steps: int = STEPS, graph=None) -> dict:
    """`graph`: HIP-graph replay of the network passes on / off (None: as the process started).
    -> {T: [T after 0, 1, ..., steps steps] (CPU), logits / labels: what the criterion saw in step 1, metrics: of
    the last step, replayed: the network passes ran from a captured graph, model, criterion}"""
    from contrastyou.hooks.base import TrainerHook
    from cyhip import graphed
    default = graphed.GRAPH_STEP
    if graph is not None:
        graphed.GRAPH_STEP = graph
    try:
        return _run_steps(steps)
    finally:
        graphed.GRAPH_STEP = default
        type(TrainerHook).names.clear()


def _run_steps(steps: int) -> dict:
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.multicore_loss import StricterAdaptiveOverSegmentedLoss
    from contrastyou.optim import RAdam
    from cyhip import graphed
    from semi_seg.epochers.features import MultiCoreTrainEpocher
    from semi_seg.hooks import create_consistency_hook
    from step_harness import OneBatchLoader
    type(TrainerHook).names.clear()
    lab, unl, _ = step_batches()
    model = UNet(input_dim=1, num_classes=K_STEP, max_channel=128)
    model.load_state_dict(initial_state())
    model.to(DEV)
    criterion = StricterAdaptiveOverSegmentedLoss(K_STEP, C_STEP, DEV)
    opt = RAdam([{"params": list(model.parameters())}], lr=LR, weight_decay=WD)
    opt.add_param_group({"params": list(criterion.parameters()), "lr": LR, "weight_decay": WD})  # MulticoreTrainer
    hook = create_consistency_hook(0.1)
    seen, T = {}, [criterion._translate_matrix.detach().cpu().clone()]
    inner = criterion.from_logits

    def spy(logits, labels):
        if "logits" not in seen:
            seen["logits"], seen["labels"] = logits.detach().float().cpu().clone(), labels.detach().cpu().clone()
        return inner(logits, labels)

    criterion.from_logits = spy
    random.seed(5)
    for e in range(steps):  # one step per epocher run, as tests/test_gpu_determinism.py drives its steps
        ep = MultiCoreTrainEpocher(model=model, optimizer=opt, labeled_loader=OneBatchLoader(lab),
                                   unlabeled_loader=OneBatchLoader(unl), sup_criterion=criterion, num_batches=1,
                                   cur_epoch=e, device=DEV, two_stage=True, disable_bn=False,
                                   scaler=torch.amp.GradScaler("cuda", enabled=False), accumulate_iter=1)
        ep.init()
        assert ep.num_classes == C_STEP
        with ep.register_hook(hook()):
            ep.run()
        torch.cuda.synchronize()
        T.append(criterion._translate_matrix.detach().cpu().clone())
        type(TrainerHook).names.clear()
    del criterion.from_logits
    replayed = any(isinstance(v, graphed.GraphedTwoPass) for v in model.__dict__.get("_cy_graphed", {}).values())
    return {"T": T, "logits": seen["logits"], "labels": seen["labels"], "metrics": ep.get_metric(),
            "replayed": replayed, "model": model, "criterion": criterion, "optimizer": opt}


if __name__ == "__main__":
    res = run_steps()
    torch.save({"T": res["T"], "replayed": res["replayed"]}, sys.argv[1])
