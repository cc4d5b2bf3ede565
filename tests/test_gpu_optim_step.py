"""FusedSGD, FusedAdam and FusedAdamW (contrastyou/optim) on the GPU: three-step trajectories against torch.optim on
the CPU, the checkpoint round trip, a move to the GPU after construction, the training step under `Optim.name` (HIP-graph
capture engaged, the flat-student EMA available) and one data-parallel case.

Trajectory bound (the rule of tests/optim_cases.py): per tensor, in 2-norm relative to the float64 trajectory, a fused
optimizer may be MARGIN = 4 times as far from torch.optim's f32 trajectory on the CPU as that trajectory is from
torch.optim's float64 one, floored at 2^-23.  Every figure is printed before it is asserted."""
import copy
import os
import random
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
from torch import nn

import optim_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = Path(__file__).resolve().parents[1]

# group 0: 3 and 7 x 5 elements; group 1: 33, a tensor without a gradient at step 1 ("late": its first update comes at
# step 2, between neighbours that are past theirs), a tensor without a gradient at step 2 ("skip") and 512 x 9.  The runs
# of group 1 start at element 0, 33, 38 and 44: 16-byte aligned and not.
SHAPES = {"a3": (3,), "b7x5": (7, 5), "c33": (33,), "late": (5,), "skip": (6,), "d512x9": (512, 9)}
GROUPS = (("a3", "b7x5"), ("c33", "late", "skip", "d512x9"))
NO_GRAD = {1: ("late",), 2: ("skip",), 3: ()}
STEPS = 3
LR_FACTOR = {1: 1.0, 2: 0.5, 3: 0.25}   # what a scheduler does between steps: param_group["lr"] is rewritten
HYPERS = {
    "SGD": (dict(lr=0.05, weight_decay=1e-4, momentum=0.9), dict(lr=0.02, weight_decay=0.0, momentum=0.9, nesterov=True)),
    "Adam": (dict(lr=1e-2, weight_decay=1e-4), dict(lr=3e-3, weight_decay=0.0, amsgrad=True)),
    "AdamW": (dict(lr=1e-2, weight_decay=1e-2), dict(lr=3e-3, weight_decay=0.1, betas=(0.8, 0.99))),
}
NAMES = tuple(HYPERS)


class Bag(nn.Module):
    def __init__(self, dtype=torch.float32):
        super().__init__()
        g = torch.Generator().manual_seed(17)
        self.p = nn.ParameterDict({k: nn.Parameter((torch.rand(*s, generator=g) * 2 - 1).to(dtype))
                                   for k, s in SHAPES.items()})
        g = torch.Generator().manual_seed(18)
        for k, s in SHAPES.items():
            self.register_buffer("t_" + k, (torch.rand(*s, generator=g) * 2 - 1).to(dtype))

    def loss(self, step: int):
        """a smooth loss whose gradient changes with the parameters; the tensors of NO_GRAD[step] take no part"""
        out = 0.0
        for i, k in enumerate(SHAPES):
            if k not in NO_GRAD[step]:
                d = self.p[k] - getattr(self, "t_" + k)
                out = out + ((0.5 + i) * d * d).sum() + (0.1 * step) * (d * d * d).sum()
        return out


def make_opt(factory, bag, hypers):
    return factory([dict(params=[bag.p[k] for k in names], **kw) for names, kw in zip(GROUPS, hypers)])


def run(opt, bag, name, first: int, last: int, each=None):
    """steps first..last of the trajectory; the lr of step s is the group's own times LR_FACTOR[s]"""
    for step in range(first, last + 1):
        for g, kw in zip(opt.param_groups, HYPERS[name]):
            g["lr"] = kw["lr"] * LR_FACTOR[step]
        opt.zero_grad(set_to_none=True)
        bag.loss(step).backward()
        opt.step()
        if each is not None:
            each(step)


def torch_trajectory(name, dtype):
    bag = Bag(dtype)
    opt = make_opt(lambda groups: getattr(torch.optim, name)(groups, foreach=False), bag, HYPERS[name])
    history = {}
    run(opt, bag, name, 1, STEPS, lambda step: history.__setitem__(step, {k: p.detach().clone() for k, p in bag.p.items()}))
    return history


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def fused(name):
    from contrastyou import optim
    return getattr(optim, name)


@pytest.mark.parametrize("name", NAMES)
def test_three_step_trajectory_against_torch(name):
    t32, t64 = torch_trajectory(name, torch.float32), torch_trajectory(name, torch.float64)
    bag = Bag().to(DEV)
    opt = make_opt(fused(name), bag, HYPERS[name])
    init = {k: p.detach().cpu().clone() for k, p in bag.p.items()}
    history, snapshot = {}, {}

    def each(step):
        history[step] = {k: p.detach().cpu().clone() for k, p in bag.p.items()}
        for k in SHAPES:
            ref = t64[step][k].double().norm().item()
            yard = (t32[step][k].double() - t64[step][k]).norm().item() / ref
            e = (history[step][k].double() - t32[step][k].double()).norm().item() / ref
            lim = max(oc.MARGIN * yard, oc.BOUND_FLOOR)
            print(f"Fused{name} step {step} {k}: {e:.3g} (<= {lim:.3g}; torch f32 against f64 {yard:.3g})")
            assert e <= lim, (name, step, k, e, lim)
        # per-parameter step counts: a parameter without a gradient stays behind, as torch's state["step"] does
        want = [[step - sum(k in NO_GRAD[s] for s in range(1, step + 1)) for k in names] for names in GROUPS]
        assert [opt._flat_state[i]["steps"] for i in range(2)] == want, (step, want)
        assert [opt._flat_state[i]["step"] for i in range(2)] == [step, step]
        if step == 1:
            snapshot["state"] = copy.deepcopy(opt.state_dict())
            snapshot["bag"] = copy.deepcopy({k: v.detach().cpu().clone() for k, v in bag.state_dict().items()})

    run(opt, bag, name, 1, STEPS, each)
    assert torch.equal(bits(history[1]["late"]), bits(init["late"])), "no gradient at step 1: not even weight decay"
    assert torch.equal(bits(history[2]["skip"]), bits(history[1]["skip"])), "no gradient at step 2: the bits stay"
    assert not torch.equal(bits(history[2]["late"]), bits(init["late"]))
    assert not torch.equal(bits(history[3]["skip"]), bits(history[2]["skip"]))
    for k in ("a3", "d512x9"):
        assert all(not torch.equal(bits(history[s][k]), bits(history[s + 1][k])) for s in (1, 2))
    flat = opt._flat[1]
    assert flat.offsets == [0, 33, 38, 44, 44 + 512 * 9] and bag.p["d512x9"].data_ptr() % 16 == 0
    assert bag.p["skip"].data_ptr() % 16 != 0   # the run that starts here (step 1) takes the one-float form

    # a checkpoint taken after step 1, loaded into a fresh optimizer over fresh parameters: the same bits from there on
    bag2 = Bag()
    bag2.load_state_dict(snapshot["bag"])
    bag2.to(DEV)
    opt2 = make_opt(fused(name), bag2, HYPERS[name])
    opt2.load_state_dict(snapshot["state"])
    assert opt2.state_dict()["flat"] is snapshot["state"]["flat"]   # pending until the flat buffers exist

    def same_bits(other, what):
        def each(step):
            for k, p in other.p.items():
                assert torch.equal(bits(p), bits(history[step][k])), f"{what} run differs at step {step}, {k}"
        return each

    run(opt2, bag2, name, 2, STEPS, same_bits(bag2, "resumed"))
    for i in range(2):
        assert opt2._flat_state[i]["steps"] == opt._flat_state[i]["steps"]
        assert list(opt2._flat_state[i]) == list(opt._flat_state[i])
        for k in opt._state_names(opt.param_groups[i]):
            assert torch.equal(bits(opt2._flat_state[i][k]), bits(opt._flat_state[i][k])), (i, k)

    # constructed on CPU parameters, flat buffers built there, THEN module.to("cuda"): rebuilt on the GPU, same bits
    bag3 = Bag()
    opt3 = make_opt(fused(name), bag3, HYPERS[name])
    opt3.zero_grad()
    assert opt3._flat[0].data.device.type == "cpu"
    bag3.to(DEV)
    run(opt3, bag3, name, 1, STEPS, same_bits(bag3, "moved"))
    assert opt3._flat[0].data.is_cuda and bag3.p["a3"].data_ptr() == opt3._flat[0].data.data_ptr()


def test_sgd_first_update_copies_the_gradient():
    """the update at a parameter's own step count 1 sets buf = g, whatever the dampening -- also when it comes late"""
    from contrastyou.optim import FusedSGD
    a, b = nn.Parameter(torch.ones(5, device=DEV)), nn.Parameter(torch.ones(7, device=DEV))
    opt = FusedSGD([a, b], lr=0.5, momentum=0.5, dampening=0.5)
    for step, params in ((1, (a,)), (2, (a, b))):
        opt.zero_grad()
        sum((p * 2.0).sum() for p in params).backward()
        opt.step()
    buf = opt._flat_state[0]["momentum_buffer"].cpu()
    assert torch.equal(buf[:5], torch.full((5,), 0.5 * 2.0 + 0.5 * 2.0))   # momentum buf + (1 - dampening) g
    assert torch.equal(buf[5:], torch.full((7,), 2.0))                      # b's first update: the copy
    assert torch.equal(b.detach().cpu(), torch.full((7,), 1.0 - 0.5 * 2.0))
    assert opt._flat_state[0]["steps"] == [2, 1]


# ---------------------------------------------------------------- the training step under Optim.name
@pytest.fixture(scope="module")
def step_data():
    from oracle import unet as ou
    from tests.test_gpu_hooks_dice import blob_batch
    g = torch.Generator().manual_seed(23)
    return (ou.init_state_dict(1, 4, 128, seed=15), [blob_batch(3, 32, 4, g) for _ in range(3)],
            [blob_batch(3, 32, 4, g) for _ in range(3)])


OPTIM_SPECS = {"SGD": dict(name="SGD", lr=1e-2, momentum=0.9, weight_decay=1e-5),
               "Adam": dict(name="Adam", lr=1e-3, weight_decay=1e-5),
               "AdamW": dict(name="AdamW", lr=1e-3, weight_decay=1e-2)}


def train_three_steps(spec, step_data, use_graph: bool):
    from contrastyou import optim
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.kl import KL_div
    from cyhip import graphed
    from semi_seg.epochers import SemiSupervisedEpocher
    from semi_seg.hooks import create_infonce_hooks
    from tests.test_gpu_hooks_dice import Loader
    sd0, lab, unl = step_data
    default = graphed.GRAPH_STEP
    graphed.GRAPH_STEP = use_graph
    try:
        type(TrainerHook).names.clear()
        model = UNet(input_dim=1, num_classes=4, max_channel=128, momentum=0.1)
        model.load_state_dict(sd0)
        model.to(DEV)
        torch.manual_seed(3)
        hook = create_infonce_hooks(model=model, feature_names="Conv5", weights=1.0, contrast_ons="partition",
                                    spatial_size=1, data_name="acdc").to(DEV)
        # Trainer._init_optimizer, line for line
        kwargs = {k: v for k, v in spec.items() if k != "name"}
        opt = getattr(optim, spec["name"])(params=[p for p in model.parameters() if p.requires_grad], **kwargs)
        opt.add_param_group(dict(params=list(hook.parameters()), **kwargs))
        ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=Loader(lab), unlabeled_loader=Loader(unl),
                                   sup_criterion=KL_div(), num_batches=3, cur_epoch=0, device=DEV, two_stage=True,
                                   disable_bn=False, scaler=torch.amp.GradScaler("cuda", enabled=False),
                                   accumulate_iter=1)
        ep.init()
        random.seed(9)
        with ep.register_hook(hook()):
            ep.run()
        torch.cuda.synchronize()
        return model, opt, ep.get_metric()
    finally:
        graphed.GRAPH_STEP = default
        type(TrainerHook).names.clear()


@pytest.mark.parametrize("name", NAMES)
def test_training_step_under_optim_name(name, step_data):
    import math
    from contrastyou.arch import UNet
    from contrastyou.optim import FlatOptimizer, FlatTeacher
    from cyhip import graphed
    model, opt, metric = train_three_steps(OPTIM_SPECS[name], step_data, use_graph=True)
    assert isinstance(opt, FlatOptimizer) and opt._flat_state[0]["step"] == 3
    assert math.isfinite(metric["semi"]["sup_loss"]) and math.isfinite(metric["semi"]["reg_loss"]), metric["semi"]
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    cache = model.__dict__.get("_cy_graphed", {})
    assert any(isinstance(v, graphed.GraphedTwoPass) for v in cache.values()), "the capture did not engage"
    eager, _, m_e = train_three_steps(OPTIM_SPECS[name], step_data, use_graph=False)
    assert not any(isinstance(v, graphed.GraphedTwoPass) for v in eager.__dict__.get("_cy_graphed", {}).values())
    for (k, a), b in zip(model.named_parameters(), eager.parameters()):
        assert torch.equal(bits(a), bits(b)), k   # same kernels in the same order on the same data
    moved = [not torch.equal(bits(p), bits(step_data[0][k])) for k, p in model.named_parameters()]
    assert sum(moved) > len(moved) // 2, "the optimizer moved the parameters"
    assert m_e["semi"]["sup_loss"] == metric["semi"]["sup_loss"]
    teacher = FlatTeacher(UNet(input_dim=1, num_classes=4, max_channel=128).to(DEV))
    assert teacher._student_is_flat([p.data for p in model.parameters()])


# ---------------------------------------------------------------- data parallel
DP_STEPS, DP_LR = 2, 0.05


def dp_model(seed):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(5, 7), nn.Tanh(), nn.Linear(7, 3))


def dp_batch(rank, step):
    g = torch.Generator().manual_seed(1000 + 10 * step + rank)
    return torch.randn(4, 5, generator=g), torch.randn(4, 3, generator=g)


def _dp_worker(rank, world, port, q):
    sys.path[:0] = [str(REPO), str(REPO / "contrast-you_amd")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from contrastyou.optim import FusedSGD
        net = dp_model(200 + rank).to("cuda:0")   # DIFFERENT initial weights per rank: rank 0's win
        opt = FusedSGD(net.parameters(), lr=DP_LR, momentum=0.9)
        assert opt._dp
        for step in range(DP_STEPS):
            x, y = (t.to("cuda:0") for t in dp_batch(rank, step))
            opt.zero_grad()
            (net(x) - y).pow(2).mean().backward()
            opt.step()
        torch.cuda.synchronize()
        assert opt.dp_steps == DP_STEPS and opt.dp_buckets == DP_STEPS
        q.put((rank, "ok", torch.cat([p.detach().reshape(-1).cpu() for p in net.parameters()]).numpy()))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, "".join(traceback.format_exception(type(e), e, e.__traceback__)), None))
    finally:
        dist.destroy_process_group()


def mean_gradient_sgd(dtype):
    """a single torch.optim.SGD on the CPU, fed the mean of the two ranks' gradients, from rank 0's initial weights"""
    net = dp_model(200).to(dtype)
    opt = torch.optim.SGD(net.parameters(), lr=DP_LR, momentum=0.9, foreach=False)
    for step in range(DP_STEPS):
        grads = []
        for rank in range(2):
            x, y = (t.to(dtype) for t in dp_batch(rank, step))
            grads.append(torch.autograd.grad((net(x) - y).pow(2).mean(), list(net.parameters())))
        for p, g0, g1 in zip(net.parameters(), *grads):
            p.grad = (g0 + g1) / 2
        opt.step()
    return [p.detach() for p in net.parameters()]


def test_two_rank_fused_sgd_keeps_replicas_identical():
    from tests.test_gpu_distributed import _spawn
    port = 33900 + (os.getpid() % 2000)
    results = _spawn(_dp_worker, lambda r, q: (r, 2, port, q))
    r0, r1 = torch.from_numpy(results[0]), torch.from_numpy(results[1])
    assert torch.equal(bits(r0), bits(r1)), "replicas diverged"
    t32, t64 = mean_gradient_sgd(torch.float32), mean_gradient_sgd(torch.float64)
    off = 0
    for i, (a, b) in enumerate(zip(t32, t64)):
        got = r0[off:off + a.numel()].view(a.shape).double()
        off += a.numel()
        ref = b.norm().item()
        yard = (a.double() - b).norm().item() / ref
        e, lim = (got - a.double()).norm().item() / ref, max(oc.MARGIN * yard, oc.BOUND_FLOOR)
        print(f"two-rank FusedSGD tensor {i}: {e:.3g} (<= {lim:.3g}; torch f32 against f64 {yard:.3g})")
        assert e <= lim, (i, e, lim)
    assert off == r0.numel()
