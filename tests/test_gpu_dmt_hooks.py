"""The differentiable-mean-teacher hooks on the GPU.
    (a) the build's hooks on the stand-in model for three steps against the reference's own float64 trajectory
        (tests/golden/dmt.npz), every method and both meta criteria;
    (b) the eval-mode backward of the HIP U-Net against the float64 oracle with pinned routing;
    (c) the fused hooks against a plain composition (tests/dmt_cases.PlainDMTHook) inside real SemiSupervisedEpocher
        steps with the HIP U-Net as teacher, eager and with the student's passes replayed from HIP graphs;
    (d) methods 2 and 4 differentiate a teacher pass between the student's forward and backward: the student's
        gradients are those of the same step with a stub hook that returns the same loss from recorded teacher logits;
    (e) one epoch through SemiTrainer: meter names, checkpoint round trip of the teacher;
    (f) one bf16-autocast step of method 4.

Bounds.  (a): four times the distance of the reference's own f32 run from its f64 run (recorded next to the trajectory),
a loss floored at 1.2e-6.  (b), (d): GRAD_TOL of tests/test_gpu_unet.py, the suite's bar for the f32 backward arithmetic
of this network.  (c): eager and replayed steps report the same numbers (what tests/test_gpu_criteria.py asks of that
comparison); fused against plain, both sides run the same network kernels and differ in the loss kernels, the Adam
kernel and the order of sums, so the bar is again GRAD_TOL, on the losses and on every tensor of the teacher's state
relative to its largest element.  (f): as (c) for the losses; see the test for the state.  Every figure is printed
before it is asserted."""
import copy
import random

import numpy as np
import pytest
import torch

import dmt_cases as dc
from test_gpu_hooks_dice import Loader, blob_batch
from test_gpu_unet import GRAD_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
K, HW, MAXC = 4, 32, 128


@pytest.fixture(scope="module")
def npz(golden_dir):
    return dc.load(golden_dir)


# ---------------------------------------------------------------- (a) against the reference's trajectory
@pytest.mark.parametrize("crit", dc.CRITERIA)
@pytest.mark.parametrize("method", dc.METHODS)
def test_hooks_follow_the_reference_for_three_steps(npz, method, crit):
    from semi_seg.hooks import DifferentiableMeanTeacherTrainerHook
    tag, h = f"{method}_{crit}", dc.HOOK
    student = dc.new_student(torch.float32, DEV)
    hook = DifferentiableMeanTeacherTrainerHook(
        name=f"dmt_{tag}", model=student, weight=h["weight"], alpha=h["alpha"], weight_decay=h["weight_decay"],
        meta_weight=h["meta_weight"], meta_criterion=crit, method_name=method)
    assert not hook._needs_init  # the construction-time pass ran (on a random image of its own: the state is set below)
    init = {k[len(tag) + 6:]: torch.from_numpy(v) for k, v in npz.items() if k.startswith(f"{tag}_init_")}
    got = dc.drive(hook, student, torch.float32, DEV, teacher_state=init)
    e_ref = npz[f"{tag}_e_ref"]
    lims = (dc.bound(e_ref[0], loss=True), dc.bound(e_ref[1], loss=True), dc.bound(e_ref[2]))
    teacher = hook.flat_teacher
    lo = teacher.flat.data.data_ptr()
    assert all(lo <= p.data_ptr() < lo + 4 * teacher.flat.numel for p in hook.teacher_model.parameters())
    for step, (loss, meters, state, counters) in enumerate(got):
        e = [dc.rel_scalar(loss, npz[f"{tag}_loss"][step]),
             max(dc.rel_scalar(v, npz[f"{tag}_meter_{m}"][step]) for m, v in meters.items()),
             dc.rel_max(state, torch.from_numpy(npz[f"{tag}_state"][step]))]
        print(f"{tag} step {step}: loss {e[0]:.3g} (<= {lims[0]:.3g})  meters {e[1]:.3g} (<= {lims[1]:.3g})  "
              f"teacher state {e[2]:.3g} (<= {lims[2]:.3g})")
        assert sorted(meters) == sorted(k[len(tag) + 7:] for k in npz if k.startswith(f"{tag}_meter_"))
        assert counters == list(npz[f"{tag}_counters"][step])
        assert all(x <= lim for x, lim in zip(e, lims)), (tag, step, e, lims)


def test_mt_update_alone_with_the_students_gradient(npz):
    from semi_seg.hooks import DifferentiableMeanTeacherTrainerHook
    student = dc.new_student(torch.float32, DEV)
    hook = DifferentiableMeanTeacherTrainerHook(name="dmt_update", model=student, weight=1.0, meta_criterion="ce",
                                                method_name="mt")()
    li, lt, ui, m = dc.hook_data(0)
    ui, m = ui.float().to(DEV), m.to(DEV)
    z = student(dc.warp_by_map(ui, m)).detach().requires_grad_(True)
    loss = hook.mt_update(unlabeled_tf_logits=z, unlabeled_image=ui, affine_transformer=lambda x: dc.warp_by_map(x, m))
    loss.backward()
    e_ref = npz["update_e_ref"]
    e = [dc.rel_scalar(loss.detach(), npz["update_loss"]), *dc.rel_grad(z.grad, torch.from_numpy(npz["update_grad"]))]
    lims = [dc.bound(e_ref[0], loss=True), dc.bound(e_ref[1]), dc.bound(e_ref[2])]
    print("mt_update: loss %.3g (<= %.3g)  grad2 %.3g (<= %.3g)  gradmax %.3g (<= %.3g)"
          % tuple(v for pair in zip(e, lims) for v in pair))
    assert all(x <= lim for x, lim in zip(e, lims)), (e, lims)


# ---------------------------------------------------------------- (b) eval-mode backward of the HIP U-Net
def test_eval_mode_gradients_match_oracle_with_pinned_routing():
    """BatchNorm in eval mode: the running statistics normalise, and the backward pass has no batch-statistics terms"""
    from contrastyou.arch import UNet
    from cyhip.functions import SoftmaxKLFn
    from oracle import losses as ol
    from oracle import unet as ou
    from step_harness import RawTaps, rel
    sd = ou.init_state_dict(1, K, MAXC, seed=21)
    g = torch.Generator().manual_seed(52)
    x = torch.rand(2, 1, HW, HW, generator=g)
    tgt = torch.randint(0, K, (2, HW, HW), generator=g)
    net = UNet(input_dim=1, num_classes=K, max_channel=MAXC, momentum=0.5)
    net.load_state_dict(sd, strict=True)
    net.to(DEV).train()
    with torch.no_grad():  # running statistics that are not the initial (0, 1)
        net(torch.rand(2, 1, HW, HW, generator=g).to(DEV))
    sd_eval = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    assert float(sd_eval["_Conv1.conv.1.running_mean"].abs().max()) > 0
    net.eval()
    for p in net.parameters():
        p.grad = None
    with RawTaps(net) as taps:
        out = net(x.to(DEV))
    loss = SoftmaxKLFn.apply(out, tgt.to(DEV), 1e-16)
    loss.backward()
    after = net.state_dict()
    assert all(torch.equal(after[k].cpu(), v) for k, v in sd_eval.items() if "running" in k or "tracked" in k)
    with torch.no_grad():
        free = ou.unet_forward(ou.clone_state_dict(sd_eval, dtype=torch.float64), x.double(), training=False)
    sd64 = ou.clone_state_dict(sd_eval, requires_grad=True, dtype=torch.float64)
    ref = ou.unet_forward(sd64, x.double(), training=False, force=taps.force)
    ol.sup_loss(ref, tgt).backward()
    e_out = rel(out, free)
    e_grad = {n: rel(p.grad, sd64[n].grad) for n, p in net.named_parameters()}
    worst = max(e_grad, key=e_grad.get)
    print(f"eval-mode U-Net: logits {e_out:.3g} (< 1e-4), worst gradient {worst} {e_grad[worst]:.3g} (< {GRAD_TOL})")
    assert e_out < 1e-4
    assert e_grad[worst] < GRAD_TOL, (worst, e_grad[worst])


# ---------------------------------------------------------------- (c), (d), (f): real epocher steps
class _Adapter:
    """makes an EpocherHook of a dmt_cases.PlainDMTHook / of any object with the three callbacks"""

    @staticmethod
    def wrap(inner, name):
        from contrastyou.hooks.base import EpocherHook

        class Hook(EpocherHook):
            def _call_implementation(self, **kw):
                return inner(**kw)

            def before_regularization(self, **kw):
                kw.pop("result_dict", None)
                return inner.before_regularization(**kw)

            def after_batch_update(self, **kw):
                kw.pop("result_dict", None)
                return inner.after_batch_update(**kw)

        return Hook(name=name)


class _Recorder:
    """stands in for SoftmaxGatherMSEFn inside semi_seg.hooks.dmt: keeps what the hook handed to it"""

    def __init__(self, real):
        self.real, self.seen = real, []

    def apply(self, teacher_logits, source_map, student_logits):
        self.seen.append((teacher_logits.detach().clone(), source_map.clone()))
        return self.real.apply(teacher_logits, source_map, student_logits)


class _Stub:
    """returns the recorded step's loss from the recorded teacher logits: no teacher pass at all"""

    def __init__(self, seen, weight):
        self.seen, self.weight, self.i = seen, weight, 0

    def before_regularization(self, **kw):
        pass

    def after_batch_update(self, **kw):
        pass

    def __call__(self, *, unlabeled_tf_logits, **kw):
        from cyhip.functions import SoftmaxGatherMSEFn
        teacher_logits, source_map = self.seen[self.i]
        self.i += 1
        return self.weight * SoftmaxGatherMSEFn.apply(teacher_logits, source_map, unlabeled_tf_logits)


WEIGHT, META_WEIGHT = 0.5, 1e-3


def run_steps(method, kind, graph, *, bf16=False, steps=2, seen=None, monkeypatch=None):
    """`steps` steps of a SemiSupervisedEpocher (2 + 2 images of 32 x 32, K = 4, the 128-channel HIP U-Net, RAdam) under
    one hook: kind "fused" (the build's), "plain" (dmt_cases.PlainDMTHook) or "stub" (the losses of `seen`).
    -> dict(meters, state = teacher state dict on the CPU, grad = the student's flat gradient after the last step,
    params = the student's flat parameters, seen, replayed)"""
    from contrastyou.amp import BF16Scaler
    from contrastyou.arch import UNet
    from contrastyou.losses.kl import KL_div
    from contrastyou.optim import RAdam
    from cyhip import graphed
    from cyhip.functions import bump_weights_epoch
    from oracle import unet as ou
    from semi_seg.epochers import SemiSupervisedEpocher
    from semi_seg.hooks import DifferentiableMeanTeacherTrainerHook, EMAUpdater
    from semi_seg.hooks import dmt as dmt_mod
    default = graphed.GRAPH_STEP
    graphed.GRAPH_STEP = graph
    try:
        g = torch.Generator().manual_seed(33)
        lab = [blob_batch(2, HW, K, g) for _ in range(steps)]
        unl = [blob_batch(2, HW, K, g) for _ in range(steps)]
        model = UNet(input_dim=1, num_classes=K, max_channel=MAXC, momentum=0.1)
        sd0 = ou.init_state_dict(1, K, MAXC, seed=14)
        model.load_state_dict(sd0)
        model.to(DEV)
        recorder, teacher_model, inner = None, None, None
        if kind == "fused":
            trainer_hook = DifferentiableMeanTeacherTrainerHook(
                name="dmt", model=model, weight=WEIGHT, meta_weight=META_WEIGHT, meta_criterion="ce",
                method_name=method)
            teacher_model = trainer_hook.teacher_model
            teacher_model.load_state_dict(model.state_dict())  # (the construction-time pass moved its statistics)
            recorder = _Recorder(dmt_mod.SoftmaxGatherMSEFn)
            monkeypatch.setattr(dmt_mod, "SoftmaxGatherMSEFn", recorder)
            ep_hook = trainer_hook()
        elif kind == "plain":
            teacher_model = copy.deepcopy(model)
            inner = dc.PlainDMTHook(method=method, model=model, teacher=teacher_model,
                                    updater=EMAUpdater(update_bn=True), criterion=KL_div(), weight=WEIGHT,
                                    meta_weight=META_WEIGHT, weights_changed=bump_weights_epoch)
            ep_hook = _Adapter.wrap(inner, "dmt")
        else:
            ep_hook = _Adapter.wrap(_Stub(seen, WEIGHT), "dmt")
        opt = RAdam(list(model.parameters()), lr=1e-3, weight_decay=1e-5)
        scaler = BF16Scaler() if bf16 else torch.amp.GradScaler("cuda", enabled=False)
        ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=Loader(lab), unlabeled_loader=Loader(unl),
                                   sup_criterion=KL_div(), num_batches=steps, cur_epoch=0, device=torch.device(DEV),
                                   two_stage=True, disable_bn=False, scaler=scaler, accumulate_iter=1)
        ep.init()
        random.seed(9)
        with ep.register_hook(ep_hook):
            ep.run()
        torch.cuda.synchronize()
        metrics = ep.get_metric()
        if kind == "plain":
            hook_meters = {k: float(torch.stack([torch.as_tensor(x).float().cpu() for x in v]).mean())
                           for k, v in inner.meters.items() if v}
        else:
            hook_meters = dict(metrics.get("dmt", {}))
        flat = opt._flat[0]
        adam_in = None   # the gradient the last Adam step was handed, one flat vector
        if kind == "fused" and method in ("method1", "method4"):
            adam_in = trainer_hook.flat_teacher.flat.grad.detach().cpu().clone()
        elif kind == "plain" and method in ("method1", "method4"):
            adam_in = torch.cat([g.reshape(-1) for g in inner.last_grads]).cpu()
        return dict(semi=metrics["semi"], meters=hook_meters, adam_in=adam_in,
                    state=None if teacher_model is None else {k: v.detach().cpu().clone()
                                                              for k, v in teacher_model.state_dict().items()},
                    grad=flat.grad.detach().cpu().clone(), params=flat.data.detach().cpu().clone(),
                    offsets=list(flat.offsets), names=[n for n, _ in model.named_parameters()],
                    seen=None if recorder is None else recorder.seen,
                    replayed=any(isinstance(v, graphed.GraphedTwoPass)
                                 for v in model.__dict__.get("_cy_graphed", {}).values()))
    finally:
        graphed.GRAPH_STEP = default


def state_errors(got, ref, two_norm_for=()):
    """{tensor: max |got - ref| / max |ref|} over the floating tensors (for the names in `two_norm_for` the 2-norm of
    the difference relative to the 2-norm of ref); the counters must be equal"""
    out = {}
    for k, v in ref.items():
        if not v.is_floating_point():
            assert torch.equal(got[k], v), k
        elif k in two_norm_for:
            out[k] = dc.rel_grad(got[k], v)[0]
        else:
            out[k] = dc.rel_max(got[k], v)
    return out


ADAM_STEP_MAX = 1.0015  # |update| / lr of one Adam step at t <= 2, see `adam_moved`


def adam_moved(method, state):
    """the tensors whose final value went through Adam's division: every parameter under method 1 (method 4 puts the
    teacher back before its EMA, so nothing Adam wrote stays).  Adam divides each gradient element by its own size, so an
    element whose gradient is smaller than the f32 noise of the sum it comes from moves by up to the learning rate in
    either direction -- in the reference's own f32 run too, whose yardstick is not available for the U-Net.  A handful
    of such elements among the 10^5 of a convolution decide the max-norm and say nothing about the arithmetic.  These
    tensors are therefore compared in 2-norm, the gradients Adam is handed in max-norm, and every element is held to
    what two Adam trajectories can differ by at all: an update is lr |m^| / (sqrt(v^) + eps) <= lr sqrt(sum a_i^2 / b_i)
    by Cauchy-Schwarz, a_i and b_i the normalised weights of the two moments, which is 1 at t = 1 and 1.0014 at t = 2;
    two runs are at most twice that apart per step."""
    if method != "method1":
        return ()
    return tuple(k for k in state if "running" not in k and "tracked" not in k)


_fused_cache = {}


def fused_run(method, graph, monkeypatch):
    key = (method, graph)
    if key not in _fused_cache:
        _fused_cache[key] = run_steps(method, "fused", graph, monkeypatch=monkeypatch)
    return _fused_cache[key]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("method", dc.METHODS)
def test_fused_equals_the_plain_composition(method, graph, monkeypatch):
    fused = fused_run(method, graph, monkeypatch)
    plain = run_steps(method, "plain", graph)
    assert fused["replayed"] == graph and plain["replayed"] == graph
    names = ["loss"] if method == "mt" else ["consistency_loss", "teacher_loss"]
    assert sorted(fused["meters"]) == names
    for k in names:
        e = dc.rel_scalar(fused["meters"][k], plain["meters"][k])
        print(f"{method} {'graph' if graph else 'eager'} meter {k}: fused {fused['meters'][k]:.9g} "
              f"plain {plain['meters'][k]:.9g}  e {e:.3g} (< {GRAD_TOL})")
        assert np.isfinite(fused["meters"][k]) and e < GRAD_TOL, (k, e)
    for k in ("sup_loss", "reg_loss"):
        e = dc.rel_scalar(fused["semi"][k], plain["semi"][k])
        print(f"{method} {k}: e {e:.3g}")
        assert e < GRAD_TOL, (k, e)
    if fused["adam_in"] is not None:
        names = [k for k in fused["state"] if "running" not in k and "tracked" not in k]
        sizes = [fused["state"][k].numel() for k in names]
        e_in = {k: dc.rel_max(a, b) for k, a, b in zip(names, fused["adam_in"].split(sizes),
                                                       plain["adam_in"].split(sizes))}
        worst = max(e_in, key=e_in.get)
        print(f"{method} gradient handed to Adam: worst {worst} {e_in[worst]:.3g} (< {GRAD_TOL})")
        assert e_in[worst] < GRAD_TOL, (worst, e_in[worst])
    raw = state_errors(fused["state"], plain["state"])
    errs = state_errors(fused["state"], plain["state"], two_norm_for=adam_moved(method, fused["state"]))
    worst, worst_raw = max(errs, key=errs.get), max(raw, key=raw.get)
    print(f"{method} teacher state: worst {worst} {errs[worst]:.3g} (< {GRAD_TOL}); in max-norm throughout: "
          f"{worst_raw} {raw[worst_raw]:.3g}")
    assert errs[worst] < GRAD_TOL, (worst, errs[worst])
    for k in adam_moved(method, fused["state"]):   # two steps of Adam: no element further apart than they can be
        ref = plain["state"][k].double()
        gap = float((fused["state"][k].double() - ref).abs().max())
        lim = 2 * ADAM_STEP_MAX * META_WEIGHT * 2 + GRAD_TOL * float(ref.abs().max())
        assert gap <= lim, (k, gap, lim)
    if adam_moved(method, fused["state"]):
        print(f"{method} largest element gap of a parameter: "
              f"{max(float((fused['state'][k] - plain['state'][k]).abs().max()) for k in adam_moved(method, fused['state'])):.3g}"
              f" (<= 2 * {ADAM_STEP_MAX} * lr * 2 steps = {4 * ADAM_STEP_MAX * META_WEIGHT:.3g} + GRAD_TOL * max)")


@pytest.mark.parametrize("method", dc.METHODS)
def test_replayed_steps_report_what_eager_steps_report(method, monkeypatch):
    eager, graph = fused_run(method, False, monkeypatch), fused_run(method, True, monkeypatch)
    assert graph["replayed"] and not eager["replayed"]
    print(method, "eager", eager["semi"]["sup_loss"], eager["semi"]["reg_loss"], eager["meters"], "graph",
          graph["semi"]["sup_loss"], graph["semi"]["reg_loss"], graph["meters"])
    assert eager["semi"]["sup_loss"] == graph["semi"]["sup_loss"]
    assert eager["semi"]["reg_loss"] == graph["semi"]["reg_loss"]
    assert eager["meters"] == graph["meters"]
    errs = state_errors(graph["state"], eager["state"])
    assert max(errs.values()) == 0.0, max(errs, key=errs.get)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("method", ["method2", "method4"])
def test_teacher_pass_leaves_the_students_step_unchanged(method, graph, monkeypatch):
    fused = fused_run(method, graph, monkeypatch)
    stub = run_steps(method, "stub", graph, seen=fused["seen"])
    assert len(fused["seen"]) == 2 and stub["replayed"] == graph
    worst = ("", 0.0)
    for name, a, b in zip(fused["names"], fused["offsets"], fused["offsets"][1:]):
        e = dc.rel_max(fused["grad"][a:b], stub["grad"][a:b])
        worst = max(worst, (name, e), key=lambda t: t[1])
    e_p = dc.rel_max(fused["params"], stub["params"])
    print(f"{method} {'graph' if graph else 'eager'}: worst student gradient {worst[0]} {worst[1]:.3g} "
          f"(< {GRAD_TOL}); parameters after two steps {e_p:.3g}")
    assert float(fused["grad"].abs().max()) > 0
    assert worst[1] < GRAD_TOL and e_p < GRAD_TOL, (worst, e_p)
    # the teacher pass must leave nothing behind at all: the same kernels run on the same inputs in the same order
    assert torch.equal(fused["grad"], stub["grad"]) and torch.equal(fused["params"], stub["params"])
    assert fused["semi"]["sup_loss"] == stub["semi"]["sup_loss"]


def test_bf16_autocast_step_of_method4(monkeypatch):
    """One bf16 step, fused and plain under the same autocast: both sides run the same bf16 network kernels and differ
    in the f32 loss arithmetic and the Adam kernel, so the bar is that of (c): GRAD_TOL on the losses and on every tensor
    of the teacher's state in max-norm (method 4 puts the teacher back before its EMA: no Adam division in the state)."""
    fused = run_steps("method4", "fused", False, bf16=True, steps=1, monkeypatch=monkeypatch)
    plain = run_steps("method4", "plain", False, bf16=True, steps=1)
    for k in ("consistency_loss", "teacher_loss"):
        e = dc.rel_scalar(fused["meters"][k], plain["meters"][k])
        print(f"bf16 method4 meter {k}: fused {fused['meters'][k]:.9g} plain {plain['meters'][k]:.9g} e {e:.3g}")
        assert np.isfinite(fused["meters"][k]) and e < GRAD_TOL, (k, e)
    assert all(bool(torch.isfinite(v).all()) for v in fused["state"].values() if v.is_floating_point())
    assert bool(torch.isfinite(fused["grad"]).all()) and float(fused["grad"].abs().max()) > 0
    errs = state_errors(fused["state"], plain["state"])
    worst = max(errs, key=errs.get)
    print(f"bf16 method4 teacher state: worst {worst} {errs[worst]:.3g} (< {GRAD_TOL})")
    assert errs[worst] < GRAD_TOL, (worst, errs[worst])


# ---------------------------------------------------------------- (e) through SemiTrainer
def test_one_epoch_through_the_trainer_and_the_checkpoint(tmp_path):
    from contrastyou.arch import UNet
    from contrastyou.losses.kl import KL_div
    from oracle import unet as ou
    from semi_seg.hooks import DifferentiableMeanTeacherTrainerHook
    from semi_seg.trainers import trainer_zoo
    g = torch.Generator().manual_seed(21)
    lab, unl = [blob_batch(2, HW, K, g) for _ in range(2)], [blob_batch(2, HW, K, g) for _ in range(2)]
    val = [{k: v[0] for k, v in blob_batch(2, HW, K, g, views=1).items()}]
    cfg = {"Optim": {"name": "RAdam", "lr": 3e-3, "weight_decay": 1e-4}, "Trainer": {"name": "semi"}}

    def make(seed, where):
        model = UNet(input_dim=1, num_classes=K, max_channel=MAXC, momentum=0.1)
        model.load_state_dict(ou.init_state_dict(1, K, MAXC, seed=seed))
        tr = trainer_zoo["semi"](model=model, labeled_loader=Loader(lab), unlabeled_loader=Loader(unl),
                                 val_loader=Loader(val), test_loader=Loader(val), criterion=KL_div(),
                                 save_dir=str(where), max_epoch=1, num_batches=2, device=DEV, disable_bn=False,
                                 two_stage=True, config=cfg, enable_scale=False)
        hook = DifferentiableMeanTeacherTrainerHook(name="dmt", model=model, weight=0.5, meta_criterion="dice",
                                                    method_name="method1")
        return tr, hook

    tr, hook = make(14, tmp_path / "a")   # built on the CPU: the construction-time pass waits for the GPU
    assert hook._needs_init
    random.seed(9)
    with tr.register_hook(hook):
        assert not hook._needs_init       # ran when the trainer moved the hook to the GPU
        tr.init()
        tr.to(DEV)
        train = tr.tra_epoch()
        tr.save_to(save_name="last.pth")
    torch.cuda.synchronize()
    assert sorted(train["dmt"]) == ["consistency_loss", "teacher_loss"]
    assert all(np.isfinite(v) and v > 0 for v in train["dmt"].values()), train["dmt"]
    assert np.isfinite(train["semi"]["reg_loss"]) and train["semi"]["reg_loss"] > 0
    teacher = hook.flat_teacher
    assert teacher.adam_steps == 2 and hook._updater._global_step == 2
    lo = teacher.flat.data.data_ptr()
    assert all(p.is_cuda and lo <= p.data_ptr() < lo + 4 * teacher.flat.numel
               for p in hook.teacher_model.parameters())
    want = {k: v.detach().cpu().clone() for k, v in hook.teacher_model.state_dict().items()}
    moved = [k for k, v in want.items() if v.is_floating_point()
             and not torch.equal(v, tr._model.state_dict()[k].cpu())]
    assert moved, "the teacher is a model of its own"
    tr2, hook2 = make(15, tmp_path / "b")
    with tr2.register_hook(hook2):
        tr2.init()
        tr2.load_state_dict_from_path(str(tmp_path / "a"), name="last.pth")
        tr2.to(DEV)
    got = hook2.teacher_model.state_dict()
    assert all(torch.equal(got[k].cpu(), v) for k, v in want.items())
    assert "_hooks.0._teacher_model._Conv1.conv.0.weight" in tr.state_dict()["module_state"]
    assert not any("exp_avg" in k for k in tr.state_dict()["module_state"])
