"""Host-side checks of the adversarial baseline (no GPU): constructor signatures against the reference's names
(tests/golden/adversarial_signatures.txt), the discriminator's state dict and initialisation, the argument checks and
workspace sizes of every entry point of csrc/cy_disc.hip (no launch is ever made), the CPU-tensor and world-size
refusals and a checkpoint round trip of the discriminator and its optimizer.  No kernel runs here."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
from torch import nn

from adversarial_fixture import BUFFERS, HIDDEN, K, PARAMS, SEED, replica, state_dict_of

ARG, WS = -1, -5


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def host():
    """a 16-byte aligned host buffer: no launch may ever see it"""
    buf = (ctypes.c_float * 80)()
    addr = ctypes.addressof(buf)
    return buf, addr + (-addr) % 16


# ---------------------------------------------------------------------------------------------- signatures
def _names(cls):
    out = []
    for n, p in inspect.signature(cls.__init__).parameters.items():
        if n != "self":
            out.append("**" + n if p.kind is inspect.Parameter.VAR_KEYWORD else n)
    return out


def test_constructor_signatures_are_the_reference_ones(golden_dir):
    from contrastyou.arch.discriminator import Discriminator
    from semi_seg.epochers.comparable import AdversarialEpocher
    from semi_seg.trainers.trainer import AdversarialTrainer
    want = dict(line.split(": ") for line in (golden_dir / "adversarial_signatures.txt").read_text().splitlines())
    assert set(want) == {"Discriminator", "AdversarialEpocher", "AdversarialTrainer"}
    for cls in (Discriminator, AdversarialEpocher, AdversarialTrainer):
        assert _names(cls) == want[cls.__name__].split(), cls.__name__
    kinds = {n: p.kind for n, p in inspect.signature(AdversarialEpocher.__init__).parameters.items()}
    assert all(k in (inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.VAR_KEYWORD)
               for n, k in kinds.items() if n != "self")
    sig = inspect.signature(AdversarialTrainer.__init__).parameters
    assert sig["dis_consider_image"].default is False and sig["reg_weight"].default is inspect.Parameter.empty
    assert AdversarialTrainer.activate_hooks is False and AdversarialTrainer.train_epocher.fget(None) is AdversarialEpocher


def test_trainer_zoo_and_stub_factories_are_unchanged():
    from semi_seg.trainers import trainer_zoo
    assert sorted(trainer_zoo) == ["dmt", "ft", "mixup", "mt", "pretrain", "pretrain_decoder", "semi"]


# ---------------------------------------------------------------------------------------------- the module
def test_state_dict_keys_shapes_and_dtypes(golden_dir):
    from contrastyou.arch.discriminator import Discriminator
    data = np.load(golden_dir / "adversarial.npz")
    for arm in (True, False):
        want = state_dict_of(data, arm)
        dis = Discriminator(5 if arm else K, HIDDEN)
        got = dis.state_dict()
        assert list(got) == list(want)
        assert [k for k in got if k not in BUFFERS] == list(PARAMS)
        for k in want:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        dis.load_state_dict(want, strict=True)
        replica(dis.state_dict(), arm)  # and back into torch's own layers, strict
    h = 8
    shapes = {k: tuple(v.shape) for k, v in Discriminator(5, h).state_dict().items()}
    assert shapes["_main.0.weight"] == (h, 5, 4, 4) and shapes["_main.2.weight"] == (2 * h, h, 4, 4)
    assert shapes["_main.5.weight"] == (4 * h, 2 * h, 4, 4) and shapes["_main.8.weight"] == (8 * h, 4 * h, 4, 4)
    assert shapes["_main.11.weight"] == (1, 8 * h, 4, 4) and shapes["_main.9.running_var"] == (8 * h,)
    assert shapes["_main.6.num_batches_tracked"] == ()


def test_weights_init_draws_what_torch_draws_under_the_seed(golden_dir):
    """the same normal_ / constant_ calls in the same module order: equal to the layers built and initialised by hand
    here, and to the state dict the reference produced under SEED"""
    from contrastyou.arch.discriminator import Discriminator, weights_init
    torch.manual_seed(SEED)
    dis = Discriminator(5, HIDDEN)
    data = np.load(golden_dir / "adversarial.npz")
    for k, v in state_dict_of(data, True).items():
        assert torch.equal(dis.state_dict()[k], v), k
    torch.manual_seed(SEED)
    h = HIDDEN
    layers = [nn.Conv2d(5, h, 4, 2, 1, bias=False), nn.Conv2d(h, 2 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(2 * h),
              nn.Conv2d(2 * h, 4 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(4 * h),
              nn.Conv2d(4 * h, 8 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(8 * h),
              nn.Conv2d(8 * h, 1, 4, 1, 0, bias=False)]
    for m in layers:
        if isinstance(m, nn.Conv2d):
            nn.init.normal_(m.weight.data, 0.0, 0.02)
        else:
            nn.init.normal_(m.weight.data, 1.0, 0.02)
            nn.init.constant_(m.bias.data, 0)
    mine = [m for m in dis._main if isinstance(m, (nn.Conv2d, nn.BatchNorm2d))]
    for a, b in zip(mine, layers):
        assert torch.equal(a.weight, b.weight)
    lin = nn.Linear(3, 3)
    before = lin.weight.clone()
    weights_init(lin)  # neither a convolution nor a BatchNorm: untouched
    assert torch.equal(lin.weight, before)


def test_cpu_tensors_are_refused():
    from contrastyou.arch.discriminator import Discriminator
    from cyhip.functions import BNLeakyReLUFn, LeakyReLUFn, SigmoidBCEFn, SoftmaxCatFn
    dis = Discriminator(5, HIDDEN)
    x, z, img = torch.rand(2, 5, 64, 64), torch.rand(2, 4, 64, 64), torch.rand(2, 1, 64, 64)
    for call in (lambda: dis(x), lambda: dis.scores(x), lambda: dis.scores_from_logits(img, z),
                 lambda: dis.scores_from_logits(None, z), lambda: SoftmaxCatFn.apply(img, z),
                 lambda: LeakyReLUFn.apply(x, 0.2), lambda: SigmoidBCEFn.apply(x, 1.0),
                 lambda: BNLeakyReLUFn.apply(x, torch.ones(5), torch.zeros(5), None, None, None, True, 0.1, 1e-5, 0.2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---------------------------------------------------------------------------------------------- the entry points
ENTRIES = ("cy_softmax_cat_fwd", "cy_softmax_cat_bwd", "cy_bn_rows_ws_bytes", "cy_bn_rows_stats", "cy_bn_lrelu_fwd",
           "cy_bn_lrelu_bwd_reduce", "cy_bn_lrelu_bwd_apply", "cy_leaky_relu_fwd", "cy_leaky_relu_bwd",
           "cy_sigmoid_bce_ws_bytes", "cy_sigmoid_bce_fwd", "cy_sigmoid_bce_bwd")


def test_library_exports_the_new_entries_and_the_abi_version_stays(lib):
    from cyhip import _lib
    assert lib.cy_abi_version() == _lib.ABI_VERSION
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.exported_names(), name


def _bn_calls(lib, p, M, C, big):
    return [("stats", lib.cy_bn_rows_stats(p, p, p, M, C, p, p, p, 0.1, p, big, None)),
            ("fwd", lib.cy_bn_lrelu_fwd(p, p, p, p, p, p, M, C, 1e-5, 0.2, None)),
            ("bwd_reduce", lib.cy_bn_lrelu_bwd_reduce(p, p, p, p, p, p, p, p, M, C, 1e-5, 0.2, p, big, None)),
            ("bwd_apply", lib.cy_bn_lrelu_bwd_apply(p, p, p, p, p, p, p, p, p, M, C, 1e-5, 0.2, 1, None))]


def test_bad_sizes_are_refused_before_any_launch(lib, host):
    _, p = host
    big = 1 << 24
    for Kc in (1, 17, 0, -4):
        assert lib.cy_softmax_cat_fwd(p, p, p, 286, 1, Kc, None) == ARG, Kc
        assert lib.cy_softmax_cat_bwd(p, p, p, 286, 1, Kc, None) == ARG, Kc
    for Ci in (-1, 5):
        assert lib.cy_softmax_cat_fwd(p, p, p, 286, Ci, 4, None) == ARG, Ci
        assert lib.cy_softmax_cat_bwd(p, p, p, 286, Ci, 4, None) == ARG, Ci
    assert lib.cy_softmax_cat_fwd(p, p, p, 286, 0, 4, None) == ARG  # an image without image channels
    assert lib.cy_softmax_cat_fwd(None, p, p, 286, 1, 4, None) == ARG  # image channels without an image
    for npix in (0, -1):
        assert lib.cy_softmax_cat_fwd(None, p, p, npix, 0, 4, None) == ARG
        assert lib.cy_softmax_cat_bwd(p, p, p, npix, 0, 4, None) == ARG
    for C in (0, -3, 1025):
        for name, rc in _bn_calls(lib, p, 48, C, big):
            assert rc == ARG, (name, C, rc)
    for M in (0, -1):
        for name, rc in _bn_calls(lib, p, M, 8, big):
            assert rc == ARG, (name, M, rc)
    # one row has no batch variance: the statistics and the batch-statistics gradient refuse it
    assert lib.cy_bn_rows_stats(p, p, p, 1, 8, None, None, None, 0.1, p, big, None) == ARG
    assert lib.cy_bn_lrelu_bwd_apply(p, p, p, p, p, p, p, p, p, 1, 8, 1e-5, 0.2, 1, None) == ARG
    assert lib.cy_bn_rows_stats(p, p, p, 48, 8, p, None, None, 0.1, p, big, None) == ARG  # one running buffer alone
    for n in (0, -5):
        assert lib.cy_leaky_relu_fwd(p, p, n, 0.2, None) == ARG
        assert lib.cy_leaky_relu_bwd(p, p, p, n, 0.2, None) == ARG
        assert lib.cy_sigmoid_bce_fwd(p, 1.0, p, n, p, big, None) == ARG
        assert lib.cy_sigmoid_bce_bwd(p, 1.0, p, p, n, None) == ARG
    for label in (0.5, -1.0, 2.0, float("nan")):
        assert lib.cy_sigmoid_bce_fwd(p, label, p, 6, p, big, None) == ARG, label
        assert lib.cy_sigmoid_bce_bwd(p, label, p, p, 6, None) == ARG, label
    # rows read 16 bytes at a time need a 16-byte aligned base
    assert lib.cy_bn_lrelu_fwd(p + 4, p, p, p, p, p, 48, 8, 1e-5, 0.2, None) == ARG
    assert lib.cy_softmax_cat_fwd(None, p + 4, p, 286, 0, 4, None) == ARG


def test_null_pointers_are_refused_before_any_launch(lib, host):
    _, p = host
    big = 1 << 24

    def each_null(fn, args, pointer_slots):
        for i in pointer_slots:
            a = list(args)
            a[i] = None
            assert fn(*a) == ARG, (fn.__name__, i)

    each_null(lib.cy_softmax_cat_fwd, [p, p, p, 286, 1, 4, None], (0, 1, 2))
    each_null(lib.cy_softmax_cat_fwd, [None, p, p, 286, 0, 4, None], (1, 2))
    each_null(lib.cy_softmax_cat_bwd, [p, p, p, 286, 1, 4, None], (0, 1, 2))
    each_null(lib.cy_bn_rows_stats, [p, p, p, 48, 8, p, p, p, 0.1, p, big, None], (0, 1, 2, 9))
    each_null(lib.cy_bn_lrelu_fwd, [p, p, p, p, p, p, 48, 8, 1e-5, 0.2, None], range(6))
    each_null(lib.cy_bn_lrelu_bwd_reduce, [p] * 8 + [48, 8, 1e-5, 0.2, p, big, None], list(range(8)) + [12])
    each_null(lib.cy_bn_lrelu_bwd_apply, [p] * 9 + [48, 8, 1e-5, 0.2, 1, None], range(9))
    each_null(lib.cy_bn_lrelu_bwd_apply, [p] * 9 + [48, 8, 1e-5, 0.2, 0, None], (0, 1, 2, 3, 4, 5, 8))
    each_null(lib.cy_leaky_relu_fwd, [p, p, 7, 0.2, None], (0, 1))
    each_null(lib.cy_leaky_relu_bwd, [p, p, p, 7, 0.2, None], (0, 1, 2))
    each_null(lib.cy_sigmoid_bce_fwd, [p, 1.0, p, 6, p, big, None], (0, 2, 4))
    each_null(lib.cy_sigmoid_bce_bwd, [p, 0.0, p, p, 6, None], (0, 2, 3))


def _bn_ws(M, C):
    V = 4 if C % 4 == 0 else 1
    ncv, lpr = C // V, 1
    while lpr < ncv and lpr < 64:
        lpr *= 2
    rows = (256 // lpr) * 8
    return 16 * C * min(256, max(1, -(-M // rows)))


@pytest.mark.parametrize("M,C", [(48, 512), (770, 128), (257, 20), (2, 4), (259, 7), (45, 1023), (768, 6), (960, 12),
                                 (60, 24), (16 * 56 * 56, 128), (16 * 28 * 28, 256), (16 * 14 * 14, 512), (1 << 33, 1024),
                                 (2, 1), (1, 1024)])
def test_bn_workspace_sizes_and_short_workspaces(lib, host, M, C):
    _, p = host
    want = _bn_ws(M, C)
    assert lib.cy_bn_rows_ws_bytes(M, C) == want
    if M >= 2:
        assert lib.cy_bn_rows_stats(p, p, p, M, C, None, None, None, 0.1, p, want - 1, None) == WS
    assert lib.cy_bn_lrelu_bwd_reduce(p, p, p, p, p, p, p, p, M, C, 1e-5, 0.2, p, want - 1, None) == WS


def test_bn_workspace_is_zero_for_sizes_out_of_range(lib):
    for M, C in ((0, 8), (-1, 8), (48, 0), (48, 1025)):
        assert lib.cy_bn_rows_ws_bytes(M, C) == 0


@pytest.mark.parametrize("n", [1, 6, 255, 256, 257, 363, 1025, 16 * 11 * 11, 270000, 1 << 31])
def test_bce_workspace_sizes_and_short_workspaces(lib, host, n):
    """one f64 partial per block of 256 scores, at most 1024 blocks"""
    _, p = host
    want = 8 * min(max((n + 255) // 256, 1), 1024)
    assert lib.cy_sigmoid_bce_ws_bytes(n) == want
    assert lib.cy_sigmoid_bce_fwd(p, 1.0, p, n, p, want - 1, None) == WS
    assert lib.cy_sigmoid_bce_ws_bytes(0) == 0


def test_wrapper_raises_on_a_refused_call(host):
    from cyhip import _lib
    _, p = host
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_ARG"):
        _lib.call("cy_sigmoid_bce_fwd", p, 0.5, p, 6, p, 1 << 20, None)
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_WORKSPACE"):
        _lib.call("cy_bn_rows_stats", p, p, p, 48, 8, None, None, None, 0.1, p, 15, None)


# ---------------------------------------------------------------------------------------------- the trainer
CFG = {"Optim": {"name": "RAdam", "lr": 1e-4, "weight_decay": 1e-5, "pre_lr": 1.0, "ft_lr": 2.0},
       "Scheduler": {"multiplier": 300, "warmup_max": 10}, "Trainer": {"name": "adv"}, "RandomSeed": 7}


class _Loader(list):
    """an empty loader whose dataset passes the epocher's transform check"""
    dataset = type("_DS", (), {"transforms": type("_T", (), {"_total_freedom": False})})()


def _trainer(tmp_path, consider_image=True, **kw):
    from contrastyou.arch import UNet
    from contrastyou.losses.kl import KL_div
    from semi_seg.trainers.trainer import AdversarialTrainer
    tr = AdversarialTrainer(model=UNet(input_dim=1, num_classes=4, max_channel=128), labeled_loader=_Loader(),
                            unlabeled_loader=_Loader(), val_loader=[], test_loader=[], criterion=KL_div(),
                            save_dir=str(tmp_path), max_epoch=30, num_batches=2, device="cpu", disable_bn=False,
                            two_stage=False, config=CFG, reg_weight=0.25, dis_consider_image=consider_image, **kw)
    tr.init()
    return tr


def test_trainer_builds_the_discriminator_under_the_config_seed(tmp_path):
    from contrastyou.arch.discriminator import Discriminator
    from contrastyou.optim import FusedRAdam
    from semi_seg.epochers.comparable import AdversarialEpocher
    tr = _trainer(tmp_path / "a")
    torch.manual_seed(CFG["RandomSeed"])
    twin = Discriminator(5, 64)
    assert all(torch.equal(a, b) for a, b in zip(tr._discriminator.state_dict().values(), twin.state_dict().values()))
    assert tr._discriminator._main[0].weight.shape == (64, 5, 4, 4)
    assert _trainer(tmp_path / "b", consider_image=False)._discriminator._main[0].weight.shape == (64, 4, 4, 4)
    assert isinstance(tr._dis_optimizer, FusedRAdam) and tr._dis_optimizer is not tr._optimizer
    group = tr._dis_optimizer.param_groups[0]
    assert group["lr"] == 1e-4 and group["weight_decay"] == 1e-5 and "pre_lr" not in group and "name" not in group
    assert [id(p) for p in group["params"]] == [id(p) for p in tr._discriminator.parameters()]
    assert tr._reg_weight == 0.25 and tr.train_epocher is AdversarialEpocher
    ep = tr._create_initialized_tra_epoch()
    assert isinstance(ep, AdversarialEpocher) and ep._discriminator is tr._discriminator
    assert ep._discr_optimizer is tr._dis_optimizer and ep._reg_weight == 0.25 and ep._dis_consider_image is True
    assert set(dict(ep.meters.statistics())["adv_reg"]) == {"dis_loss", "gen_loss", "reg_weight"}
    assert "reg_loss" not in dict(ep.meters.statistics())["semi"]


def test_checkpoint_round_trip_of_discriminator_and_optimizer(tmp_path):
    tr = _trainer(tmp_path)
    sd = tr.state_dict()
    assert "_discriminator._main.0.weight" in sd["module_state"]
    assert "_discriminator._main.9.running_var" in sd["module_state"]
    assert "_discriminator._main.3.num_batches_tracked" in sd["module_state"]
    assert {"_optimizer", "_dis_optimizer"} <= set(sd["other_state"])
    dopt = tr._dis_optimizer
    dopt.zero_grad()  # builds the flat buffers (on the CPU here)
    st = dopt._flat_state[0]
    st["step"], st["steps"] = 3, [3] * len(st["steps"])
    st["exp_avg"].copy_(torch.linspace(-1, 1, st["exp_avg"].numel()))
    st["exp_avg_sq"].copy_(torch.linspace(0, 2, st["exp_avg_sq"].numel()))
    with torch.no_grad():
        tr._discriminator._main[0].weight.fill_(0.125)
        tr._discriminator._main[6].running_mean.fill_(-0.5)
        tr._discriminator._main[9].running_var.fill_(1.5)
        tr._discriminator._main[3].num_batches_tracked.fill_(9)
    tr.save_to(save_name="last.pth")
    tr2 = _trainer(tmp_path)
    assert float(tr2._discriminator._main[0].weight.detach().flatten()[0]) != 0.125
    tr2.resume_from_path(str(tmp_path))
    d2 = tr2._discriminator
    assert torch.equal(d2._main[0].weight, tr._discriminator._main[0].weight)
    assert float(d2._main[6].running_mean[0]) == -0.5 and float(d2._main[9].running_var[0]) == 1.5
    assert int(d2._main[3].num_batches_tracked) == 9
    for k, v in tr._discriminator.state_dict().items():
        assert torch.equal(d2.state_dict()[k], v), k
    tr2._dis_optimizer.zero_grad()  # the loaded moments are applied when the flat buffers exist
    st2 = tr2._dis_optimizer._flat_state[0]
    assert st2["step"] == 3 and st2["steps"] == [3] * len(st2["steps"])
    assert torch.equal(st2["exp_avg"], st["exp_avg"]) and torch.equal(st2["exp_avg_sq"], st["exp_avg_sq"])
    assert float(d2._main[0].weight.detach().flatten()[0]) == 0.125  # flattening kept the loaded values


def test_more_than_one_process_is_refused(tmp_path, monkeypatch):
    """two flat-buffer optimizers would both write cyhip.ops.DP_EARLY: a mocked torch.distributed with world size 2"""
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="DP_EARLY"):
        _trainer(tmp_path)
    monkeypatch.undo()
    assert _trainer(tmp_path)._reg_weight == 0.25
