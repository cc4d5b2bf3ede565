"""Loader augmentation on the GPU (csrc/cy_augment.hip) against the NumPy restatement of tests/augment_cases.py and
the stored Pillow run (tests/golden/augment.npz), bit for bit; the device loader's batches; one training step fed by it.

The tolerance is zero and that is derived, not measured: the nearest path and the contrast mean are integer
arithmetic, the bilinear path is a fixed sequence of single IEEE float64 operations and the jitter one of single
float32 operations (contraction to fma is off in the kernels), and the restatement performs the same operations in the
same order; ToTensor is a table both sides read.  Pillow is not imported here."""
import random
from pathlib import Path

import numpy as np
import pytest
import torch

import augment_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = np.load(Path(__file__).resolve().parent / "golden" / "augment.npz")


def _t(a):
    return torch.from_numpy(np.array(a))  # a copy: the shared cases are read-only


def _run(c, ip=None, labels=True, out_hw=None, lut="case"):
    from cyhip import ops
    if lut == "case":
        lut = None if c["mapping"] is None else _t(ac.label_lut(c["mapping"])).to(DEV)
    return ops.augment_views(_t(c["arena_img"]).to(DEV), _t(c["arena_lab"]).to(DEV), _t(c["table"]),
                             _t(c["ip"] if ip is None else ip), _t(c["fp"]), lut, out_hw or c["out_hw"], labels=labels)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", list(ac.CASES))
def test_kernels_equal_the_restatement_and_the_goldens(name):
    c = ac.case(name)
    images, labels = _run(c)
    B, (h, w) = len(c["views"]), c["out_hw"]
    assert images.shape == (B, 1, h, w) and images.dtype == torch.float32 and images.is_contiguous()
    assert labels.shape == (B, 1, h, w) and labels.dtype == torch.int64
    diff = _bits(images) != c["images"].view(np.uint32)
    print(f"{name}: {B} views of {h}x{w}: {int(diff.sum())} image values and "
          f"{int((labels.cpu().numpy() != c['labels']).sum())} labels differ")
    assert not diff.any()
    assert np.array_equal(labels.cpu().numpy(), c["labels"])
    # Pillow's own output, stored: the f32 values are the table's entries of its uint8 pixels
    assert np.array_equal(_bits(images)[:, 0], ac.TENSOR_LUT[GOLDEN[f"{name}_jit"]].view(np.uint32))
    assert np.array_equal(labels.cpu().numpy()[:, 0], ac.label_lut(c["mapping"])[GOLDEN[f"{name}_lab"]])
    assert np.array_equal(GOLDEN[f"{name}_ip"], c["ip"]) and np.array_equal(GOLDEN[f"{name}_fp"], c["fp"])


def test_two_runs_give_the_same_bits_and_labels_are_optional():
    c = ac.case("past_one_tile")
    a, la = _run(c)
    b, lb = _run(c)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(la, lb)
    only, none = _run(c, labels=False)
    assert none is None and torch.equal(only.view(torch.int32), a.view(torch.int32))
    # an explicit identity table is the default
    _, lid = _run(c, lut=torch.arange(256, dtype=torch.uint8, device=DEV))
    assert torch.equal(lid, la)


def test_limits_run_and_one_above_each_is_refused():
    from cyhip import _lib, ops
    img, lab = ac.noise(40, 40, 21)
    arena_i, arena_l = _t(img.reshape(-1)).to(DEV), _t(lab.reshape(-1)).to(DEV)
    table = torch.tensor([[0, 40, 40]], dtype=torch.int64)

    def call(views, h, w):
        ip = np.zeros((views, ac.IP_LEN), dtype=np.int32)
        ip[:, ac.IP["ch"]], ip[:, ac.IP["cw"]] = 40, 40
        ip[:, ac.IP["qy"]] = np.arange(views) % 33
        return ops.augment_views(arena_i, arena_l, table, _t(ip), torch.zeros(views, ac.FP_LEN, dtype=torch.float64),
                                 None, (h, w))

    images, labels = call(4096, 8, 8)  # the most views
    want = np.stack([ac.window(img, q % 33, 0, 8, 8) for q in (0, 1, 32, 33, 4095)])
    assert np.array_equal(_bits(images[[0, 1, 32, 33, 4095], 0]), ac.TENSOR_LUT[want].view(np.uint32))
    assert np.array_equal(labels[4095, 0].cpu().numpy(), ac.window(lab, 4095 % 33, 0, 8, 8))
    images, labels = call(1, 512, 512)  # the largest output: the slice in a corner of zeros
    assert np.array_equal(_bits(images[0, 0]), ac.TENSOR_LUT[ac.window(img, 0, 0, 512, 512)].view(np.uint32))
    assert int(labels.sum()) == int(lab.sum())
    for views, h, w in ((4097, 8, 8), (1, 513, 512), (1, 512, 513)):
        with pytest.raises(_lib.HipKernelError, match="CY_ERR_SHAPE"):
            call(views, h, w)


def test_rejections_give_their_exact_status():
    from cyhip import _lib
    c = ac.case("three_sizes")

    def bad(col, value):
        ip = c["ip"].copy()
        ip[1, col] = value
        return ip

    for col, value, status in ((ac.IP["slice"], 3, "CY_ERR_SHAPE"), (ac.IP["slice"], -1, "CY_ERR_SHAPE"),
                               (ac.IP["cw"], 1025, "CY_ERR_SHAPE"), (ac.IP["qy"], 5000, "CY_ERR_SHAPE"),
                               (ac.IP["fv"], 2, "CY_ERR_ARG"), (ac.IP["njit"], 4, "CY_ERR_ARG"),
                               (ac.IP["kind0"], 3, "CY_ERR_ARG")):
        with pytest.raises(_lib.HipKernelError, match=status):
            _run(c, ip=bad(col, value))
    short = dict(c, arena_img=c["arena_img"][:-1], arena_lab=c["arena_lab"][:-1])  # the last slice leaves the arena
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_SHAPE"):
        _run(short)
    with pytest.raises(ValueError, match="one record per view"):
        _run(c, ip=c["ip"][:, :-1])
    images, _ = _run(c)  # and the unchanged records still run
    assert np.array_equal(_bits(images), c["images"].view(np.uint32))


# ---- the loader ----------------------------------------------------------------------------------------------------
def _store(n=12, hw=40, mapping=None):
    from semi_seg.data import DeviceSliceStore
    pairs = [ac.noise(hw, hw, 100 + i) for i in range(n)]
    names = [f"patient{i // 4:03d}_{i % 2:02d}_{i:02d}" for i in range(n)]
    store = DeviceSliceStore.from_arrays([p[0] for p in pairs], [p[1] for p in pairs], names,
                                         group_re=r"patient\d+_\d+", partitions=[str(i % 3) for i in range(n)],
                                         mapping=mapping, device=DEV)
    return store, pairs, names


def _pipeline(total_freedom=False, mapping=None):
    from contrastyou.augment import DevicePipeline
    return DevicePipeline(rotation=30, vflip=True, hflip=True, crop=32, jitter=((0.5, 1.5),) * 3, mapping=mapping,
                          total_freedom=total_freedom)


@pytest.mark.parametrize("twice", [True, False])
def test_loader_yields_the_batch_the_epochers_unpack(twice):
    from semi_seg.data import DeviceLoader
    from semi_seg.epochers.helper import (preprocess_input_with_single_transformation,
                                          preprocess_input_with_twice_transformation)
    store, pairs, names = _store(mapping=ac.ACDC_MYO)
    indices = [[3, 0, 7], [11, 2, 5], [1]]
    loader = DeviceLoader(store, _pipeline(mapping=ac.ACDC_MYO), indices, twice=twice, seed=4)
    assert len(loader) == 3 and loader.dataset.transforms._total_freedom is False
    batches = list(loader)
    assert len(batches) == 3
    for idx, data in zip(indices, batches):
        assert sorted(data) == ["filename", "gt", "img", "partition", "scan_num"]
        if twice:
            (v1, t1), (v2, t2), filename, partition, scan = preprocess_input_with_twice_transformation(data, DEV)
            assert data["filename"][1] == filename
            views = [(v1, t1), (v2, t2)]
        else:
            v1, t1, filename, partition, scan = preprocess_input_with_single_transformation(data, DEV)
            views = [(v1, t1)]
        assert filename == [names[i] for i in idx] and partition == [str(i % 3) for i in idx]
        assert scan == [names[i][:13] for i in idx]
        for img, gt in views:
            assert img.shape == (len(idx), 1, 32, 32) and img.dtype == torch.float32 and img.is_cuda
            assert gt.shape == (len(idx), 1, 32, 32) and gt.dtype == torch.int64 and gt.is_cuda
            assert 0.0 <= float(img.min()) and float(img.max()) <= 1.0 and float(img.max()) > 0.3
            assert set(gt.unique().tolist()) == {0, 1}  # through ToLabel's mapping
    if twice:  # total_freedom False: one geometry (the labels agree), two jitters (the images do not)
        data = batches[0]
        assert torch.equal(data["gt"][0], data["gt"][1]) and not torch.equal(data["img"][0], data["img"][1])
    # the views are the restatement's for the records the pipeline drew
    from semi_seg.data import batch_seed
    seed = batch_seed(4, 0, 0)
    p = loader.pipeline.draw_twice(3, seed, store.sizes(indices[0]))[0] if twice else \
        loader.pipeline.draw(3, seed, store.sizes(indices[0]))
    first = batches[0]["img"][0] if twice else batches[0]["img"]
    for k, i in enumerate(indices[0]):
        r, f = p.int_params[k], p.f64_params[k]
        v = ac.view(fv=bool(r[ac.IP["fv"]]), fh=bool(r[ac.IP["fh"]]), post=(int(r[ac.IP["qy"]]), int(r[ac.IP["qx"]])),
                    jitter=[("bc"[r[ac.IP["kind0"] + j] - 1], f[ac.FP["f0"] + j]) for j in range(r[ac.IP["njit"]])])
        v["m"] = [float(x) for x in f[:6]] if r[ac.IP["rot"]] else None
        want = ac.jitter(ac.geometry(pairs[i][0], v, (32, 32), False), v["jitter"])
        assert np.array_equal(_bits(first[k, 0]), ac.TENSOR_LUT[want].view(np.uint32)), k


def test_two_epochs_and_two_loaders_with_one_seed_agree_and_ranks_differ():
    from semi_seg.data import DeviceLoader
    store, _, _ = _store()
    indices = [[0, 1, 2, 3], [4, 5, 6, 7]]
    loader = DeviceLoader(store, _pipeline(total_freedom=True), indices, seed=7)
    first, second = list(loader), list(loader)
    other = list(DeviceLoader(store, _pipeline(total_freedom=True), indices, seed=7))
    ranked = list(DeviceLoader(store, _pipeline(total_freedom=True), indices, seed=7, rank=1))
    for a, b, c, d in zip(first, second, other, ranked):
        for k in range(2):
            assert torch.equal(a["img"][k], b["img"][k]) and torch.equal(a["gt"][k], b["gt"][k])
            assert torch.equal(a["img"][k], c["img"][k]) and torch.equal(a["gt"][k], c["gt"][k])
            assert not torch.equal(a["img"][k], d["img"][k])
        assert not torch.equal(a["gt"][0], a["gt"][1])  # total freedom: two geometries
    assert not torch.equal(first[0]["img"][0], first[1]["img"][0])
    with pytest.raises(IndexError):
        next(iter(DeviceLoader(store, _pipeline(), [[0, 12]])))


def test_a_training_step_fed_by_two_device_loaders():
    """two batches of SemiSupervisedEpocher from a labeled and an unlabeled DeviceLoader over one 12-slice store: the
    losses are finite and the weights move; producing a batch makes no host synchronisation (sync debug mode raises
    on one), so nothing stands between next(loader) and the step but the stream they share"""
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.kl import KL_div
    from contrastyou.optim import RAdam
    from oracle import unet as ou
    from semi_seg.data import DeviceLoader
    from semi_seg.epochers import SemiSupervisedEpocher
    from semi_seg.hooks import create_infonce_hooks
    store, _, _ = _store()
    lab = DeviceLoader(store, _pipeline(), [[0, 1, 2], [3, 4, 5]], seed=1)
    unl = DeviceLoader(store, _pipeline(), [[6, 7, 8], [9, 10, 11]], seed=2)
    next(iter(lab))  # the first batch uploads the tables kept per device
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        it = iter(unl)
        data = [next(it), next(it)]
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert all(torch.isfinite(d["img"][0]).all() for d in data)

    model = UNet(input_dim=1, num_classes=4, max_channel=128, momentum=0.01)
    model.load_state_dict(ou.init_state_dict(1, 4, 128, seed=3))
    model.to(DEV)
    type(TrainerHook).names.clear()
    torch.manual_seed(3)
    hook = create_infonce_hooks(model=model, feature_names="Conv5", weights=1.0, contrast_ons="partition",
                                spatial_size=1, data_name="acdc").to(DEV)
    opt = RAdam([{"params": list(model.parameters())}, {"params": list(hook.parameters())}], lr=1e-3, weight_decay=1e-5)
    before = [p.detach().clone() for p in model.parameters()]
    ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=lab, unlabeled_loader=unl,
                               sup_criterion=KL_div(), num_batches=2, cur_epoch=0, device=DEV, two_stage=True,
                               disable_bn=False, scaler=torch.amp.GradScaler("cuda", enabled=False), accumulate_iter=1)
    ep.init()
    random.seed(5)
    with ep.register_hook(hook()):
        ep.run()
    torch.cuda.synchronize()
    semi = ep.get_metric()["semi"]
    assert np.isfinite(semi["sup_loss"]) and semi["sup_loss"] > 0 and np.isfinite(semi["reg_loss"])
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    assert all(torch.isfinite(p).all() for p in model.parameters())
