"""SLIC superpixels on the GPU (csrc/cy_slic.hip), stage by stage against the NumPy restatement of tests/slic_cases.py:
the blur within one quantisation step of scipy's float64 blur, everything after it bit for bit; then the online
superpixel hook against `SuperPixelInfoNCEHook` fed the same map."""
import random

import numpy as np
import pytest
import torch

import slic_cases as sc
from test_gpu_hooks_dice import Loader, blob_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(DEV, dtype=dtype)  # a copy: the shared cases are read-only


def _np(t):
    return t.cpu().numpy()


# ---- blur ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,sigma", sc.BLUR_CASES)
def test_blur_within_one_step_of_float64(H, W, sigma):
    """|q_dev - q_f64| <= 1 (two f32 passes of at most 129 taps err by about 1e-5, under one step of 1/65535) and at
    most 2 % of the pixels differ -- twice the cap the f32 restatement is held to in test_slic_host.py.  The device
    also equals that f32 restatement wherever host and device round the weights alike; reported, not asserted."""
    from cyhip import ops
    images = sc.blobs(2, H, W, seed=11)
    got = _np(ops.slic_blur_q(_dev(images), sigma)).astype(np.int64)
    d = np.abs(got - sc.blur_q_f64(images, sigma))
    same = np.array_equal(got, sc.blur_q_f32(images, sigma))
    print(f"{H}x{W} sigma {sigma}: max |dq| {d.max()}, {100 * (d > 0).mean():.3f} % differ; "
          f"equals the f32 restatement: {same}")
    assert d.max() <= 1
    assert (d > 0).mean() <= 0.02


def test_blur_accepts_the_channel_axis_and_half_precision():
    from cyhip import ops
    images = sc.blobs(2, 37, 53, seed=12)
    x = _dev(images)
    want = ops.slic_blur_q(x, 1.0)
    assert want.dtype == torch.int32 and want.shape == (2, 37, 53)
    assert torch.equal(ops.slic_blur_q(x[:, None], 1.0), want)
    half = x.to(torch.bfloat16)
    assert torch.equal(ops.slic_blur_q(half, 1.0), ops.slic_blur_q(half.float(), 1.0))
    with pytest.raises(ValueError):
        ops.slic_blur_q(x[:, None].repeat(1, 2, 1, 1), 1.0)


def test_sigma_zero_is_exact():
    from cyhip import ops
    images = sc.noise(3, 37, 53, seed=13)
    images[0, 0, :4] = [-0.5, 1.5, 0.0, 1.0]  # clamped
    got = _np(ops.slic_blur_q(_dev(images), 0.0))
    assert np.array_equal(got, sc.blur_q_f64(images, 0.0))
    assert got[0, 0, :4].tolist() == [0, 65535, 0, 65535]


# ---- cluster, fed the device's own q --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.CASES))
def test_cluster_equals_the_restatement(name):
    from cyhip import ops
    c = sc.CASES[name]
    q = ops.slic_blur_q(_dev(sc.case(name)["images"]), c["sigma"])
    labels, centres = ops.slic_cluster(q, c["n_segments"], c["compactness"])
    want_labels, want_centres = sc.cluster(_np(q).astype(np.int64), c["n_segments"], c["compactness"])
    assert np.array_equal(_np(centres), want_centres)
    assert np.array_equal(_np(labels), want_labels)


def test_cluster_round_counts():
    """max_iter = 0 leaves the grid and the all-zero labels; one round is one assignment and one update"""
    from cyhip import ops
    c = sc.CASES["odd_37x53"]
    q = sc.case("odd_37x53")["q"]
    for rounds in (0, 1, 3):
        labels, centres = ops.slic_cluster(_dev(q, torch.int32), c["n_segments"], c["compactness"], max_iter=rounds)
        want_labels, want_centres = sc.cluster(q, c["n_segments"], c["compactness"], max_iter=rounds)
        assert np.array_equal(_np(labels), want_labels) and np.array_equal(_np(centres), want_centres), rounds


# ---- connect, fed arbitrary label maps ------------------------------------------------------------------------------
def _check_connect(labels, n_segments):
    from cyhip import ops
    ids, count = ops.slic_connect(_dev(labels, torch.int32), n_segments)
    want_ids, want_count = sc.connect(np.asarray(labels), n_segments)
    assert ids.dtype == torch.uint8 and count.dtype == torch.int32
    assert np.array_equal(_np(count), want_count)
    assert np.array_equal(_np(ids), want_ids)
    return want_count


@pytest.mark.parametrize("name", list(sc.CASES))
def test_connect_equals_the_restatement_on_the_cases(name):
    """the label maps of the cases: the noise case (sigma 0, compactness 1e-3) has hundreds of components and long
    merge chains, the constant image only ties"""
    c = sc.case(name)
    if name == "noise_96x160":
        assert len(sc.components(c["labels"][0])[1]) > 300
    _check_connect(c["labels"], c["n_segments"])


def test_connect_on_two_interleaved_spirals():
    """64 x 64, two one-pixel-wide spirals wound into each other: components about 2000 pixels long"""
    assert _check_connect(sc.spirals(), 4).tolist() == [2]
    assert _check_connect(sc.spirals(), 1).tolist() == [1]  # the second spiral is under min_size: joins the first


def test_connect_on_speckle_and_stripes():
    """labels no clustering would give: independent pixels (hundreds of one-pixel components, chains of merges along
    the rows and up column 0), and stripes whose labels are far outside 0 .. K-1"""
    _check_connect(sc.speckle(37, 53, 2, 9), 20)
    _check_connect(sc.speckle(70, 130, 5, 10), 40)
    columns = np.broadcast_to(np.arange(130)[None, None, :] // 7 * 100003 - 7, (1, 70, 130))
    rows = np.broadcast_to(-(np.arange(70)[None, :, None] // 3), (1, 70, 130))
    assert _check_connect(np.concatenate([columns, rows]).astype(np.int32), 40).tolist() == [19, 24]


# ---- all of it ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd_37x53", "tiles_70x130_n5", "one_centre", "noise_96x160", "reference_224"])
def test_slic_is_the_chain_of_its_stages_and_repeats_bit_for_bit(name):
    from cyhip import ops
    c = sc.CASES[name]
    x = _dev(sc.case(name)["images"])
    kw = dict(n_segments=c["n_segments"], sigma=c["sigma"], compactness=c["compactness"])
    ids, count = ops.slic(x, **kw)
    ids2, count2 = ops.slic(x[:, None], **kw)
    assert torch.equal(ids, ids2) and torch.equal(count, count2)
    labels, _ = ops.slic_cluster(ops.slic_blur_q(x, c["sigma"]), c["n_segments"], c["compactness"])
    ids3, count3 = ops.slic_connect(labels, c["n_segments"])
    assert torch.equal(ids, ids3) and torch.equal(count, count3)
    assert int(count.max()) < 207
    assert [int(i.max()) + 1 for i in ids] == count.tolist()


def test_slic_refuses_before_launching():
    from cyhip import _lib, ops
    x = _dev(sc.blobs(1, 37, 53, seed=1))
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_SHAPE"):
        ops.slic(x, n_segments=40)  # K = 40 needs 2560 pixels
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_ARG"):
        ops.slic(x, n_segments=20, compactness=0.0)
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_SHAPE"):
        ops.slic(x, n_segments=20, sigma=10.0)  # r = 40 > 37


# ---- the hook -------------------------------------------------------------------------------------------------------
SLIC_KW = dict(n_segments=16, sigma=2.0, compactness=0.1)


def _model_and_batch(seed):
    from contrastyou.arch import UNet
    from oracle import unet as ou
    g = torch.Generator().manual_seed(seed)
    n, hw, K = 3, 48, 4
    batch = blob_batch(n, hw, K, g)
    batch["img"] = [batch["img"][0], torch.rand(n, 1, hw, hw, generator=g)]
    model = UNet(input_dim=1, num_classes=K, max_channel=256, momentum=0.01)
    model.load_state_dict(ou.init_state_dict(1, K, 256, seed=3))
    return model.to(DEV), batch


def _pretrain_loss(hook_cls, with_map, projector_state=None, **extra):
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.kl import KL_div
    from contrastyou.optim import RAdam
    from cyhip import ops
    from semi_seg.epochers import PretrainDecoderEpocher
    from semi_seg.superpixel import as_batch_entry
    model, batch = _model_and_batch(8)
    if with_map:
        batch["superpixel"] = as_batch_entry(ops.slic(batch["img"][0].to(DEV), **SLIC_KW)[0])
    type(TrainerHook).names.clear()
    hook = hook_cls(name="infonce/Up_conv2/superpixel", model=model, feature_name="Up_conv2", weight=1.0,
                    spatial_size=(6, 6), data_name="acdc", contrast_on="self", **extra).to(DEV)
    if projector_state is not None:
        hook._projector.load_state_dict(projector_state)
    state = {k: v.detach().clone() for k, v in hook._projector.state_dict().items()}
    opt = RAdam([{"params": list(model.parameters())}, {"params": list(hook.parameters())}], lr=1e-3)
    ep = PretrainDecoderEpocher(model=model, optimizer=opt, labeled_loader=Loader([batch]),
                                unlabeled_loader=Loader([batch]), sup_criterion=KL_div(), num_batches=1, cur_epoch=0,
                                device=DEV, two_stage=False, disable_bn=False, chain_dataloader=[batch],
                                inference_until="Up_conv2", scaler=torch.amp.GradScaler("cuda", enabled=False),
                                accumulate_iter=1)
    ep.init()
    random.seed(3)
    with ep.register_hook(hook()):
        ep.run()
    torch.cuda.synchronize()
    return ep.get_metric()["infonce/Up_conv2/superpixel"]["loss"], state, batch


def test_online_hook_equals_the_offline_hook_fed_the_same_map():
    """under PretrainDecoderEpocher, OnlineSuperPixelInfoNCEHook on a batch without "superpixel" gives bit for bit the
    loss of SuperPixelInfoNCEHook fed as_batch_entry(ops.slic(unlabeled_image)[0]); a batch that carries a map is
    used as it is"""
    from semi_seg.hooks import OnlineSuperPixelInfoNCEHook, SuperPixelInfoNCEHook
    want, state, batch = _pretrain_loss(SuperPixelInfoNCEHook, with_map=True)
    ids = (batch["superpixel"][0] * 255.0).type(torch.uint8)
    assert ids.shape == (3, 1, 48, 48) and len(ids.unique()) > 8  # a real map: the labels are not all alike
    got, _, _ = _pretrain_loss(OnlineSuperPixelInfoNCEHook, with_map=False, projector_state=state, **SLIC_KW)
    assert np.isfinite(want) and got == want, (got, want)
    # other parameters, another map, another loss -- unless the batch brings its own map
    other, _, _ = _pretrain_loss(OnlineSuperPixelInfoNCEHook, with_map=False, projector_state=state, n_segments=4,
                                 sigma=2.0, compactness=0.1)
    assert other != want
    own, _, _ = _pretrain_loss(OnlineSuperPixelInfoNCEHook, with_map=True, projector_state=state, n_segments=4,
                               sigma=2.0, compactness=0.1)
    assert own == want


def _semi_step(batch_unl, model, batch_lab):
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.kl import KL_div
    from contrastyou.optim import RAdam
    from semi_seg.epochers import SemiSupervisedEpocher
    from semi_seg.hooks import OnlineSuperPixelInfoNCEHook
    type(TrainerHook).names.clear()
    hook = OnlineSuperPixelInfoNCEHook(name="infonce/Up_conv2/online", model=model, feature_name="Up_conv2", weight=0.5,
                                       spatial_size=(6, 6), data_name="acdc", contrast_on="self", **SLIC_KW).to(DEV)
    opt = RAdam([{"params": list(model.parameters())}, {"params": list(hook.parameters())}], lr=1e-3)
    ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=Loader([batch_lab]),
                               unlabeled_loader=Loader([batch_unl]), sup_criterion=KL_div(), num_batches=1, cur_epoch=0,
                               device=DEV, two_stage=True, disable_bn=False,
                               scaler=torch.amp.GradScaler("cuda", enabled=False), accumulate_iter=1)
    ep.init()
    random.seed(5)
    with ep.register_hook(hook()):
        ep.run()
    torch.cuda.synchronize()
    return ep.get_metric(), hook


def test_online_hook_trains_a_step_inside_the_semi_supervised_epocher():
    """SemiSupervisedEpocher hands its hooks no batch_data: the map comes from unlabeled_image"""
    model, batch = _model_and_batch(9)
    before = [p.detach().clone() for p in model.parameters()]
    stats, hook = _semi_step(batch, model, batch)
    loss = stats["infonce/Up_conv2/online"]["loss"]
    assert np.isfinite(loss) and loss > 0
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    assert all(torch.isfinite(p).all() for p in hook._projector.parameters())


def test_online_hook_refuses_a_two_channel_image():
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from semi_seg.hooks import OnlineSuperPixelInfoNCEHook
    model = UNet(input_dim=1, num_classes=4, max_channel=256).to(DEV)
    type(TrainerHook).names.clear()
    hook = OnlineSuperPixelInfoNCEHook(name="infonce/Up_conv2/two", model=model, feature_name="Up_conv2", weight=1.0,
                                       spatial_size=(6, 6), data_name="acdc", contrast_on="self").to(DEV)
    epoch_hook = hook()
    try:
        with pytest.raises(ValueError, match="single-channel"):
            epoch_hook._call_implementation(unlabeled_image=torch.rand(3, 2, 48, 48, device=DEV))
    finally:
        epoch_hook.close()
