"""The surface-distance kernels (csrc/cy_surface.hip), `ops.surface_stats`, `SurfaceMeter` and the "ASD" meter of
`InferenceEpocher` against two oracles:

  * tests/golden/surface.npz -- the reference's own SurfaceMeter over a scipy.ndimage stand-in of medpy
    (tests/golden/gen_goldens_surface.py): per-(volume, class) ASD / HD / HD95, summaries, skipped volumes, and for
    the small cases the border masks and int32 squared-distance maps of both directions;
  * a brute-force oracle of this file that uses neither scipy nor those maps: border sets by a pad-and-shift
    neighbour test in torch, squared distances by the minimum over all (voxel, border voxel) pairs on the CPU.

Maps are compared as integers, everywhere, with no tolerance.  HD is the square root of an integer on both sides and
must be equal.  ASD and HD95 have bit-equal, non-negative terms on both sides and differ in the order of summation
only: a 256-long serial partial plus a tree is bounded by about 300 * 2^-53 = 3e-14 relative, numpy's pairwise mean by
less; the bound asserted is 1e-12.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL = 1e-12
NO_BORDER = 1 << 30
CLASSES = [1, 2, 3]
SMALL = ["d1", "flat", "line1", "hlong", "wlong", "h130", "h257"]
SHAPES = {"d1": (1, 9, 13), "flat": (9, 13), "line1": (2, 1, 5), "hlong": (3, 67, 5), "wlong": (5, 33, 70),
          "h130": (4, 130, 3), "h257": (2, 257, 3), "pair": (3, 20, 24), "large": (5, 230, 230)}
METERS = {"asd": "average_surface", "hd": "hausdorff", "mhd": "mod_hausdorff"}


@pytest.fixture(scope="module")
def fx(golden_dir):
    g = np.load(golden_dir / "surface.npz")
    data = {k: g[k] for k in g.files}
    for tag, shape in SHAPES.items():
        assert data[f"{tag}_pred"].shape[1:] == shape and data[f"{tag}_pred"].dtype == np.uint8, tag
    assert data["large_pred"][0].size >= 262145
    return data


def volume(fx, tag, b=0):
    return (torch.from_numpy(fx[f"{tag}_pred"][b]).long().to(DEV), torch.from_numpy(fx[f"{tag}_target"][b]).long().to(DEV))


def ndim_of(tag):
    return len(SHAPES[tag])


# ---------------------------------------------------------------------------------------------- brute-force oracle
def brute_border(mask: torch.Tensor) -> torch.Tensor:
    """mask & ~(every face neighbour in mask), background outside; every axis of `mask` is tested"""
    dims = range(mask.dim())
    padded = torch.nn.functional.pad(mask.to(torch.uint8), [1, 1] * mask.dim(), value=0).bool()
    inside = mask.clone()
    for ax in dims:
        for lo in (0, 2):  # the neighbour below and the neighbour above along `ax`
            inside &= padded[tuple(slice(lo if a == ax else 1, (lo if a == ax else 1) + mask.shape[a]) for a in dims)]
    return mask & ~inside


def brute_d2(border_b: torch.Tensor) -> torch.Tensor:
    """int32 map: min over the border voxels u of |v - u|^2 for every voxel v (f64 products of small integers: exact)"""
    shape = border_b.shape
    every = torch.stack(torch.meshgrid(*[torch.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, len(shape))
    u = every[border_b.reshape(-1)].double()
    if len(u) == 0:
        return torch.full(shape, NO_BORDER, dtype=torch.int32)
    v = every.double()
    out = torch.empty(len(v), dtype=torch.float64)
    for i in range(0, len(v), 4096):
        c = v[i:i + 4096]
        out[i:i + 4096] = ((c * c).sum(1)[:, None] + (u * u).sum(1)[None] - 2 * c @ u.T).min(1).values
    return out.to(torch.int32).reshape(shape)


_BRUTE = {}


def brute(fx, tag, b=0, pred=None, target=None):
    """(border uint8 [2, 3, *shape], d2 int32 [2, 3, *shape], values {meter: f64 [3], NaN where a side is empty})"""
    key = (tag, b)
    if pred is None and key in _BRUTE:
        return _BRUTE[key]
    p = torch.from_numpy(fx[f"{tag}_pred"][b] if pred is None else pred).long()
    t = torch.from_numpy(fx[f"{tag}_target"][b] if target is None else target).long()
    border = torch.zeros((2, 3) + tuple(p.shape), dtype=torch.uint8)
    d2 = torch.zeros((2, 3) + tuple(p.shape), dtype=torch.int32)
    values = {k: np.full(3, np.nan) for k in METERS}
    for r, c in enumerate(CLASSES):
        edges = [brute_border(p == c), brute_border(t == c)]
        for d in (0, 1):
            border[d, r] = edges[d]
            d2[d, r] = brute_d2(edges[1 - d])
        if edges[0].any() and edges[1].any():
            sd = [np.sqrt(d2[d, r][edges[d]].numpy().astype(np.float64)) for d in (0, 1)]
            values["asd"][r] = np.mean((sd[0].mean(), sd[1].mean()))
            values["hd"][r] = max(sd[0].max(), sd[1].max())
            values["mhd"][r] = max(np.percentile(sd[0], 95), np.percentile(sd[1], 95))
    res = (border, d2, values)
    if pred is None:
        _BRUTE[key] = res
    return res


def check_value(what, got, want, exact=False):
    print(f"{what}: got {got!r} want {want!r} rel {abs(got - want) / abs(want) if want == want and want else 0.0:.3e}")
    if want != want:
        assert got != got, what
    elif exact:
        assert got == want, what
    else:
        assert abs(got - want) <= REL * abs(want), what


# ---------------------------------------------------------------------------------------------- maps
def test_fixture_holds_an_empty_class_and_the_depth_one_rule(fx):
    assert fx["line1_skipped"].tolist() == [1] and np.isnan(fx["line1_asd"]).sum() == 2
    # depth 1 as 3-D: every object voxel is border; the same labels as 2-D have interior voxels
    assert np.array_equal(fx["d1_border"][0, :, 0], np.stack([fx["d1_pred"][0, 0] == c for c in CLASSES]))
    assert fx["flat_border"].sum() < fx["d1_border"].sum()


@pytest.mark.parametrize("tag", SMALL)
def test_maps_equal_the_fixture_and_the_brute_force_oracle(fx, tag):
    from cyhip import ops
    p, t = volume(fx, tag)
    count, total, maxd2, d2, border = ops.surface_stats(p, t, CLASSES, ndim=ndim_of(tag), maps=True)
    shape = SHAPES[tag] if ndim_of(tag) == 3 else (1,) + SHAPES[tag]
    assert tuple(d2.shape) == tuple(border.shape) == (2, 3) + shape
    assert d2.dtype == torch.int32 and border.dtype == torch.uint8
    d2, border = d2.cpu().reshape((2, 3) + SHAPES[tag]), border.cpu().reshape((2, 3) + SHAPES[tag])
    b_bf, d2_bf, _ = brute(fx, tag)
    for name, want_b, want_d in (("fixture", torch.from_numpy(fx[f"{tag}_border"]), torch.from_numpy(fx[f"{tag}_d2"])),
                                 ("brute force", b_bf, d2_bf)):
        print(f"{tag} vs {name}: border voxels {int(border.sum())} / {int(want_b.sum())}, border mismatches "
              f"{int((border != want_b).sum())}, d2 mismatches {int((d2 != want_d).sum())}, d2 max {int(d2.max())}")
        assert torch.equal(border, want_b), (tag, name)
        assert torch.equal(d2, want_d), (tag, name)
    # the scalar outputs are the reductions of those maps
    count, total, maxd2 = count.cpu(), total.cpu(), maxd2.cpu()
    for d in (0, 1):
        for r in range(3):
            on = border[d, r].bool()
            assert int(count[d, r]) == int(on.sum()), (tag, d, r)
            assert int(maxd2[d, r]) == (int(d2[d, r][on].max()) if on.any() else 0), (tag, d, r)
            want = float(np.sqrt(d2[d, r][on].numpy().astype(np.float64)).sum())
            check_value(f"{tag} sum[{d}][{r}]", float(total[d, r]), want)
    if tag == "line1":
        assert (count == 0).any() and (d2 == NO_BORDER).any()


def test_stats_without_maps_equal_stats_with_maps(fx):
    from cyhip import ops
    p, t = volume(fx, "wlong")
    with_maps = ops.surface_stats(p, t, CLASSES, maps=True)
    without = ops.surface_stats(p, t, CLASSES)
    assert len(without) == 3
    for a, b in zip(without, with_maps):
        assert torch.equal(a, b)
    # a single class, and the classes in another order
    one = ops.surface_stats(p, t, [2])
    rev = ops.surface_stats(p, t, [3, 2, 1])
    for a, b, c in zip(one, rev, without):
        assert torch.equal(a[:, 0], c[:, 1]) and torch.equal(b.flip(1), c)


# ---------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("tag", list(SHAPES))
def test_values_equal_the_references(fx, tag):
    """per (volume, class): one meter per class, so that an empty class drops nothing but itself"""
    from contrastyou.meters import SurfaceMeter
    B = len(fx[f"{tag}_pred"])
    for key, metername in METERS.items():
        for b in range(B):
            p, t = volume(fx, tag, b)
            for r, c in enumerate(CLASSES):
                m = SurfaceMeter(C=4, report_axises=[c], metername=metername)
                m.add(p[None], t[None])
                want = float(fx[f"{tag}_{key}"][b, r])
                got = float(m.value()[0][0])
                check_value(f"{tag}[{b}] {key} class {c}", got, want, exact=key == "hd")
                assert m.skipped == int(want != want)
                if tag in SMALL:
                    check_value(f"{tag}[{b}] {key} class {c} (brute force)", got, float(brute(fx, tag, b)[2][key][r]),
                                exact=key == "hd")


@pytest.mark.parametrize("tag", list(SHAPES))
def test_summaries_equal_the_references(fx, tag):
    """the meter as the epocher uses it: classes 1..3 together, every volume of the case in one add"""
    from contrastyou.meters import SurfaceMeter
    p = torch.from_numpy(fx[f"{tag}_pred"]).long().to(DEV)
    t = torch.from_numpy(fx[f"{tag}_target"]).long().to(DEV)
    for key, metername in METERS.items():
        m = SurfaceMeter(C=4, report_axises=[1, 2, 3], metername=metername)
        m.add(p, t)
        s = m.summary()
        ab = SurfaceMeter.abbr[metername]
        assert list(s) == [f"{ab}1", f"{ab}2", f"{ab}3", f"{ab}_mean"]
        for name, want in zip(s, fx[f"{tag}_sum_{key}"]):
            check_value(f"{tag} summary {name}", s[name], float(want), exact=key == "hd" and name != f"{ab}_mean")
        assert m.skipped == int(fx[f"{tag}_skipped"].sum())
        means, stds = m.value()
        assert len(means) == (3 if m.skipped < len(p) else 4)


def test_simplex_prediction_with_one_hot_target(fx):
    from contrastyou.meters import SurfaceMeter
    p, t = volume(fx, "wlong")
    onehot_t = torch.nn.functional.one_hot(t[None], 4).movedim(-1, 1)
    simplex_p = torch.nn.functional.one_hot(p[None], 4).movedim(-1, 1).float() * 0.7 + 0.1
    m = SurfaceMeter(C=4, report_axises=[1, 2, 3], metername="average_surface")
    m.add(simplex_p, onehot_t)
    for r in range(3):
        check_value(f"simplex class {r + 1}", float(m.value()[0][r]), float(fx["wlong_asd"][0, r]))


def test_the_three_functions(fx):
    from contrastyou.meters import average_surface_distance, hausdorff_distance, mod_hausdorff_distance
    for tag in ("flat", "hlong"):
        p, t = volume(fx, tag)
        check_value(f"{tag} assd", average_surface_distance(p == 2, t == 2), float(fx[f"{tag}_asd"][0, 1]))
        check_value(f"{tag} hd", hausdorff_distance(p == 2, t == 2), float(fx[f"{tag}_hd"][0, 1]), exact=True)
        check_value(f"{tag} hd95", mod_hausdorff_distance(p == 2, t == 2), float(fx[f"{tag}_mhd"][0, 1]))
    p, t = volume(fx, "line1")
    assert np.isnan(fx["line1_asd"][0, 0])
    with pytest.raises(RuntimeError, match="does not contain any binary object"):
        average_surface_distance(p == 1, t == 1)


# ---------------------------------------------------------------------------------------------- skip rule
def test_a_volume_with_an_empty_class_is_dropped_whole(fx):
    from contrastyou.meters import SurfaceMeter
    p = torch.from_numpy(fx["pair_pred"]).long().to(DEV)
    t = torch.from_numpy(fx["pair_target"]).long().to(DEV)
    assert len(p) == 2 and not (p[1] == 2).any() and (t[1] == 2).any() and (p[0] == 2).any()
    for key, metername in METERS.items():
        m = SurfaceMeter(C=4, report_axises=[1, 2, 3], metername=metername)
        m.add(p, t)  # one add, two volumes
        means, stds = m.value()
        assert m.skipped == 1 and len(m._mhd) == 1 and len(means) == 3
        for r in range(3):
            check_value(f"pair {key} class {r + 1}", float(means[r]), float(fx[f"pair_{key}"][0, r]), exact=key == "hd")
            assert float(stds[r]) == 0.0
        assert m.value()[0].tolist() == means.tolist() and m.skipped == 1  # reading twice changes nothing
        m.reset()
        assert m.skipped == 0 and math.isnan(m.summary()[f"{SurfaceMeter.abbr[metername]}_mean"])


# ---------------------------------------------------------------------------------------------- determinism
def test_two_runs_of_the_large_case_give_the_same_bits(fx):
    from cyhip import ops
    p, t = volume(fx, "large")
    assert -(-p.numel() // 256) > 1024  # more blocks of 256 than the partial-sum grid has
    first = ops.surface_stats(p, t, CLASSES, maps=True)
    second = ops.surface_stats(p, t, CLASSES, maps=True)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert first[1].view(torch.int64).equal(second[1].view(torch.int64))
    assert (first[0] > 0).all()


# ---------------------------------------------------------------------------------------------- epocher
def _noisy_classes_from_intensity(module, inputs, logits):
    """forward hook: `blob_batch` images are class / 3 * 0.8 + 0.1 * u, u in [0, 1); thresholds 0.06 above each level send
    the pixels with u >= 0.6 to the next class, so the arg-max holds every class and differs from the target"""
    cls = ((inputs[0][:, 0] - 0.06) / (0.8 / 3)).floor().long().add(1).clamp(0, 3)
    return logits + 40.0 * torch.nn.functional.one_hot(cls, 4).movedim(-1, 1).to(logits.dtype)


@pytest.mark.parametrize("hooked", [False, True])
def test_inference_epocher_reports_asd(tmp_path, hooked):
    """the tiny U-Net and loader of tests/test_gpu_round2_rows.py::test_inference_epocher_writes_predictions, with a file
    name per image so that every prediction is kept.  The untrained network predicts one class, so that epoch only
    takes the skip path; `hooked` adds an intensity-dependent term to its logits, which makes every class appear."""
    from contrastyou.arch import UNet
    from contrastyou.losses.kl import KL_div
    from oracle import unet as ou
    from semi_seg.epochers import EvalEpocher, InferenceEpocher
    from tests.test_gpu_hooks_dice import Loader, blob_batch
    g = torch.Generator().manual_seed(8)
    sd = ou.init_state_dict(1, 4, 128, seed=2)
    model = UNet(input_dim=1, num_classes=4, max_channel=128, momentum=0.01)
    model.load_state_dict(sd)
    model.to(DEV)
    if hooked:
        model.register_forward_hook(_noisy_classes_from_intensity)
    batches = []
    for k in range(2):
        b = blob_batch(3, 32, 4, g, views=1)
        batches.append({"img": b["img"][0], "gt": b["gt"][0], "filename": [f"b{k}_{n}" for n in b["filename"][0]],
                        "partition": b["partition"][0], "scan_num": b["scan_num"][0]})
    kw = dict(model=model, loader=Loader(batches), sup_criterion=KL_div(), device=DEV,
              scaler=torch.amp.GradScaler("cuda", enabled=False), accumulate_iter=1)
    ev = EvalEpocher(**kw)
    ev.init()
    ev.run()
    inf = InferenceEpocher(enable_prediction_saver=True, save_dir=str(tmp_path), **kw)
    inf.init()
    inf.run()
    assert abs(inf.get_score() - ev.get_score()) < 1e-12
    stats = inf.get_metric()["infer"]
    assert list(stats["ASD"]) == ["ASD1", "ASD2", "ASD3", "ASD_mean"]
    assert "ASD" not in ev.get_metric()["eval"]
    # the oracle on what the epoch saved: each batch is one [3, 32, 32] volume
    rows, skipped = [], 0
    for k, batch in enumerate(batches):
        pred = np.stack([np.load(tmp_path / "predictions" / f"b{k}_f{i}.npy") for i in range(3)])
        vals = brute(None, f"epoch{k}", pred=pred.astype(np.int64), target=batch["gt"][:, 0].numpy())[2]["asd"]
        print(f"batch {k}: predicted classes {np.unique(pred).tolist()}, oracle ASD {vals.tolist()}")
        if np.isnan(vals).any():
            skipped += 1
        else:
            rows.append(vals)
    assert inf.meters["ASD"].skipped == skipped
    assert skipped == (0 if hooked else 2)
    want = np.mean(rows, axis=0) if rows else np.full(3, np.nan)
    for r in range(3):
        check_value(f"epoch ASD{r + 1}", stats["ASD"][f"ASD{r + 1}"], float(want[r]))
    check_value("epoch ASD_mean", stats["ASD"]["ASD_mean"], float(np.mean(want)))
