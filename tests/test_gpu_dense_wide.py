"""The streamed matrix-core form of the dense projector (csrc/cy_dense_wide.h): 16-bit maps with 256 or 512 channels --
`Up_conv5` at max_channel 512, `Up_conv5` / `Up_conv4` at max_channel 1024.  Method of
test_dense_projector_matrix_core_kernels (tests/test_gpu_next_rows.py): W1 and x are representable in the storage type,
the reference is the oracle's conv -> lrelu -> conv -> pool -> normalise on the CPU, all bins and a bin list, and the
forward and the backward are repeated and compared bit for bit.  Every case first asks the host-side plan that it runs
the streamed form (forward and dx on the matrix cores; dW1 / db1 of these maps on the VALU kernel): a silent fall back
to the VALU kernels for everything fails here instead of passing.

Tolerances are that test's: z 1e-4 (exact products, f32 sums), dx 1e-2 and parameter gradients 3e-3 (the pooled
gradient is rounded to 16 bits before the dx product, dx is stored in 16 bits).  The lengths of the sums over
pixels and over hidden units do not grow with C, and the channel sum is exact products accumulated in f32."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16


def cpu(t):
    return t.detach().float().cpu()


def close(a, b, rel, what):
    a, b = cpu(a).double(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = b.abs().max().item() + 1e-30
    err = (a - b).abs().max().item()
    print(f"{what}: max err {err:.3e} = {err / scale:.2e} of {scale:.3e} (bound {rel:.0e})")
    assert err <= rel * scale, f"{what}: max err {err:.3e} > {rel:.1e} * {scale:.3e}"


def nhwc(t, dtype):
    return t.to(dtype).to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def assert_streamed(cin, hid, dtype):
    from cyhip import _lib, ops
    p = ops.dense_proj_plan(cin, hid, dtype)
    assert p["form"] == _lib.CY_DENSE_PROJ_MFMA_STREAM, p
    return p


def _head(cin, hid, out, s, dtype, seed=11):
    from contrastyou.projectors.heads import DenseProjectionHead
    from oracle import losses as ol
    sd = ol.init_dense_projector_sd(cin, hid, out, seed=seed)
    sd["_projector.0.weight"] = sd["_projector.0.weight"].to(dtype).float()
    head = DenseProjectionHead(input_dim=cin, hidden_dim=hid, output_dim=out, head_type="mlp", normalize=True,
                               spatial_size=(s, s))
    head.load_state_dict(sd, strict=True)
    return head.to(DEV), sd


@pytest.mark.parametrize("n,hw,s,hid,dtype,cin", [
    (2, 28, 14, 256, BF16, 256),  # the Up_conv5 geometry: H % s == 0, two-pixel bins, no shared pixels, odd cell segments empty
    (3, 45, 8, 128, F16, 256),    # ragged bins, shared rows and columns
    (5, 56, 20, 256, BF16, 256),  # 7605 cells on the dx kernel's 1024 waves (one workgroup per CU): 7-8 jobs per wave
    (1, 33, 32, 128, BF16, 256),  # bins of one and two pixels
    (2, 14, 7, 256, BF16, 512),   # C = 512: two forward passes over the hidden units, W1 of the dx kernel from the workspace
    (3, 20, 6, 128, F16, 512),    # C = 512, ragged bins
])
def test_dense_projector_streamed_kernels(n, hw, s, hid, dtype, cin):
    from oracle import losses as ol
    plan = assert_streamed(cin, hid, dtype)
    assert plan["channel_blocks"] == cin // 32
    if cin == 512 and hid == 256:
        assert plan["fwd_passes"] > 1
    gen = torch.Generator().manual_seed(hw + s)
    out = 64
    head, sd = _head(cin, hid, out, s, dtype)
    x = torch.randn(n, cin, hw, hw, generator=gen).to(dtype).float()
    coef = torch.randn(n, out, s, s, generator=gen)

    xa = nhwc(x, dtype).requires_grad_(True)
    z = head(xa)
    (z * coef.to(DEV)).sum().backward()
    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    zo = ol.dense_projection_head(osd, xo, (s, s))
    (zo * coef).sum().backward()
    close(z, zo, 1e-4, "z")
    close(xa.grad, xo.grad, 1e-2, "dx")
    for k, p in head.named_parameters():
        close(p.grad, osd[k].grad, 3e-3, k)
    # run to run: bit-identical (fixed job -> wave assignment, fixed reduction order); the forward alone eight times
    # (its C = 256 kernel runs two workgroups per CU), then forward + backward three times
    with torch.no_grad():
        for _ in range(8):
            assert torch.equal(head(xa), z), "z differs between runs"
    first = {k: p.grad.clone() for k, p in head.named_parameters()}
    dx_first = xa.grad.clone()
    for _ in range(3):
        head.zero_grad()
        xr = nhwc(x, dtype).requires_grad_(True)
        (head(xr) * coef.to(DEV)).sum().backward()
        assert torch.equal(xr.grad, dx_first), "dx differs between runs"
        for k, p in head.named_parameters():
            assert torch.equal(p.grad, first[k]), f"{k} differs between runs"

    # a bin list: a 2 x 3 patch of neighbouring bins of image 0 (all four colour classes) plus the last bin of the last
    # image
    per_image = [[] for _ in range(n)]
    per_image[0] = [(i, j) for i in (1, 2) for j in (0, 1, 2)]
    per_image[n - 1] = per_image[n - 1] + [(s - 1, s - 1)]
    pts = [(b, i, j) for b, lst in enumerate(per_image) for i, j in lst]
    cr = torch.randn(len(pts), out, generator=gen)

    def listed():
        head.zero_grad()
        xb = nhwc(x, dtype).requires_grad_(True)
        rows = head.project_points(xb, per_image)
        (rows * cr.to(DEV)).sum().backward()
        return rows, xb.grad, {k: p.grad.clone() for k, p in head.named_parameters()}

    rows, dxb, gb = listed()
    for v in osd.values():
        v.grad = None
    xo2 = x.clone().requires_grad_(True)
    zo2 = ol.dense_projection_head(osd, xo2, (s, s))
    ro = torch.stack([zo2[b, :, i, j] for b, i, j in pts])
    (ro * cr).sum().backward()
    close(rows, ro, 1e-4, "rows")
    close(dxb, xo2.grad, 1e-2, "dx (bin list)")
    for k in gb:
        close(gb[k], osd[k].grad, 3e-3, k + " (bin list)")
    for _ in range(3):
        _, dxr, gr = listed()
        assert torch.equal(dxr, dxb), "dx (bin list) differs between runs"
        for k in gb:
            assert torch.equal(gr[k], gb[k]), f"{k} (bin list) differs between runs"


def test_dense_hook_points_on_a_256_channel_tap():
    """what the dense InfoNCE hook does with `Up_conv5` at max_channel 512: five seeded points per image of the 7 x 7
    grid of a [4, 256, 14, 14] bf16 map.  project_points against the oracle's region_extractor(head(features)), and
    against forward() at the same bins."""
    from oracle import losses as ol
    from oracle import next_rows as onr
    from semi_seg.hooks.infonce import region_extractor, region_points
    n, cin, hw, s, hid, out, dtype = 4, 256, 14, 7, 256, 256, BF16
    assert_streamed(cin, hid, dtype)
    gen = torch.Generator().manual_seed(21)
    head, sd = _head(cin, hid, out, s, dtype, seed=5)
    x = torch.randn(n, cin, hw, hw, generator=gen).to(dtype).float()
    seed = 77
    pts = region_points(n, s, s, point_nums=5, seed=seed)
    assert pts == onr.region_points(n, s, s, seed)
    coef = torch.randn(n * 5, out, generator=gen)

    xa = nhwc(x, dtype).requires_grad_(True)
    rows = head.project_points(xa, pts)
    (rows * coef.to(DEV)).sum().backward()
    ga = {k: p.grad.clone() for k, p in head.named_parameters()}
    head.zero_grad()

    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    ro = onr.region_extractor(ol.dense_projection_head(osd, xo, (s, s)), seed)
    (ro * coef).sum().backward()
    close(rows, ro, 1e-4, "rows vs oracle")
    close(xa.grad, xo.grad, 1e-2, "dx vs oracle")
    for k in osd:
        close(ga[k], osd[k].grad, 3e-3, k + " vs oracle")

    xb = nhwc(x, dtype).requires_grad_(True)
    rows_full = region_extractor(head(xb), point_nums=5, seed=seed)
    (rows_full * coef.to(DEV)).sum().backward()
    close(rows, cpu(rows_full), 1e-5, "points vs full map")
    close(xa.grad, cpu(xb.grad), 1e-2, "dx points vs full map")
    for k, p in head.named_parameters():
        close(ga[k], cpu(p.grad), 1e-3, k + " points vs full map")
