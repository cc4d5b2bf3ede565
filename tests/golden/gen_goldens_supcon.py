#!/usr/bin/env python3
"""Generate tests/golden/supcon_masks.npz: the REFERENCE's SupConLoss1 (contrastyou/losses/contrastive.py:23-100) with an
explicit `mask=`, exclude_other_pos False and True, evaluated on the CPU in f64 on seeded inputs.

    python tests/golden/gen_goldens_supcon.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers.

n = 70 pairs of unit-norm embeddings of width 16: R = 140 rows span three 64-row tiles of the fused kernels and the
fold `row - n` crosses a tile boundary inside the second one.  Five masks [n][n] (int8), the reference reads them as
1 = positive, 0 = negative, anything else = neither, and never transposes them:

    a  symmetric, binary                         b  asymmetric, binary, density about 0.2
    c  symmetric, values in {0, 1, -1}           d  asymmetric, values in {0, 1, -1, 2}
    z  asymmetric, binary, ZERO diagonal (the two views of a sample are no positive pair); every row keeps a positive

a-d have an all-ones diagonal, so every row has a positive.  Per case: `<c>_mask`, `<c>_pos` / `<c>_neg` (the
reference's 2n x 2n masks, uint8) and per exclude_other_pos e in {0, 1} `<c>_e<e>_loss`, `_dz1`, `_dz2`; for d also
`d_sim_logits`, `d_sim_exp`.  Losses are stored in f64, gradients and matrices rounded to f32 (6e-8 of their size).
The archive is written with fixed member dates: running this again reproduces the committed file byte for byte.
"""
import io
import sys
import zipfile
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import gen_goldens as gg  # noqa: E402

OUT = Path(__file__).resolve().parent / "supcon_masks.npz"
N, D, T = 70, 16, 0.07
CASES = ("a", "b", "c", "d", "z")


def make_masks():
    g = torch.Generator().manual_seed(521)
    eye = torch.eye(N, dtype=torch.bool)
    r = lambda p: torch.rand(N, N, generator=g) < p  # noqa: E731
    sym = r(0.1)
    sym = sym | sym.t() | eye
    asym = r(0.2) | eye
    a = sym.to(torch.int8)
    b = asym.to(torch.int8)
    ign = r(0.08)
    ign = (ign | ign.t()) & ~sym
    c = a.clone()
    c[ign] = -1
    d = (r(0.2) | eye).to(torch.int8)
    d[r(0.12) & ~eye] = -1
    d[r(0.10) & ~eye] = 2
    z = (r(0.2) & ~eye).to(torch.int8)
    masks = dict(a=a, b=b, c=c, d=d, z=z)
    # what each case is there for
    for k in ("a", "c"):
        assert torch.equal(masks[k], masks[k].t()), k
    for k in ("b", "d", "z"):
        assert not torch.equal(masks[k] == 1, (masks[k] == 1).t()), k
    assert not torch.equal(d == 0, (d == 0).t())
    assert set(a.unique().tolist()) == {0, 1} and set(b.unique().tolist()) == {0, 1} and set(z.unique().tolist()) == {0, 1}
    assert set(c.unique().tolist()) == {-1, 0, 1} and set(d.unique().tolist()) == {-1, 0, 1, 2}
    for k in ("a", "b", "c", "d"):
        assert bool((masks[k].diagonal() == 1).all()), k
    assert bool((z.diagonal() == 0).all())
    assert 0.15 < float((b == 1).float().mean()) < 0.25
    return masks


def write_npz(path, arrays):
    """np.savez_compressed with the members' dates pinned (zipfile stamps the wall clock otherwise)"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    scratch = gg.setup_reference()
    from contrastyou.losses.contrastive import SupConLoss1

    g = torch.Generator().manual_seed(520)
    z1 = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1)
    z2 = torch.nn.functional.normalize(z1 + 0.4 * torch.randn(N, D, generator=g), dim=1)
    out = {"z1": z1.numpy(), "z2": z2.numpy(), "t": np.float64(T)}
    masks = make_masks()
    off = ~torch.eye(2 * N, dtype=torch.bool)
    for c in CASES:
        m = masks[c]
        out[f"{c}_mask"] = m.numpy()
        for excl in (0, 1):
            a = z1.double().clone().requires_grad_(True)
            b = z2.double().clone().requires_grad_(True)
            crit = SupConLoss1(temperature=T, exclude_other_pos=bool(excl))
            loss = crit(a, b, mask=m)
            loss.backward()
            pos, neg = crit.pos_mask, crit.neg_mask
            assert float(pos.sum(1).min()) >= 1, (c, "a row without a positive")
            assert torch.equal(pos.bool(), (m == 1).repeat(2, 2) & off) and torch.equal(neg.bool(), (m == 0).repeat(2, 2) & off)
            out[f"{c}_e{excl}_loss"] = np.float64(loss.item())
            out[f"{c}_e{excl}_dz1"], out[f"{c}_e{excl}_dz2"] = (x.grad.numpy().astype(np.float32) for x in (a, b))
            out[f"{c}_pos"], out[f"{c}_neg"] = pos.numpy().astype(np.uint8), neg.numpy().astype(np.uint8)
            if c == "d" and not excl:
                out["d_sim_logits"] = crit.sim_logits.detach().numpy().astype(np.float32)
                out["d_sim_exp"] = crit.sim_exp.detach().numpy().astype(np.float32)
    write_npz(OUT, out)
    print(f"{OUT}: {OUT.stat().st_size} bytes")
    for c in CASES:
        print(f"  {c}: loss {float(out[c + '_e0_loss']):.6f}  exclude_other_pos {float(out[c + '_e1_loss']):.6f}  "
              f"positives/row {int(out[c + '_pos'].sum(1).min())}..{int(out[c + '_pos'].sum(1).max())}  "
              f"neither {int((2 * N) ** 2 - 2 * N - out[c + '_pos'].sum() - out[c + '_neg'].sum())}")
    del scratch


if __name__ == "__main__":
    main()
