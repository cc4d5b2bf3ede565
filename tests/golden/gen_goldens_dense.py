#!/usr/bin/env python3
"""Generate tests/golden/dense_options.npz: the REFERENCE's DenseProjectionHead without pooling
(pool_name "identical" / "none") for both head types, with and without normalisation, evaluated on the CPU in f64 on
seeded inputs: the output map and every gradient of sum(out * coef).

    python tests/golden/gen_goldens_dense.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers.
Shapes: 2 x 16 x 7 x 9 features, 32 hidden units, 24 outputs.  The features are stored quantised (int8 / 32: exact in
f32, bf16 and f16); weights, coefficients and the f64 results are stored as f32.
"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gen_goldens as gg  # noqa: E402

OUT = Path(__file__).resolve().parent / "dense_options.npz"
POOLS, HEADS, NORMS = ("identical", "none"), ("mlp", "linear"), (True, False)


def f32(t):
    return t.detach().to(torch.float32).numpy()


def main():
    scratch = gg.setup_reference()
    from contrastyou.projectors.heads import DenseProjectionHead

    out = {}
    gen = torch.Generator().manual_seed(501)
    feat = torch.randn(2, 16, 7, 9, generator=gen).mul(32).round().clamp(-128, 127).to(torch.int8)
    out["feat_i8d32"] = feat.numpy()
    x = feat.double() / 32
    for pool in POOLS:
        for head_type in HEADS:
            for normalize in NORMS:
                tag = f"{pool}_{head_type}_{int(normalize)}"
                head = DenseProjectionHead(input_dim=16, hidden_dim=32, output_dim=24, head_type=head_type,
                                           normalize=normalize, pool_name=pool)
                sd = {k: (torch.randn(v.shape, generator=gen) * 0.3).float() for k, v in head.state_dict().items()}
                head.load_state_dict(sd, strict=True)
                head = head.double()
                out[f"{tag}_names"] = np.array(sorted(sd))
                coef = torch.randn(2, 24, 7, 9, generator=gen).float()
                xi = x.clone().requires_grad_(True)
                y = head(xi)
                assert tuple(y.shape) == (2, 24, 7, 9)
                (y * coef.double()).sum().backward()
                out[f"{tag}_coef"] = f32(coef)
                out[f"{tag}_y"], out[f"{tag}_dx"] = f32(y), f32(xi.grad)
                for k, v in sd.items():
                    out[f"{tag}_w_{k}"] = f32(v)
                for k, p in head.named_parameters():
                    out[f"{tag}_g_{k}"] = f32(p.grad)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {OUT.stat().st_size} bytes, {len(out)} arrays")
    del scratch


if __name__ == "__main__":
    main()
