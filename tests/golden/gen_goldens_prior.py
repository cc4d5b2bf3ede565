#!/usr/bin/env python3
"""Generate tests/golden/prior.npz from the REFERENCE's two hook modules, run on the CPU in f32:
semi_seg/hooks/autoencoder.py (AuxiliaryLayer, DenoisingAutoEncoderEpocherHook) and semi_seg/hooks/orthogonal.py
(_OrthogonalEpocherHook).

    python tests/golden/gen_goldens_prior.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers.  The
cases and the layout of the file: tests/prior_cases.py.

    aux_k<K>_weight, aux_k<K>_bias      AuxiliaryLayer(in_features=K).state_dict() under torch.manual_seed(seed),
                                        (K, seed) of prior_cases.AUX_INIT
    per DAE hook case <tag> of prior_cases.HOOK_DAE (the layer is the recorded one of the case's K):
        <tag>_z_i8d8 [N,K,H,W] int8     logits on the 1/8 grid, exact in f32
        <tag>_image [N,Cimg,H,W] f32
        <tag>_value, <tag>_meter        what _call_implementation returned (weight * loss) and what its meter received
        <tag>_g_logits, <tag>_g_weight, <tag>_g_bias      the gradients of the returned value
    per orthogonality case <tag> of prior_cases.HOOK_ORTHO:
        <tag>_v [K,C,1,1] f32, <tag>_value, <tag>_meter, <tag>_g_v
"""
import sys
import types
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import gen_goldens as gg  # noqa: E402
import gen_goldens_cc  # noqa: E402,F401  (the import stubs the hook modules need)
from gen_goldens_imsat import Rec, leaf  # noqa: E402
import prior_cases as pc  # noqa: E402

OUT = Path(__file__).resolve().parent / "prior.npz"


def main():
    scratch = gg.setup_reference()
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {})
    sys.modules["torch.utils.tensorboard"] = tb
    from semi_seg.hooks import autoencoder as ref_ae
    from semi_seg.hooks import orthogonal as ref_or

    out = {}
    layers = {}
    for K, seed in pc.AUX_INIT:
        torch.manual_seed(seed)
        layers[K] = ref_ae.AuxiliaryLayer(in_features=K)
        sd = layers[K].state_dict()
        assert sorted(sd) == ["fc.bias", "fc.weight"], sorted(sd)
        out[f"aux_k{K}_weight"], out[f"aux_k{K}_bias"] = sd["fc.weight"].numpy().copy(), sd["fc.bias"].numpy().copy()

    gen = torch.Generator().manual_seed(1907)
    for h in pc.HOOK_DAE:
        tag, K = h["tag"], h["K"]
        z = (torch.randn(h["N"], K, h["H"], h["W"], generator=gen) * 12).round().clamp(-48, 48).to(torch.int8)
        img = torch.rand(h["N"], h["Cimg"], h["H"], h["W"], generator=gen)
        out[f"{tag}_z_i8d8"], out[f"{tag}_image"] = z.numpy(), img.numpy()
        layer = layers[K]
        layer.zero_grad()
        hook = ref_ae.DenoisingAutoEncoderEpocherHook(extra_layer=layer, weight=h["weight"])
        assert hook._name == "deAE"
        hook.meters = {"ls": Rec()}
        logits = leaf(z.float() / 8, torch.float32)
        value = hook._call_implementation(unlabeled_image_tf=img, unlabeled_tf_logits=logits)
        value.backward()
        out[f"{tag}_value"], out[f"{tag}_meter"] = np.float32(value.item()), np.array(hook.meters["ls"].got)
        out[f"{tag}_g_logits"] = logits.grad.numpy().copy()
        out[f"{tag}_g_weight"], out[f"{tag}_g_bias"] = layer.fc.weight.grad.numpy().copy(), layer.fc.bias.grad.numpy().copy()

    for h in pc.HOOK_ORTHO:
        tag = h["tag"]
        v = torch.randn(h["K"], h["C"], 1, 1, generator=gen) * torch.exp(torch.rand(h["K"], 1, 1, 1, generator=gen) * 4 - 2)
        out[f"{tag}_v"] = v.numpy().copy()
        p = leaf(v, torch.float32)
        hook = ref_or._OrthogonalEpocherHook(name="orth", prototypes=p, weight=h["weight"])
        hook.meters = {"loss": Rec()}
        value = hook._call_implementation()
        value.backward()
        out[f"{tag}_value"], out[f"{tag}_meter"] = np.float32(value.item()), np.array(hook.meters["loss"].got)
        out[f"{tag}_g_v"] = p.grad.numpy().copy()

    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {OUT.stat().st_size} bytes, {len(out)} arrays")
    for k in sorted(out):
        if k.endswith("_value"):
            print(f"  {k} = {float(out[k]):.8g}")
    del scratch


if __name__ == "__main__":
    main()
