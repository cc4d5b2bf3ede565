#!/usr/bin/env python3
"""Generate tests/golden/dmt.npz: the REFERENCE's differentiable-mean-teacher hooks (semi_seg/hooks/dmt.py) driven for
three consecutive steps on the CPU, in f32 and in f64; its `mt_update` alone with the student's gradient; and
torch.optim.Adam's own float64 results for the Adam kernel's cases.  Also tests/golden/dmt_signatures.txt: the parameter
names of `DifferentiableMeanTeacherTrainerHook.__init__`.

    python tests/golden/gen_goldens_dmt.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers and names.
The cases, the stand-in model, the gather warp and the step driver: tests/dmt_cases.py.

`MTEpocherHook` and `DifferentiableMeanTeacherEpocherHook1/2/4` run as they are, through the trainer hook that builds
them, for every method and both meta criteria.  Four things of the environment are set, none of the hooks' arithmetic:
  * `simplex` of semi_seg/hooks/mt.py answers True.  The hooks wrap their criteria in L2LossChecker, which asserts that
    both inputs are distributions; the warped teacher probabilities are the all-zero vector wherever the zero-padded map
    reaches outside the image, so the assertion fails as soon as one pixel does (it is an `assert`: `python -O` drops it).
  * Optimizer.zero_grad() keeps zeroed gradients (set_to_none=False), the default of the torch the reference was written
    for; method 1 copies into `teacher_p.grad.data`, which needs them.
  * The construction-time random image takes the model's dtype (the reference draws f32, which an f64 model refuses)
    and a generator of its own.
  * The reference's EMAUpdater uses `add_(Number, Tensor)`, deprecated and still accepted; its warning is silenced.
Recorded after every step: the returned loss, the meter values, every teacher parameter and floating-point buffer (one
vector in state-dict order) and the batch counters, from the f64 run; and the f32 run's distance from it (the yardstick).
"""
import functools
import sys
import types
import warnings
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import gen_goldens as gg  # noqa: E402
import gen_goldens_cc  # noqa: E402,F401  (the import stubs the hook modules need)
from gen_goldens_imsat import arg_names  # noqa: E402
import dmt_cases as dc  # noqa: E402

OUT = Path(__file__).resolve().parent / "dmt.npz"
NAMES = Path(__file__).resolve().parent / "dmt_signatures.txt"


def main():
    scratch = gg.setup_reference()
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {})
    sys.modules["torch.utils.tensorboard"] = tb
    warnings.filterwarnings("ignore", message=".*overload of add_ is deprecated.*")
    from semi_seg.hooks import dmt as ref_dmt
    from semi_seg.hooks import mt as ref_mt

    ref_mt.simplex = lambda *a, **k: True
    zero_grad = torch.optim.Optimizer.zero_grad
    torch.optim.Adam.zero_grad = lambda self, set_to_none=False: zero_grad(self, set_to_none=False)

    def init_grad(teacher_model, teacher_optimizer):
        p = next(teacher_model.parameters())
        g = torch.Generator().manual_seed(dc.HOOK["seed"])
        image = torch.randn(1, 1, 224, 224, generator=g, dtype=torch.float64).to(p.dtype)
        teacher_model(image).mean().backward()
        teacher_optimizer.zero_grad()

    ref_dmt.DifferentiableMeanTeacherTrainerHook._initialize_teacher_gradient = staticmethod(init_grad)

    NAMES.write_text("DifferentiableMeanTeacherTrainerHook: " + " ".join(arg_names(
        scratch / "ref" / "semi_seg/hooks/dmt.py", "DifferentiableMeanTeacherTrainerHook", "__init__")) + "\n")

    out, table = {}, []
    h = dc.HOOK
    # ---- the four hooks, three steps each
    for method in dc.METHODS:
        for crit in dc.CRITERIA:
            tag = f"{method}_{crit}"
            runs = {}
            for dt in (torch.float32, torch.float64):
                student = dc.new_student(dt, "cpu")
                hook = ref_dmt.DifferentiableMeanTeacherTrainerHook(
                    name=f"dmt_{tag}_{dt}", model=student, weight=h["weight"], alpha=h["alpha"],
                    weight_decay=h["weight_decay"], meta_weight=h["meta_weight"], meta_criterion=crit,
                    method_name=method)
                init = {k: v.detach().clone() for k, v in hook.teacher_model.state_dict().items()}
                runs[dt] = (init, dc.drive(hook, student, dt, "cpu"))
            (_, r32), (init64, r64) = runs[torch.float32], runs[torch.float64]
            for k, v in init64.items():
                out[f"{tag}_init_{k}"] = v.numpy()
            meters = sorted(r64[0][1])
            out[f"{tag}_loss"] = np.array([s[0] for s in r64])
            for m in meters:
                out[f"{tag}_meter_{m}"] = np.array([s[1][m] for s in r64])
            out[f"{tag}_state"] = np.stack([s[2].numpy() for s in r64])
            out[f"{tag}_counters"] = np.array([s[3] for s in r64], dtype=np.int64)
            assert [s[3] for s in r32] == [s[3] for s in r64]
            e = [max(dc.rel_scalar(a[0], b[0]) for a, b in zip(r32, r64)),
                 max(dc.rel_scalar(a[1][m], b[1][m]) for a, b in zip(r32, r64) for m in meters),
                 max(dc.rel_max(a[2], b[2]) for a, b in zip(r32, r64))]
            out[f"{tag}_e_ref"] = np.array(e)
            table.append((tag, e))

    # ---- mt_update alone, with the student's gradient
    res = {}
    li, lt, ui, m = dc.hook_data(0)
    for dt in (torch.float32, torch.float64):
        student = dc.new_student(dt, "cpu")
        hook = ref_dmt.DifferentiableMeanTeacherTrainerHook(
            name=f"dmt_update_{dt}", model=student, weight=1.0, meta_criterion="ce", method_name="mt")()
        z = student(dc.warp_by_map(ui.to(dt), m)).detach().requires_grad_(True)
        loss = hook.mt_update(teacher_model=hook.teacher_model, criterion=hook._criterion, unlabeled_tf_logits=z,
                              unlabeled_image=ui.to(dt), affine_transformer=lambda x: dc.warp_by_map(x, m))
        loss.backward()
        res[dt] = (loss.detach(), z.grad)
    (v32, g32), (v64, g64) = res[torch.float32], res[torch.float64]
    out["update_loss"], out["update_grad"] = np.float64(v64), g64.numpy()
    e = [dc.rel_scalar(v32, v64), *dc.rel_grad(g32, g64)]
    out["update_e_ref"] = np.array(e)
    table.append(("mt_update", e))

    # ---- torch.optim.Adam in float64 on the kernel's 257-element cases
    for step, wd, case, zero in dc.adam_cases():
        if case != dc.FlatCase(257, False):
            continue
        p, g, mm, v = dc.adam_inputs(step, case.n, zero)
        got = dc.adam_torch(p, g, mm, v, step, float(np.float32(wd)), torch.float64)
        for name, t in zip(("p", "m", "v"), got):
            out[f"adam_s{step}_wd{wd:g}_z{int(zero)}_{name}"] = t.numpy()

    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {OUT.stat().st_size} bytes; {NAMES}: {NAMES.read_text()}")
    print("reference f32 vs f64:  run | loss | meters | teacher state (max-norm)      [mt_update: loss | grad2 | gradmax]")
    for name, e in table:
        print(f"  {name:16s} | {e[0]:.2e} | {e[1]:.2e} | {e[2]:.2e}")
    del scratch


if __name__ == "__main__":
    main()
