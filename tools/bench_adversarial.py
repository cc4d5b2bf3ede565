#!/usr/bin/env python3
"""ms / step of the adversarial baseline at the C2 shape (16 labeled + 16 unlabeled slices of 224 x 224, 4 classes,
`Discriminator(5, hidden_dim=64)`, `dis_consider_image=True`, f32 like the reference's epocher), and the kernels of
csrc/cy_disc.hip one by one at the shapes of that step.

Four steps are timed in the same process, alternating, each with its own U-Net, discriminator and optimizers:
    hip      `AdversarialEpocher._adversarial_step` as built: fused softmax + concat, the implicit-GEMM `Conv4x4Fn`,
             BatchNorm + LeakyReLU and sigmoid + BCE kernels;
    im2col   the same step with `Discriminator.conv` set to the `Conv2dFn` form (im2col + GEMM + col2im) around it;
    torch-D  the same step with the discriminator section replaced by torch-ROCm's own layers (`nn.Sequential` of
             Conv2d / BatchNorm2d / LeakyReLU / Sigmoid, `nn.BCELoss`, `torch.cat` + `softmax`): the yardstick;
    sup      the plain supervised step (reg_weight = 0): what the regulariser costs on top.
All four update the same meters (sup_loss, sup_dice, gen_loss, dis_loss).  A step is timed as host wall time over
`--steps` steps that end in a device synchronise (30 steps: a window of 0.2-0.8 s), after `--warmup` steps; `--rounds`
rounds, the median and the spread are printed.  Kernel lines: tools/bench_cc.py's harness with 200 repetitions per
window (`gpu` = device time of back-to-back executions, with the algorithmic bytes over it and that rate's share of the
8.0 TB/s HBM peak).  Convolution lines: `Conv4x4Fn` and `Conv2dFn` side by side at the five layer shapes of the step
-- forward, forward + data gradient (the G step's pass) and forward + both gradients (a D-step pass; weight packing,
autograd and the output allocations included) -- with the new kernels' FLOP rate against the 157.3 TFLOP/s f32 matrix
peak, and their sums over one step.  Two gate lines close the output: the new step against the im2col step of the same
run (faster by more than the min-max spread of the rounds), and no stride-2 layer slower than `Conv2dFn` in any column.

    python tools/bench_adversarial.py [--n 16] [--hw 224] [--steps 30] [--warmup 3] [--rounds 5] [--json out.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
from bench_cc import DEV, gpu_us, issue_us  # noqa: E402  (puts contrast-you_amd on sys.path)
from contrastyou.arch import UNet  # noqa: E402
from contrastyou.arch.discriminator import Discriminator, conv_im2col, conv_implicit  # noqa: E402
from contrastyou.losses.kl import KL_div  # noqa: E402
from contrastyou.optim import RAdam  # noqa: E402
from cyhip import ops  # noqa: E402
from cyhip.glue import Conv2dFn, Conv4x4Fn  # noqa: E402
from semi_seg.epochers.comparable import AdversarialEpocher  # noqa: E402
from semi_seg.epochers.epocher import _sup_loss  # noqa: E402

K, HIDDEN, HBM_PEAK, F32_MATRIX_PEAK = 4, 64, 8.0e12, 157.3e12


class _Loader(list):
    dataset = type("_DS", (), {"transforms": type("_T", (), {"_total_freedom": False})})()


def make_step(kind, data, reg_weight=0.1):
    """-> a callable that runs one step of `kind` in ("hip", "im2col", "torch", "sup")"""
    torch.manual_seed(0)
    model = UNet(input_dim=1, num_classes=K).to(DEV)
    dis = Discriminator(1 + K, HIDDEN).to(DEV)
    opt = RAdam([{"params": list(model.parameters())}], lr=1e-6)
    dopt = RAdam([{"params": list(dis.parameters())}], lr=1e-6)
    ep = AdversarialEpocher(model=model, optimizer=opt, labeled_loader=_Loader(), unlabeled_loader=_Loader(),
                            sup_criterion=KL_div(), num_batches=1, device=DEV, discriminator=dis, disc_optimizer=dopt,
                            reg_weight=reg_weight if kind != "sup" else 0.0, dis_consider_image=True,
                            scaler=torch.amp.GradScaler("cuda", enabled=False))
    ep.init()
    ep.meters.reset()
    model.train()
    lab_img, lab_tgt, unl_img = data
    if kind in ("hip", "sup"):
        return lambda: ep._adversarial_step(lab_img, lab_tgt, None, unl_img if kind == "hip" else None)
    if kind == "im2col":
        def im2col_step():
            Discriminator.conv = staticmethod(conv_im2col)  # the class attribute is the only selector there is
            try:
                ep._adversarial_step(lab_img, lab_tgt, None, unl_img)
            finally:
                Discriminator.conv = staticmethod(conv_implicit)
        return im2col_step

    main, bce, crit = dis._main, nn.BCELoss(), KL_div()  # torch's own layers over the same parameters

    def feed(image, logits):
        return torch.cat([image, logits.softmax(1)], dim=1)

    def step():
        opt.zero_grad()
        lab = model(lab_img)
        sup = _sup_loss(crit, lab, lab_tgt, K)
        unl = model(unl_img)
        out = main(feed(unl_img, unl))
        gen = bce(out, torch.ones_like(out))
        (sup + reg_weight * gen).backward()
        opt.step()
        with torch.no_grad():  # the meters of `_adversarial_step`
            ep.meters["sup_loss"].add(sup.detach())
            ep.meters["sup_dice"].add_logits(lab, lab_tgt, group_name=None)
            with ep.meters.focus_on("adv_reg"):
                ep.meters["gen_loss"].add(gen.detach())
        dopt.zero_grad()
        out_l, out_u = main(feed(lab_img, lab.detach())), main(feed(unl_img, unl.detach()))
        disc = bce(out_l, torch.ones_like(out_l)) + bce(out_u, torch.zeros_like(out_u))
        (disc * reg_weight).backward()
        dopt.step()
        with ep.meters.focus_on("adv_reg"):
            ep.meters["dis_loss"].add(disc.detach())

    return step


def time_steps(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


REPS = 200  # repetitions per timed window of a kernel line


def kernel_line(name, fn, nbytes):
    g, i = min(gpu_us(fn, REPS), gpu_us(fn, REPS)), min(issue_us(fn, REPS), issue_us(fn, REPS))
    rate = nbytes / (g * 1e-6)
    print(f"{name:44s} gpu {g:8.1f} us  issue {i:8.1f} us  {nbytes / 1e6:8.2f} MB  {rate / 1e9:7.1f} GB/s  "
          f"{100 * rate / HBM_PEAK:5.1f} % of HBM peak", flush=True)
    return {"name": name, "gpu_us": g, "issue_us": i, "bytes": nbytes, "share_of_hbm_peak": rate / HBM_PEAK}


def kernels(n, hw):
    gen = torch.Generator().manual_seed(1)
    rows = []
    z = ops.to_nhwc((torch.randn(n, K, hw, hw, generator=gen) * 2).to(DEV))
    img = torch.rand(n, 1, hw, hw, generator=gen).to(DEV)
    npix = n * hw * hw
    cat = ops.softmax_cat_fwd(img, z)
    rows.append(kernel_line(f"softmax_cat_fwd {npix} x (1 + {K})", lambda: ops.softmax_cat_fwd(img, z),
                            4 * npix * (K + 1 + 1 + K)))
    rows.append(kernel_line(f"softmax_cat_bwd {npix} x (1 + {K})", lambda: ops.softmax_cat_bwd(z, cat, 1),
                            4 * npix * (K + (1 + K) + K)))
    a = torch.randn(n, hw // 2, hw // 2, HIDDEN, generator=gen).to(DEV)
    rows.append(kernel_line(f"leaky_relu_fwd {a.numel()}", lambda: ops.leaky_relu_fwd(a, 0.2), 8 * a.numel()))
    rows.append(kernel_line(f"leaky_relu_bwd {a.numel()}", lambda: ops.leaky_relu_bwd(a, a, 0.2), 12 * a.numel()))
    for div, Cc in ((4, 2 * HIDDEN), (8, 4 * HIDDEN), (16, 8 * HIDDEN)):
        M = n * (hw // div) ** 2
        x, dy = torch.randn(M, Cc, generator=gen).to(DEV), torch.randn(M, Cc, generator=gen).to(DEV)
        g, b = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
        mean, var = ops.bn_rows_stats(x)
        nb, tag = 4 * M * Cc, f"{M} x {Cc}"
        rows.append(kernel_line(f"bn_rows_stats {tag} (2 launches)", lambda: ops.bn_rows_stats(x), nb))
        rows.append(kernel_line(f"bn_lrelu_fwd {tag}", lambda: ops.bn_lrelu_fwd(x, mean, var, g, b, 1e-5, 0.2), 2 * nb))
        rows.append(kernel_line(f"bn_lrelu_bwd reduce + apply {tag} (3)",
                                lambda: ops.bn_lrelu_bwd(x, dy, mean, var, g, b, 1e-5, 0.2, True), 5 * nb))
    m = hw // 16 - 3
    s = torch.randn(n, 1, m, m, generator=gen).to(DEV)
    gs = torch.ones(1, device=DEV)
    rows.append(kernel_line(f"sigmoid_bce_fwd {s.numel()} (2 launches)", lambda: ops.sigmoid_bce_fwd(s, 1.0),
                            4 * s.numel()))
    rows.append(kernel_line(f"sigmoid_bce_bwd {s.numel()}", lambda: ops.sigmoid_bce_bwd(s, 1.0, gs), 8 * s.numel()))
    return rows


def convolutions(n, hw):
    """`Conv4x4Fn` and `Conv2dFn` at the five layer shapes: device time of the forward, of forward + data gradient and
    of forward + both gradients; -> rows and, per function, the device time of all convolution work of one step (3
    forwards, of which one is followed by a data-gradient backward and two by full backwards)"""
    gen = torch.Generator().manual_seed(2)
    layers = [(1 + K, HIDDEN, hw, 2, 1), (HIDDEN, 2 * HIDDEN, hw // 2, 2, 1), (2 * HIDDEN, 4 * HIDDEN, hw // 4, 2, 1),
              (4 * HIDDEN, 8 * HIDDEN, hw // 8, 2, 1), (8 * HIDDEN, 1, hw // 16, 1, 0)]
    forms = {"conv4x4": lambda x, w, s, p: Conv4x4Fn.apply(x, w, s, p),
             "conv2d": lambda x, w, s, p: Conv2dFn.apply(x, w, None, s, p)}
    rows, per_step = [], {name: 0.0 for name in forms}
    for i, (cin, cout, h, stride, pad) in enumerate(layers):
        x = ops.to_nhwc(torch.randn(n, cin, h, h, generator=gen).to(DEV))
        w = (0.02 * torch.randn(cout, cin, 4, 4, generator=gen)).to(DEV)
        row = {"layer": i, "stride": stride}
        for name, conv in forms.items():
            with torch.no_grad():
                gy = torch.ones_like(conv(x, w, stride, pad))

            def fwd():
                with torch.no_grad():
                    conv(x, w, stride, pad)

            def fwd_bwd(x_grad, w_grad):
                def run():
                    xs, ws = x.detach().requires_grad_(x_grad), w.detach().requires_grad_(w_grad)
                    conv(xs, ws, stride, pad).backward(gy)
                return run

            t_f = min(gpu_us(fwd, 50), gpu_us(fwd, 50))
            t_g = min(gpu_us(fwd_bwd(True, False), 50), gpu_us(fwd_bwd(True, False), 50))
            t_d = min(gpu_us(fwd_bwd(i > 0, True), 50), gpu_us(fwd_bwd(i > 0, True), 50))
            row[name] = {"fwd_us": t_f, "fwd_dgrad_us": t_g, "fwd_both_us": t_d}
            per_step[name] += t_g + 2 * t_d
        flop = 2.0 * n * gy.shape[2] * gy.shape[3] * cout * 16 * cin  # one GEMM of the layer
        new, old = row["conv4x4"], row["conv2d"]
        rates = [flop / (new["fwd_us"] * 1e-6), 2 * flop / (new["fwd_dgrad_us"] * 1e-6),
                 (3 if i > 0 else 2) * flop / (new["fwd_both_us"] * 1e-6)]
        row["conv4x4"]["flops"], row["gemm_flop"] = rates, flop
        row["patch_bytes"] = n * (gy.shape[2] * gy.shape[3]) * 16 * cin * 4
        print(f"conv {i}: {cin:3d} -> {cout:3d} at {h:3d}^2  fwd {new['fwd_us']:7.1f} | {old['fwd_us']:7.1f} us  "
              f"+ dgrad {new['fwd_dgrad_us']:7.1f} | {old['fwd_dgrad_us']:7.1f} us  "
              f"+ dgrad + wgrad {new['fwd_both_us']:7.1f} | {old['fwd_both_us']:7.1f} us  (Conv4x4Fn | Conv2dFn);  "
              f"Conv4x4Fn {rates[0] / 1e12:5.1f} / {rates[1] / 1e12:5.1f} / {rates[2] / 1e12:5.1f} TFLOP/s = "
              + " / ".join(f"{100 * r / F32_MATRIX_PEAK:4.1f}" for r in rates) + " % of the f32 matrix peak", flush=True)
        rows.append(row)
    for name in forms:
        print(f"convolutions of one step (G pass + two D passes), {name}: {per_step[name] / 1e3:.2f} ms device time",
              flush=True)
    return rows, {name: t / 1e3 for name, t in per_step.items()}


def gates(result):
    """the two conditions this tool is run for; -> {name: bool}, printed"""
    new, old = result["hip_ms_all"], result["im2col_ms_all"]
    spread = max(max(new) - min(new), max(old) - min(old))
    step_ok = result["im2col_ms"] - result["hip_ms"] > spread
    print(f"gate, step: Conv4x4Fn {result['hip_ms']:.2f} ms vs Conv2dFn {result['im2col_ms']:.2f} ms, min-max spread "
          f"{spread:.2f} ms: {'PASS' if step_ok else 'FAIL'}")
    slower = [(r["layer"], c) for r in result["convolutions"] if r["stride"] == 2
              for c in ("fwd_us", "fwd_dgrad_us", "fwd_both_us") if r["conv4x4"][c] > r["conv2d"][c]]
    print(f"gate, layers: stride-2 layers slower than Conv2dFn in a column: {slower or 'none'}: "
          f"{'PASS' if not slower else 'FAIL'}")
    return {"step": bool(step_ok), "layers": not slower}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adversarial.py measures on the GPU; there is no CPU fallback")
    print(f"# device {torch.cuda.get_device_name(0)}; {a.n} + {a.n} slices of {a.hw} x {a.hw}, K = {K}, "
          f"hidden_dim = {HIDDEN}, f32")
    gen = torch.Generator().manual_seed(0)
    data = (torch.rand(a.n, 1, a.hw, a.hw, generator=gen).to(DEV),
            torch.randint(0, K, (a.n, 1, a.hw, a.hw), generator=gen).to(DEV),
            torch.rand(a.n, 1, a.hw, a.hw, generator=gen).to(DEV))
    kinds = ("hip", "im2col", "torch", "sup")
    steps = {k: make_step(k, data) for k in kinds}
    for k in kinds:
        for _ in range(a.warmup):
            steps[k]()
    torch.cuda.synchronize()
    times = {k: [] for k in kinds}
    for _ in range(a.rounds):
        for k in kinds:  # alternating: every round times all four
            times[k].append(time_steps(steps[k], a.steps))
    result = {"n": a.n, "hw": a.hw, "steps": a.steps, "rounds": a.rounds}
    for k, label in zip(kinds, ("this build (Conv4x4Fn)", "this build, Discriminator.conv = Conv2dFn form",
                                "torch-ROCm discriminator + BCELoss", "supervised step alone")):
        med = statistics.median(times[k])
        print(f"step {k:6s} {med:8.2f} ms  (min {min(times[k]):.2f}, max {max(times[k]):.2f})  {label}", flush=True)
        result[f"{k}_ms"] = med
        result[f"{k}_ms_all"] = times[k]
    print(f"regulariser cost: hip {result['hip_ms'] - result['sup_ms']:.2f} ms, "
          f"im2col {result['im2col_ms'] - result['sup_ms']:.2f} ms, "
          f"torch-D {result['torch_ms'] - result['sup_ms']:.2f} ms per step")
    del steps
    torch.cuda.empty_cache()
    result["kernels"] = kernels(a.n, a.hw)
    result["convolutions"], result["convolutions_ms_per_step"] = convolutions(a.n, a.hw)
    result["gates"] = gates(result)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
