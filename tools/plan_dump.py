"""Dump every host-side launch-plan query of the 3x3 conv and its weight gradient over a fixed descriptor grid.

    python tools/plan_dump.py [--lib PATH] [--print] [--reduced]      # the CY_* switches of the environment
    python tools/plan_dump.py [--lib PATH] --all-settings             # one child process per switch setting
    python tools/plan_dump.py [--lib PATH] [--print] --families       # the eleven other families' plan queries

Prints the number of records and their SHA-256 (--print: the records themselves, one line each).  The planner is a pure
host function and needs no GPU, so two builds of the library are compared by diffing the output of this tool: identical
hashes under every setting mean identical kernels, tiles, split-K factors, partial counts and workspaces for every
descriptor of the grid.  Run it before and after a change of a planner rule to see exactly which layers it moves.
"""
import argparse
import ctypes as C
import hashlib
import itertools
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "contrast-you_amd"))
from cyhip._lib import ConvDesc, ConvPlan, WgradPlan, WgradReduceEntry  # noqa: E402  (struct mirrors only)

DTYPES = (0, 1, 2)  # CY_F32, CY_BF16, CY_F16
SIZES = ((7, 7), (14, 14), (16, 16), (24, 24), (28, 28), (30, 16), (32, 32), (28, 56), (40, 40), (56, 56), (64, 64),
         (112, 112), (128, 128), (224, 224), (256, 256))
BATCHES = (1, 2, 3, 8, 16, 32, 48, 512)
BATCHES_REDUCED = (1, 3, 16, 32, 512)
CHANNELS = (8, 16, 32, 64, 128, 256, 512, 1024)
# every switch setting a planner refactor has to reproduce (each one changes some plan of the grid)
SETTINGS = ("", "CY_FLOW=0", "CY_STREAM=0", "CY_STREAM=2", "CY_CONV_PLANE=0", "CY_FLOW_CFG=1", "CY_FLOW_CFG=2",
            "CY_FLOW_CFG=3", "CY_FLOW_CFG=4", "CY_DGRAD_BN_ALL=1", "CY_WGRAD_SPEC=0", "CY_WGRAD_DMA=0", "CY_WGRAD_BLK=0",
            "CY_FIRST_WGRAD_MFMA=0")


def load(path):
    lib = C.CDLL(str(path))
    pd = C.POINTER(ConvDesc)
    for name, res, args in (("cy_conv3x3_plan", C.c_int, [pd, C.POINTER(ConvPlan)]),
                            ("cy_conv3x3_num_partials", C.c_int, [pd]),
                            ("cy_conv3x3_fwd_ws_bytes", C.c_size_t, [pd]),
                            ("cy_conv3x3_stat_workgroups", C.c_int, [pd]),
                            ("cy_conv3x3_dgrad_bn_ok", C.c_int, [pd]),
                            ("cy_conv3x3_dgrad_dz_ok", C.c_int, [pd, C.c_int, C.c_int]),
                            ("cy_conv3x3_wgrad_plan", C.c_int, [pd, C.c_int, C.POINTER(WgradPlan)]),
                            ("cy_conv3x3_first_wgrad_reduce_entry", C.c_int, [C.c_int] * 6 + [C.POINTER(WgradReduceEntry)])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def descriptors(reduced=False):
    """the grid as ConvDesc field tuples (invalid combinations included: their error codes are part of the dump)"""
    lds = (1,) if reduced else (1, 2)
    for dt, (H, W), N, C1, Cout in itertools.product(DTYPES, SIZES, BATCHES_REDUCED if reduced else BATCHES, CHANNELS,
                                                     CHANNELS):
        for C2, mode, pro, split, ld in itertools.product((0, C1), (0, 1, 2), (0, 1, 2), (0, Cout // 2), lds):
            yield (N, H, W, C1, C2, Cout, mode, pro, dt, dt, ld * C1, ld * C2, ld * Cout, split,
                   ld * (Cout - split) if split else 0)


def conv_record(lib, d, plan, wplan):
    """all queries of one descriptor as a flat tuple of ints (plan fields are zeroed before every call)"""
    C.memset(C.byref(plan), 0, C.sizeof(plan))
    rec = [lib.cy_conv3x3_plan(d, plan)]
    rec += [plan.kernel, plan.th, plan.tw, plan.bn, plan.ksplit, plan.one_per_cu, plan.partials, plan.workgroups]
    rec += [lib.cy_conv3x3_num_partials(d), lib.cy_conv3x3_fwd_ws_bytes(d), lib.cy_conv3x3_stat_workgroups(d),
            lib.cy_conv3x3_dgrad_bn_ok(d), lib.cy_conv3x3_dgrad_dz_ok(d, 0, d.Cout),
            lib.cy_conv3x3_dgrad_dz_ok(d, d.split_c, d.Cout - d.split_c)]
    for n_b in (0, d.N) if d.N <= 32 else (0,):
        C.memset(C.byref(wplan), 0, C.sizeof(wplan))
        rec.append(lib.cy_conv3x3_wgrad_plan(d, n_b, wplan))
        rec += [wplan.twelve, wplan.wco, wplan.wci, wplan.wk, wplan.th, wplan.tw, wplan.splits, wplan.workgroups,
                wplan.dma, wplan.blk_order]
    return rec


def records(lib, reduced=False):
    d, plan, wplan, entry = ConvDesc(), ConvPlan(), WgradPlan(), WgradReduceEntry()
    names = [n for n, _ in ConvDesc._fields_]
    for fields in descriptors(reduced):
        for n, v in zip(names, fields):
            setattr(d, n, v)
        yield list(fields) + conv_record(lib, d, plan, wplan)
    for dt, (H, W), N, Cout in itertools.product((1, 2), SIZES, BATCHES_REDUCED if reduced else BATCHES, (32, 64)):
        C.memset(C.byref(entry), 0, C.sizeof(entry))
        rc = lib.cy_conv3x3_first_wgrad_reduce_entry(N, 1, H, W, Cout, dt, entry)
        yield [N, 1, H, W, Cout, dt, rc, entry.kind, entry.S, entry.SG, entry.Cout, entry.Cin, entry.co_pad, entry.ci_pad,
               entry.blocks]


def dump(lib_path, show, reduced):
    lib, h, n = load(lib_path), hashlib.sha256(), 0
    for rec in records(lib, reduced):
        line = " ".join(map(str, rec)) + "\n"
        h.update(line.encode())
        n += 1
        if show:
            sys.stdout.write(line)
    return n, h.hexdigest()


# ---- --families: the eleven plan queries of the loss, projector, optimiser and loader kernels, through cyhip.ops only
# (the ops.*_plan interface does not change when the C side of a query does, so one file dumps two builds)
KS = (1, 2, 3, 4, 8, 16, 17, 20, 64, 65)  # both sides of every K threshold: compiled K, the 16 / 17 split, the 64 cap
ALIGNS = (1, 2, 4, 8, 16)
COUNTS = (0, 1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1000, 4096, 4097, 65536, 65537, 262144, 262145, 2097152, 2097153,
          10 ** 7)  # 0 and 1, and each grid cap (blocks x items per block) with the size one past it


def family_calls():
    """(family, ops function name, positional arguments) over the fixed grid, refused arguments included"""
    import torch
    dts = (torch.float32, torch.bfloat16, torch.float16)
    P = itertools.product
    for Cc, hid, dt, slope in P((0, 8, 12, 16, 32, 64, 128, 256, 512, 1024), (0, 1, 64, 128, 256, 512), dts,
                                (0.01, 1.0, 1.5)):
        yield "dense_proj", "dense_proj_plan", (Cc, hid, dt, slope)
    for N, (H, W), k, pad, patch, kern in P((1, 3), ((24, 20), (64, 64), (33, 70), (256, 192)), KS, (0, 1, 3, 7),
                                            (1, 2, 16, 64), (None, "per_displacement", "staged")):
        yield "joint_patch", "joint_patch_plan", (N, H, W, k, pad, patch, kern)
    for M, Cc, hid, out, dt in P((0, 1, 31, 32, 33, 64, 65, 16384, 16385, 65536, 65537, 10 ** 6), (0, 1, 32, 33, 256, 257),
                                 (0, 16, 256, 257), (0, 1, 4, 256, 257), dts):
        yield "pixel_mlp", "pixel_mlp_plan", (M, Cc, hid, out, dt)
    for form, R, K, align in P(("rows", "pair", "logits"), COUNTS, KS, ALIGNS):
        yield "imsat", "imsat_plan", (form, R, K, align)
    for form, N, per, K, align in P(("images", "mixkl", "mixmse"), (0, 1, 2, 1024, 1025, 3000),
                                    (0, 1, 10, 143, 4096, 1 << 20), KS, ALIGNS):
        yield "mix", "mix_plan", (form, N, per, K, align)
    for npix, K, Cc, align in P(COUNTS, KS, (0, 1, 4, 5), ALIGNS):
        yield "prior", "prior_plan", ("dae", K, Cc, npix, align)
    for K, Cc in P(KS, (0, 1, 16, 63, 64, 65, 256, 257, 512)):
        yield "prior", "prior_plan", ("ortho", K, Cc, 0, 16)
    for form, n, K, align in P(("adam", "axpy", "ema_multi", "gathermse"), COUNTS, (0,) + KS, ALIGNS):
        yield "teacher", "teacher_plan", (form, n, K, align)
    for form, n, align in P(("sgd", "adamw"), COUNTS, ALIGNS):
        yield "optim", "optim_plan", (form, n, align)
    for fam, npix, K, align in P(("entropy", "selfmse", "uamt", "mixmse"), COUNTS, KS, ALIGNS):
        yield "wide_reg", "wide_reg_plan", (fam, npix, K, align)
    for N, (H, W), ns, sigma, comp, it in P((0, 1, 3, 65535, 65536), ((8, 8), (32, 32), (64, 48), (224, 224), (1024, 1024),
                                                                      (1025, 8)),
                                            (0, 1, 16, 40, 100, 101, 400), (-1.0, 0.0, 1.0, 5.0, 16.0, 17.0),
                                            (0.0, 0.1, 2.0), (-1, 0, 10)):
        yield "slic", "slic_plan", (N, H, W, ns, sigma, comp, it)
    for views, oh, ow in P((0, 1, 2, 4096, 4097), (0, 1, 8, 224, 512, 513), (0, 1, 8, 224, 512, 513)):
        yield "augment", "augment_plan", (views, oh, ow)


def dump_families(lib_path, show):
    """per family: the record count and the SHA-256 of `arguments, then the refusal or key=value in the dict's order`"""
    from cyhip import _lib
    _lib.LIB_PATH = Path(lib_path)
    from cyhip import ops
    out = {}
    for family, fn, args in family_calls():
        try:
            answer = " ".join(f"{k}={v}" for k, v in getattr(ops, fn)(*args).items())
        except _lib.HipKernelError as e:
            answer = "refused " + str(e).split("failed: ")[1]
        line = f"{family} {' '.join(str(a).replace('torch.', '') for a in args)} : {answer}\n"
        n, h = out.setdefault(family, [0, hashlib.sha256()])
        out[family][0] = n + 1
        h.update(line.encode())
        if show:
            sys.stdout.write(line)
    return {family: (n, h.hexdigest()) for family, (n, h) in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--families", action="store_true",
                    help="the eleven ops.*_plan queries beside the conv planner's, count and hash per family")
    ap.add_argument("--lib", default=str(ROOT / "contrast-you_amd" / "lib" / "libcontrastyou_hip.so"))
    ap.add_argument("--print", action="store_true", dest="show", help="print every record instead of count and hash only")
    ap.add_argument("--reduced", action="store_true", help="unit leading dimensions and five batch sizes only")
    ap.add_argument("--all-settings", action="store_true", help="one run per switch setting of SETTINGS, count and hash each")
    ap.add_argument("--jobs", type=int, default=min(len(SETTINGS), os.cpu_count() or 1))
    a = ap.parse_args()
    if a.families:
        total = hashlib.sha256()
        for family, (n, digest) in dump_families(a.lib, a.show).items():
            total.update(digest.encode())
            if not a.show:
                print(f"{family:12s} {n} {digest}")
        if not a.show:
            print(f"{'(all)':12s} {total.hexdigest()}")
        return
    if not a.all_settings:
        n, digest = dump(a.lib, a.show, a.reduced)
        if not a.show:
            print(n, digest)
        return

    def one(setting):  # (the library reads its switches once per process: a child per setting)
        env = {k: v for k, v in os.environ.items() if not k.startswith("CY_")}
        env.update(dict(kv.split("=") for kv in setting.split()))
        cmd = [sys.executable, __file__, "--lib", a.lib] + (["--reduced"] if a.reduced else [])
        return subprocess.run(cmd, env=env, check=True, capture_output=True, text=True).stdout.strip()

    with ThreadPoolExecutor(max_workers=a.jobs) as ex:
        for setting, out in zip(SETTINGS, ex.map(one, SETTINGS)):
            print(f"{setting or '(default)':24s} {out}")


if __name__ == "__main__":
    main()
