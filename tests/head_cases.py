"""The cases tests/test_gpu_head_dispatch.py is parametrised with, and what tests/test_head_plan_coverage.py requires
of them.  A plain module (no GPU, no library call at import): the GPU tests and the CPU guard read the launch plan of a
case through the same host-side queries, cyhip.ops.head_plan / cluster_head_plan.

A head case is (shape (N, H, W), C, K, dtype name, bias, parts).  `parts` names what the GPU test runs:
  "all"  forward; backward with (dx, dw), dx only, dw only; the accumulating form        (small cases)
  "fwd"  forward, and on its logits softmax-KL / softmax-MSE forward and backward        (second trips, VALU forward)
  "dx"   the data gradient alone;  "dw"  the parameter gradients alone;  "mc"  forward and backward  (second trips)
Cases whose parts are not "all" go round a grid-stride loop a second time and carry sentinel pixels."""
from collections import namedtuple

HeadCase = namedtuple("HeadCase", "shape C K dtype bias parts")
ClusterCase = namedtuple("ClusterCase", "M C S k dtype T")

DTYPES = ("f32", "bf16", "f16")
SMALL = (2, 17, 9)    # 306 pixels: two blocks of every launch, the last one short
RAGGED = (3, 7, 13)   # 273 pixels: nine 32-pixel tiles, the last one of 17

# VALU kernels, K <= 16: head_fwd_kernel<T,16>, head_bwd_dx_kernel, head_bwd_dw_kernel<T,4>
VALU_NARROW = [(8, 1), (8, 4), (16, 4), (24, 3), (40, 5), (64, 8), (128, 12), (256, 16), (32, 16)]
# VALU kernels, K > 16: head_fwd_kernel<T,128>, head_bwd_dw_kernel<T,16>; (96, 100), (128, 20) and (128, 100) take
# head_bwd_dx_wide_kernel, the others the 8-channel one
VALU_WIDE = [(16, 20), (16, 18), (16, 128), (96, 100), (128, 20), (128, 100), (40, 17), (8, 33)]
# matrix cores: C in {32, 64}, K > 16; (32, 108) | (32, 109) is where eight waves' tiles stop fitting the LDS
MATRIX_CORE = [(32, 17), (32, 20), (32, 108), (32, 109), (32, 128), (64, 17), (64, 100), (64, 128)]

# second trips: the smallest pixel counts (within 5 %) that send some thread or wave round its loop again
FWD2 = (2, 512, 513)   # 525 312 > 2048 blocks x 256 pixels (forward, loss backward; C/8 = 2: 8-channel dx)
DW2 = (1, 250, 526)    # 131 500 > 512 blocks x 256 pixels: 257 pixels per block, the last block has 173
MC8 = (1, 263, 250)    # 65 750 > 256 blocks x 8 waves x 32 pixels (and 512 blocks x 4 waves x 32 of the backward)
MC4 = (1, 181, 182)    # 32 942 > 256 blocks x 4 waves x 32 pixels

HEAD_CASES = (
    [HeadCase(SMALL, C, K, dt, True, "all") for C, K in VALU_NARROW for dt in DTYPES]
    + [HeadCase((1, 20, 10), 16, 4, "bf16", True, "all"),     # 200 pixels: one block, fewer pixels than threads
       HeadCase(SMALL, 32, 5, "f32", False, "all")]            # no bias
    + [HeadCase(SMALL, C, K, dt, True, "all") for C, K in VALU_WIDE for dt in DTYPES]
    + [HeadCase(RAGGED, C, K, dt, True, "all") for C, K in MATRIX_CORE for dt in DTYPES]
    + [HeadCase(FWD2, 8, 4, "f32", True, "fwd"),               # 16-byte logits rows in the losses
       HeadCase(FWD2, 8, 5, "f16", True, "fwd"),               # scalar logits rows
       HeadCase(FWD2, 16, 4, "bf16", True, "dx"),              # head_bwd_dx_kernel past 4096 blocks
       HeadCase(FWD2, 128, 20, "bf16", True, "dx"),            # head_bwd_dx_wide_kernel past 8192 blocks
       HeadCase(DW2, 8, 4, "f16", True, "dw"),                 # head_bwd_dw_kernel<T,4>
       HeadCase(DW2, 8, 20, "f32", True, "dw"),                # head_bwd_dw_kernel<T,16>, vector and scalar groups
       HeadCase(MC8, 32, 20, "bf16", True, "mc"),              # eight waves; the backward's second trip too
       HeadCase(MC4, 32, 109, "f32", True, "mc")])             # four waves

CLUSTER_CASES = [
    ClusterCase(65750, 32, 5, 20, "bf16", 0.7),   # eight waves, k % 4 == 0, second trip forward and backward
    ClusterCase(32942, 32, 5, 22, "f32", 0.7),    # four waves (K = 110), k % 4 != 0, second trip forward
    ClusterCase(31, 32, 5, 20, "f16", 0.7),       # less than one tile
    ClusterCase(33, 64, 5, 22, "f32", 1.0),       # one tile and one pixel
]

DICE_CASES = [(2, 128, 129, 4), (2, 128, 129, 5)]  # (N, H, W, K): HW = 16 512 > 64 blocks x 256 pixels per sample


def case_id(c):
    if isinstance(c, HeadCase):
        n, h, w = c.shape
        return f"C{c.C}-K{c.K}-{c.dtype}-{n}x{h}x{w}-{c.parts}" + ("" if c.bias else "-nobias")
    return f"M{c.M}-C{c.C}-S{c.S}-k{c.k}-{c.dtype}"


def npix(c):
    n, h, w = c.shape
    return n * h * w


def plan(c, need_dx=True, need_dw=True):
    from cyhip import ops
    return ops.head_plan(npix(c), c.C, c.K, need_dx, need_dw)
