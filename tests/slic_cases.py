"""The SLIC superpixels of csrc/cy_slic.hip restated in NumPy (int64 arithmetic; scipy.ndimage for the float64 blur and
for the components), and the cases the host and GPU tests share.

The restatement is the specification of include/contrastyou_hip.h ("On-device SLIC superpixels"): after the blur every
quantity is an integer, so the device has to reproduce `cluster` and `connect` bit for bit.  The blur is held against
scipy's float64 `gaussian_filter`; `blur_q_f32` is the kernel's own arithmetic (f32, taps in order).
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np
from scipy import ndimage

MAX_SIDE, MAX_K, MAX_SIGMA = 1024, 100, 16
OK, ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = 0, -1, -2, -5


# ---- geometry -------------------------------------------------------------------------------------------------------
def radius(sigma: float) -> int:
    return int(4.0 * sigma + 0.5)


def gauss_weights(sigma: float):
    """(r, float64 weights over i = -r .. r), scipy.ndimage's _gaussian_kernel1d"""
    r = radius(sigma)
    i = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 * (i / sigma) ** 2)
    return r, w / w.sum()


def grid(H: int, W: int, n_segments: int):
    """(S, start, ys, xs): skimage.util.regular_grid for a 2-D slice"""
    s = math.sqrt(H * W / n_segments)
    S, start = round(s), int(s // 2)  # round(): half to even
    if S < 1:
        return S, start, [], []
    return S, start, list(range(start, H, S)), list(range(start, W, S))


def status(N, H, W, n_segments=40, sigma=5.0, compactness=0.1, max_iter=10) -> int:
    """the refusal of these sizes, in the order the header gives"""
    if max_iter < 0 or N < 1:
        return ERR_ARG
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE) or N > 65535:
        return ERR_SHAPE
    if not sigma >= 0:
        return ERR_ARG
    if sigma > MAX_SIGMA or radius(sigma) > min(H, W):
        return ERR_SHAPE
    if not math.isfinite(compactness) or not 1 <= round(compactness * 65535) <= 65535:
        return ERR_ARG
    if n_segments < 1:
        return ERR_ARG
    S, _, ys, xs = grid(H, W, n_segments)
    K = len(ys) * len(xs)
    if S < 1 or not 1 <= K <= MAX_K or H * W < 64 * K:
        return ERR_SHAPE
    return OK


# ---- a. blur and quantise -------------------------------------------------------------------------------------------
def quantise(v: np.ndarray) -> np.ndarray:
    """floor(clamp(v, 0, 1) * 65535 + 0.5) in float64, where it is exact for a float32 v"""
    return np.floor(np.clip(v.astype(np.float64), 0.0, 1.0) * 65535.0 + 0.5).astype(np.int64)


def blur_q_f64(images: np.ndarray, sigma: float) -> np.ndarray:
    """images [N,H,W] -> q int64: scipy's float64 Gaussian (reflect, truncate 4) along H and W of every slice"""
    x = images.astype(np.float64)
    if sigma > 0:
        x = ndimage.gaussian_filter(x, sigma=(0, sigma, sigma), mode="reflect", truncate=4.0)
    return quantise(x)


def _blur_axis_f32(x: np.ndarray, w32: np.ndarray, r: int, axis: int) -> np.ndarray:
    n = x.shape[axis]
    idx = np.arange(n)
    acc = np.zeros_like(x)
    for i in range(-r, r + 1):  # the kernel's tap order; product and sum each rounded to f32
        j = idx + i
        j = np.where(j < 0, -j - 1, np.where(j >= n, 2 * n - 1 - j, j))
        acc = acc + w32[abs(i)] * np.take(x, j, axis=axis)
    return acc


def blur_q_f32(images: np.ndarray, sigma: float) -> np.ndarray:
    """the kernel's arithmetic: weights normalised in f64 then cast, f32 accumulation along H then W, then the exact
    quantisation"""
    x = images.astype(np.float32)
    if sigma > 0:
        r, w = gauss_weights(sigma)
        w32 = w[r:].astype(np.float32)  # w[|i|]
        x = _blur_axis_f32(_blur_axis_f32(x, w32, r, 1), w32, r, 2)
    return quantise(x)


# ---- b, c. grid and the rounds --------------------------------------------------------------------------------------
def cluster(q: np.ndarray, n_segments: int, compactness: float, max_iter: int = 10):
    """q int [N,H,W] -> (labels int64 [N,H,W], centres int64 [N,K,3] = cy, cx, cq after the last update)"""
    N, H, W = q.shape
    S, _, ys, xs = grid(H, W, n_segments)
    M = round(compactness * 65535)
    K = len(ys) * len(xs)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    labels = np.zeros((N, H, W), dtype=np.int64)
    centres = np.zeros((N, K, 3), dtype=np.int64)
    far = np.iinfo(np.int64).max
    for n in range(N):
        qn = q[n].astype(np.int64)
        c = np.array([(y, x, qn[y, x]) for y in ys for x in xs], dtype=np.int64).reshape(K, 3)
        for _ in range(max_iter):
            best_key = np.full((H, W), far, dtype=np.int64)
            best = np.full((H, W), -1, dtype=np.int64)
            for k in range(K):
                dy, dx, dc = yy - c[k, 0], xx - c[k, 1], qn - c[k, 2]
                key = dc * dc * (S * S) + (dy * dy + dx * dx) * (M * M)
                take = (np.abs(dy) <= 2 * S) & (np.abs(dx) <= 2 * S) & ((best < 0) | (key < best_key))
                best_key = np.where(take, key, best_key)
                best = np.where(take, k, best)
            labels[n] = np.where(best >= 0, best, labels[n])
            flat = labels[n].ravel()
            cnt = np.bincount(flat, minlength=K)
            for j, v in enumerate((yy, xx, qn)):
                tot = np.zeros(K, dtype=np.int64)
                np.add.at(tot, flat, v.ravel())
                has = cnt > 0
                c[has, j] = (2 * tot[has] + cnt[has]) // (2 * cnt[has])
        centres[n] = c
    return labels, centres


# ---- d. connectivity ------------------------------------------------------------------------------------------------
def components(labels2d: np.ndarray):
    """(comp [H,W]: index of every pixel's 4-connected component of equal label, numbered by increasing root;
    roots, sizes per component)"""
    H, W = labels2d.shape
    comp = np.zeros((H, W), dtype=np.int64)
    n = 0
    for v in np.unique(labels2d):
        lab, m = ndimage.label(labels2d == v)  # default structure: 4-connectivity
        comp = np.where(lab > 0, lab + n, comp)
        n += m
    flat = comp.ravel() - 1
    roots = np.full(n, H * W, dtype=np.int64)
    np.minimum.at(roots, flat, np.arange(H * W, dtype=np.int64))
    order = np.argsort(roots)
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    comp = rank[flat].reshape(H, W)
    return comp, roots[order], np.bincount(comp.ravel(), minlength=n)


def connect(labels: np.ndarray, n_segments: int):
    """labels int [N,H,W] -> (ids uint8 [N,H,W], count int32 [N])"""
    N, H, W = labels.shape
    _, _, ys, xs = grid(H, W, n_segments)
    min_size = (H * W) // (2 * len(ys) * len(xs))
    ids = np.zeros((N, H, W), dtype=np.uint8)
    count = np.zeros(N, dtype=np.int32)
    for n in range(N):
        comp, roots, sizes = components(labels[n])
        flat = comp.ravel()
        final = np.arange(len(roots))
        for c in range(len(roots)):  # by increasing root: the target's own fate is known already
            r = int(roots[c])
            if r != 0 and sizes[c] < min_size:
                final[c] = final[flat[r - 1 if r % W > 0 else r - W]]
        kept = final == np.arange(len(roots))
        number = np.cumsum(kept) - 1
        count[n] = int(kept.sum())
        ids[n] = number[final[comp]].astype(np.uint8)
    return ids, count


def slic(images: np.ndarray, n_segments=40, sigma=5.0, compactness=0.1, max_iter=10, blur=blur_q_f64):
    labels, _ = cluster(blur(images, sigma), n_segments, compactness, max_iter)
    return connect(labels, n_segments)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def blobs(N: int, H: int, W: int, seed: int) -> np.ndarray:
    """f32 [N,H,W] in 0..1: a few soft discs on a ramp plus noise -- structure at the scale of the superpixels"""
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.empty((N, H, W), dtype=np.float32)
    for n in range(N):
        img = 0.2 + 0.2 * xx / W + 0.1 * yy / H
        for _ in range(6):
            cy, cx, rad, amp = g.uniform(0, H), g.uniform(0, W), g.uniform(0.08, 0.3) * min(H, W), g.uniform(-0.3, 0.5)
            img = img + amp / (1.0 + np.exp((np.hypot(yy - cy, xx - cx) - rad) / 1.5))
        out[n] = np.clip(img + g.normal(0, 0.03, (H, W)), 0, 1)
    return out


def noise(N: int, H: int, W: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).random((N, H, W), dtype=np.float32)


def constant(N: int, H: int, W: int, seed: int) -> np.ndarray:
    return np.full((N, H, W), 0.25, dtype=np.float32)  # 0.25 * 65535 + 0.5 is far from an integer


def spirals(H: int = 64, W: int = 64) -> np.ndarray:
    """int32 [1,H,W]: a one-pixel-wide spiral of 1s wound from the corner inwards with one-pixel gaps; the gaps are a
    spiral of 0s -- two interleaved components, each about H*W/2 long"""
    m = np.zeros((H, W), dtype=np.int32)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1
    turns = 0
    while turns < 2:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        free = 0 <= ny < H and 0 <= nx < W and m[ny, nx] == 0
        ahead = not (0 <= ay < H and 0 <= ax < W) or m[ay, ax] == 0
        if free and ahead:
            y, x, turns = ny, nx, 0
            m[y, x] = 1
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return m[None]


def speckle(H: int, W: int, values: int, seed: int) -> np.ndarray:
    """int32 [1,H,W]: every pixel an independent label -- hundreds of tiny components, long merge chains"""
    return np.random.default_rng(seed).integers(0, values, (1, H, W)).astype(np.int32)


# name -> N, H, W, n_segments, sigma, compactness, image maker, seed.  Between them: an odd size whose windows are
# clipped on every side, a size past one block of pixels and past one blur tile in both directions, K = 1, N = 1 and
# N = 5, sigma = 0 (the quantise-only form), the widest blur (r = 64, the largest LDS tile), all ties, and the
# reference's own parameters at its own size.
CASES = {
    "odd_37x53": dict(N=1, H=37, W=53, n_segments=20, sigma=1.0, compactness=0.1, make=blobs, seed=1),
    "tiles_70x130_n5": dict(N=5, H=70, W=130, n_segments=40, sigma=2.0, compactness=0.1, make=blobs, seed=2),
    "one_centre": dict(N=1, H=37, W=53, n_segments=1, sigma=1.0, compactness=0.1, make=blobs, seed=3),
    "noise_96x160": dict(N=1, H=96, W=160, n_segments=40, sigma=0.0, compactness=1e-3, make=noise, seed=4),
    "constant": dict(N=1, H=37, W=53, n_segments=20, sigma=1.0, compactness=0.1, make=constant, seed=0),
    "widest_blur": dict(N=1, H=70, W=130, n_segments=40, sigma=16.0, compactness=0.1, make=blobs, seed=5),
    "reference_224": dict(N=1, H=224, W=224, n_segments=40, sigma=5.0, compactness=0.1, make=blobs, seed=6),
}
# the blur alone: the sizes and sigmas of the prototype (37x53, 96x160, 224^2; sigma 1, 2, 5)
BLUR_CASES = [(37, 53, 1.0), (37, 53, 2.0), (37, 53, 5.0), (96, 160, 1.0), (96, 160, 2.0), (96, 160, 5.0),
              (224, 224, 1.0), (224, 224, 2.0), (224, 224, 5.0), (70, 130, 16.0)]


@lru_cache(maxsize=None)
def case(name: str):
    """the case's images and the restatement's result on them, computed once and shared (treat as read-only):
    images f32, q (float64 blur), labels, centres, ids, count"""
    c = CASES[name]
    images = c["make"](c["N"], c["H"], c["W"], c["seed"])
    q = blur_q_f64(images, c["sigma"])
    labels, centres = cluster(q, c["n_segments"], c["compactness"])
    ids, count = connect(labels, c["n_segments"])
    out = dict(c, images=images, q=q, labels=labels, centres=centres, ids=ids, count=count)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
