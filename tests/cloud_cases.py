"""Shared by tests/test_cloud_host.py (CPU) and tests/test_gpu_cloud.py (MI355X): the definition of the packed point cloud
(include/mvsgi.h, "packed point cloud") in numpy, seeded case generators, and the shapes and keep patterns the GPU tests run.

The definition: per frame b and pixel p = i * W + j, d = fp32(bf) / inv (numpy's float32 division is the IEEE one), xyz = rays * d,
keep = lattice & mask & finite(d) & d_min <= d <= d_max & every gate inside its closed interval (& some camera valid, with
require_colour); a comparison with a NaN is false.  The kept pixels of a frame in ascending p; colour of the lowest valid camera or
no_colour; written = min(kept, capacity)."""
import numpy as np

TILE = 1024                      # pixels per tile of csrc/cloud.hip
SCAN_PASS = 256                  # tiles one pass of its scan takes
F32_TINY = float(np.finfo(np.float32).tiny)
F32_MAX = float(np.finfo(np.float32).max)
D_RANGE = (F32_TINY, F32_MAX)    # hip_ops.CLOUD_D_RANGE: every positive finite distance

# (B, H, W) and the property each covers
SHAPES = [
    (2, 7, 13),        # one partial tile, last word partial, two frames
    (1, 3, 130),       # 390 pixels: words that straddle rows, W no multiple of 4
    (1, 16, 64),       # exactly one tile
    (2, 33, 65),       # 2145 pixels: two full tiles and a tail tile
    (1, 129, 2049),    # 264321 pixels = 259 tiles: more than one scan pass (256 tiles) takes, so the carry between passes runs
]
assert -(-129 * 2049 // TILE) > SCAN_PASS

ONE_AT = (0, 63, 64, 1023, 1024, "last")
PATTERNS = ["all", "none"] + [f"one@{p}" for p in ONE_AT] + ["empty_words", "empty_tiles", "bern0.03", "bern0.5", "bern0.97"]
BERNOULLI = {"bern0.03": 0.03, "bern0.5": 0.5, "bern0.97": 0.97}


def pattern_exists(name: str, B: int, H: int, W: int) -> bool:
    HW = H * W
    if name.startswith("one@") and name != "one@last":
        return int(name[4:]) < HW
    if name == "empty_tiles":
        return HW > TILE
    return True


def keep_pattern(name: str, B: int, H: int, W: int, seed: int = 0) -> np.ndarray:
    """-> bool [B, H, W], the keep pattern `name` (seeded per frame where it is random)."""
    HW = H * W
    k = np.zeros((B, HW), dtype=bool)
    p = np.arange(HW)
    for b in range(B):
        rng = np.random.default_rng([seed, b, HW])
        if name == "all":
            k[b] = True
        elif name == "none":
            pass
        elif name.startswith("one@"):
            k[b, HW - 1 if name == "one@last" else int(name[4:])] = True
        elif name == "empty_words":          # every other 64-pixel word empty, the others half full; frame 1 the other way round
            k[b] = ((p // 64) % 2 == b % 2) & (rng.random(HW) < 0.5)
        elif name == "empty_tiles":          # even tiles empty (frame 1: odd tiles), the others half full
            k[b] = ((p // TILE) % 2 != b % 2) & (rng.random(HW) < 0.5)
        else:
            k[b] = rng.random(HW) < BERNOULLI[name]
    return k.reshape(B, H, W)


def unit_rays(H: int, W: int, seed: int = 1) -> np.ndarray:
    r = np.random.default_rng([seed, H, W]).standard_normal((3, H, W))
    return (r / np.linalg.norm(r, axis=0, keepdims=True)).astype(np.float32)


def positive_inv(B: int, H: int, W: int, bf: float, seed: int = 2) -> np.ndarray:
    """inv = bf / dist for distances log-uniform in [0.5, 100]."""
    rng = np.random.default_rng([seed, B, H, W])
    dist = np.exp(rng.random((B, H, W)) * np.log(200.0) + np.log(0.5))
    return (bf / dist).astype(np.float32)


# name -> settings of make_case: the variations of the GPU bit test
VARIANTS = {
    "plain_bf1":        dict(bf=1.0),
    "gate1_mask2":      dict(n_gates=1, mask="hw"),
    "gate4_mask3":      dict(n_gates=4, mask="bhw"),
    "step23":           dict(step=(2, 3), n_gates=1),
    "colour":           dict(C=3, A=0, mask="hw"),
    "colour_attrs":     dict(C=3, A=2, n_gates=4, bf=1.0),
    "colour_required":  dict(C=3, A=2, require_colour=True, no_colour=-1.0, step=(2, 3), mask="bhw"),
    "attrs_only":       dict(A=2, n_gates=1),
    "record16":         dict(C=3, A=10, n_gates=1),
    "drange":           dict(d_range=(2.0, 40.0), A=2),
}
VARIANT_SHAPES = [(2, 7, 13), (2, 33, 65)]
N_CAMS = 3


def make_case(B, H, W, seed=0, bf=96.0, n_gates=0, mask=None, step=(1, 1), C=0, A=0, require_colour=False, no_colour=0.0,
              d_range=D_RANGE, capacity=None, p_mask=0.8, p_valid=0.4) -> dict:
    """A seeded case: every array numpy, fp32 / bool."""
    rng = np.random.default_rng([seed, B, H, W, n_gates, C, A])
    case = dict(B=B, H=H, W=W, bf=float(bf), step=tuple(step), d_range=tuple(d_range), require_colour=require_colour,
                no_colour=float(no_colour), rays=unit_rays(H, W), inv=positive_inv(B, H, W, bf, seed + 2))
    case["mask"] = None if mask is None else rng.random((H, W) if mask == "hw" else (B, H, W)) < p_mask
    case["gates"] = [(rng.random((B, H, W)).astype(np.float32), 0.1, 0.9) for _ in range(n_gates)]
    case["attrs"] = [rng.standard_normal((B, H, W)).astype(np.float32) for _ in range(A)]
    if C:
        case["warped"] = rng.random((B, N_CAMS, C, H, W)).astype(np.float32)
        case["valid"] = rng.random((B, N_CAMS, H, W)) < p_valid
    else:
        case["warped"] = case["valid"] = None
    case["capacity"] = (-(-H // step[0])) * (-(-W // step[1])) if capacity is None else int(capacity)
    return case


def distance(case) -> np.ndarray:
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.float32(case["bf"]) / case["inv"].astype(np.float32)


def keep_reference(case) -> np.ndarray:
    """-> bool [B, H, W]."""
    B, H, W = case["B"], case["H"], case["W"]
    sy, sx = case["step"]
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    keep = np.broadcast_to((i % sy == 0) & (j % sx == 0), (B, H, W)).copy()
    if case["mask"] is not None:
        keep &= np.broadcast_to(case["mask"] != 0, (B, H, W))
    d = distance(case)
    with np.errstate(invalid="ignore"):
        keep &= np.isfinite(d) & (d >= np.float32(case["d_range"][0])) & (d <= np.float32(case["d_range"][1]))
        for g, lo, hi in case["gates"]:
            keep &= (g >= np.float32(lo)) & (g <= np.float32(hi))
    if case["require_colour"]:
        keep &= case["valid"].any(axis=1)
    return keep


def records_reference(case) -> np.ndarray:
    """-> fp32 [B, H * W, R]: the record of every pixel, kept or not."""
    B, H, W = case["B"], case["H"], case["W"]
    with np.errstate(invalid="ignore", over="ignore"):
        xyz = case["rays"][None] * distance(case)[:, None]                       # [B, 3, H, W]
    parts = [xyz]
    if case["warped"] is not None:
        valid, warped = case["valid"], case["warped"]
        first = valid.argmax(axis=1)                                            # the lowest valid camera (0 when none)
        col = np.take_along_axis(warped, first[:, None, None].repeat(warped.shape[2], axis=2), axis=1)[:, 0]
        parts.append(np.where(valid.any(axis=1)[:, None], col, np.float32(case["no_colour"])).astype(np.float32))
    if case["attrs"]:
        parts.append(np.stack(case["attrs"], axis=1))
    return np.concatenate(parts, axis=1).astype(np.float32).transpose(0, 2, 3, 1).reshape(B, H * W, -1)


def pack_reference(case):
    """-> (points: list of [written_b, R] fp32, index: list of [written_b] int32, counts [B, 2] int32)."""
    keep, rec = keep_reference(case).reshape(case["B"], -1), records_reference(case)
    points, index, counts = [], [], np.zeros((case["B"], 2), np.int32)
    for b in range(case["B"]):
        idx = np.flatnonzero(keep[b])
        counts[b] = (min(len(idx), case["capacity"]), len(idx))
        idx = idx[:case["capacity"]]
        points.append(rec[b][idx])
        index.append(idx.astype(np.int32))
    return points, index, counts


def pack_loop(case):
    """The same, pixel by pixel in plain Python (tiny cases only)."""
    B, H, W = case["B"], case["H"], case["W"]
    f = np.float32
    points, index, counts = [], [], np.zeros((B, 2), np.int32)
    for b in range(B):
        pts, idx, kept = [], [], 0
        for i in range(H):
            for j in range(W):
                if i % case["step"][0] or j % case["step"][1]:
                    continue
                m = case["mask"]
                if m is not None and not (m[i, j] if m.ndim == 2 else m[b, i, j]):
                    continue
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    d = f(case["bf"]) / case["inv"][b, i, j]
                    if not (np.isfinite(d) and d >= f(case["d_range"][0]) and d <= f(case["d_range"][1])):
                        continue
                    if not all(g[b, i, j] >= f(lo) and g[b, i, j] <= f(hi) for g, lo, hi in case["gates"]):
                        continue
                    cam = None
                    if case["valid"] is not None:
                        cam = next((n for n in range(case["valid"].shape[1]) if case["valid"][b, n, i, j]), None)
                    if case["require_colour"] and cam is None:
                        continue
                    kept += 1
                    if kept > case["capacity"]:
                        continue
                    r = [case["rays"][c, i, j] * d for c in range(3)]
                if case["warped"] is not None:
                    r += [f(case["no_colour"]) if cam is None else case["warped"][b, cam, c, i, j] for c in range(case["warped"].shape[2])]
                r += [a[b, i, j] for a in case["attrs"]]
                pts.append(r)
                idx.append(i * W + j)
        points.append(np.array(pts, dtype=np.float32).reshape(len(pts), -1))
        index.append(np.array(idx, dtype=np.int32))
        counts[b] = (min(kept, case["capacity"]), kept)
    return points, index, counts


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                                                         b.view(np.int32) if b.dtype == np.float32 else b)
