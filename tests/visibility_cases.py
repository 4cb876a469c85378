"""Cases and CPU restatement (torch fp32) of the camera range images and the visibility test (mvs_gi_amd/dropin/visibility.py,
csrc/visibility.hip).  TEST INFRASTRUCTURE ONLY.  Steps 1-5 are the closed forms of oracle.grid_oracle in the composition of
tests/reproject_cases.py (tests/test_visibility_host.py shows that views() returns reproject_cases.compose's grid and validity
bit for bit on its rigs); rigs, ranges and camera parameters are that module's.

Definition (include/mvsgi.h, "camera range images and visibility"), frame b, pixel (i, j), camera n; fp32, one IEEE operation each:
  1. v = inv[b, i, j], d = bf / v, p = rays * d, q = T_n p, (g, in_fov), valid_n: steps 1-5 of the back-projection
  2. live = 0 < v <= FLT_MAX and d <= FLT_MAX      (a NaN, zero, negative or infinite v is not live)
  3. r2 = (qx qx + qy qy) + qz qz
  4. cx = clamp(int(floor(((gx + 1) * float(Wz)) * 0.5)), 0, Wz - 1), cy likewise with Hz
  5. splat iff live and valid_n and mask != 0: z2[b, n, cy, cx] = min(., r2), from +inf; footprint 2: the four cells
     (clamp(x0 + dx), clamp(y0 + dy)), dx, dy in {0, 1}, x0 = floor(((gx + 1) * float(Wz) - 1) * 0.5), y0 likewise
  6. visible_n = live and valid_n and r2 <= z2[b, n, cy, cx] * k2, k2 = fp32((1 + tol)^2), at the cell of step 4
  7. n_visible = sum_n visible_n
  8. range = sqrt(z2)
"""
import numpy as np
import torch

import reproject_cases as RC
from oracle import grid_oracle as G

TOL = 0.02
FLT_MAX = float(np.finfo(np.float32).max)
BAD_INV = (0.0, -1.0, float("nan"), float("inf"))

# name: the rig of a reproject case (`base`: its cameras and poses), frames, map, buffer, the seeded fraction of inv that is one of BAD_INV
CASES = {
    "tail": dict(base="tail_u8", B=2, hw=(6, 10), zshape=(12, 20), bad=0.08, seed=511),          # row tail
    "odd_buffer": dict(base="eq_f32c3", B=2, hw=(8, 16), zshape=(5, 7), bad=0.05, seed=521),     # vector form, odd Wz
    "eight": dict(base="eight_u8", B=2, hw=(1, 7), zshape=(2, 7), bad=0.0, seed=531),            # eight cameras, one row
    "one_cell": dict(base="tail_u8", B=2, hw=(6, 10), zshape=(1, 1), bad=0.05, seed=541),        # every pixel of a camera contends for one word
    "b3": dict(base="tail_u8", B=3, hw=(7, 13), zshape=(14, 13), bad=0.05, seed=551),
}
# the launch's geometry: 1200 threads per frame and camera, several blocks, every wave busy
LARGE = {"waves": dict(base="tail_u8", B=3, hw=(48, 100), zshape=(96, 100), bad=0.02, seed=561)}
ALL = {**CASES, **LARGE}


def k2(tol: float) -> np.float32:
    """fp32((1 + tol)^2), rounded once from double"""
    return np.float32((1.0 + float(tol)) * (1.0 + float(tol)))


def spec(name: str) -> dict:
    c = ALL[name]
    b = RC.CASES[c["base"]]
    return dict(c, N=b["N"], all_eq=b["all_eq"], models=[RC.is_double_sphere(c["base"], n) for n in range(b["N"])])


def rays(hw) -> torch.Tensor:
    return G.rays_panorama(np.ones(1, np.float32), RC.LON, RC.LAT, tuple(hw))[:, 0]


def transforms(poses) -> torch.Tensor:
    return torch.stack([torch.linalg.inv(p.to(torch.float64)).to(torch.float32) for p in poses])


def make_inputs(name: str) -> dict:
    """-> dict(inv [B, H, W] fp32 = 96 / d with d log-uniform in 0.5 ... 100 m and the seeded bad values, mask_hw uint8 [H, W],
    mask_frames uint8 [B, H, W])"""
    c = ALL[name]
    rng = np.random.default_rng(c["seed"])
    H, W = c["hw"]
    d = np.exp(rng.uniform(np.log(0.5), np.log(100.0), size=(c["B"], H, W))).astype(np.float32)
    inv = np.float32(RC.BF) / d
    flat = inv.reshape(-1)
    if c["bad"]:
        pos = rng.permutation(flat.size)[:max(int(round(c["bad"] * flat.size)), len(BAD_INV))]
        flat[pos] = np.asarray(BAD_INV, np.float32)[np.arange(pos.size) % len(BAD_INV)]
    mask_hw = (rng.random((H, W)) < 0.7).astype(np.uint8)
    mask_frames = (rng.random((c["B"], H, W)) < 0.7).astype(np.uint8) * np.uint8(3)              # any non-zero byte selects
    return dict(inv=torch.from_numpy(inv), mask_hw=torch.from_numpy(mask_hw), mask_frames=torch.from_numpy(mask_frames))


def views(inv: torch.Tensor, ray_table: torch.Tensor, T: torch.Tensor, double_sphere, bf: float = RC.BF) -> dict:
    """Steps 1-3 on the CPU -> dict(grid [B, N, H, W, 2], valid [B, N, H, W], live [B, H, W], r2 [B, N, H, W]).
    double_sphere[n]: camera n is RC's double-sphere camera, else equirectangular."""
    B, H, W = inv.shape
    d = RC.distance(inv, bf)
    xyz = ray_table.unsqueeze(0) * d.unsqueeze(1)
    live = (inv > 0) & (inv <= FLT_MAX) & (d <= FLT_MAX)
    grids, fovs, r2s = [], [], []
    for n, ds in enumerate(double_sphere):
        q = G.transform_points(T[n].unsqueeze(0).expand(B, 4, 4).contiguous(), xyz.unsqueeze(2))
        if ds:
            g, m = G.grid_double_sphere(q, RC.DS_PARAMS, RC.DS_CALIB)
        else:
            g, m = G.grid_equirect(q), torch.ones((B, 1, H, W), dtype=torch.bool)
        grids.append(g[:, 0])
        fovs.append(m[:, 0])
        qx, qy, qz = q[:, 0, 0], q[:, 1, 0], q[:, 2, 0]
        r2s.append((qx * qx + qy * qy) + qz * qz)
    grid, in_fov = torch.stack(grids, dim=1), torch.stack(fovs, dim=1)
    valid = in_fov & (grid[..., 0].abs() <= 1) & (grid[..., 1].abs() <= 1)
    return dict(grid=grid, valid=valid, live=live, r2=torch.stack(r2s, dim=1))


def _cell(g: torch.Tensor, n: int) -> torch.Tensor:
    return torch.clamp(torch.floor(((g + 1.0) * float(n)) * 0.5), 0, n - 1).to(torch.int64)


def _lower(g: torch.Tensor, n: int) -> torch.Tensor:
    return torch.floor(((g + 1.0) * float(n) - 1.0) * 0.5)


def restate(v: dict, zshape, tol: float = TOL, footprint: int = 1, mask=None) -> dict:
    """Steps 4-8 from views() -> dict(z2, range [B, N, Hz, Wz], visible bool [B, N, H, W], n_visible uint8 [B, H, W], splat bool).
    The minimum is taken by a plain loop-free scatter (numpy's minimum.at): the order of the points cannot matter.  range is the
    correctly rounded root, RN_fp32(sqrt(float64(z2)))."""
    Hz, Wz = zshape
    grid, valid, live, r2 = v["grid"], v["valid"], v["live"], v["r2"]
    B, N, H, W = valid.shape
    ok = valid & live.unsqueeze(1)
    splat = ok if mask is None else ok & (mask != 0).expand(B, H, W).unsqueeze(1)
    zero = torch.zeros_like(r2)
    gx, gy = torch.where(ok, grid[..., 0], zero), torch.where(ok, grid[..., 1], zero)
    cx, cy = _cell(gx, Wz), _cell(gy, Hz)
    plane = (torch.arange(B).view(B, 1, 1, 1) * N + torch.arange(N).view(1, N, 1, 1)) * (Hz * Wz)
    z2 = np.full(B * N * Hz * Wz, np.inf, np.float32)
    if footprint == 1:
        cells = [(cx, cy)]
    else:
        x0, y0 = _lower(gx, Wz), _lower(gy, Hz)
        cells = [(torch.clamp(x0 + float(dx), 0, Wz - 1).to(torch.int64), torch.clamp(y0 + float(dy), 0, Hz - 1).to(torch.int64))
                 for dy in (0, 1) for dx in (0, 1)]
    for sx, sy in cells:
        at = (plane + sy * Wz + sx)[splat].numpy()
        np.minimum.at(z2, at, r2[splat].numpy())
    z2 = torch.from_numpy(z2)
    nearest = z2[(plane + cy * Wz + cx).reshape(-1)].view(B, N, H, W)
    visible = ok & (r2 <= nearest * torch.tensor(k2(tol)))
    cnt = torch.zeros((B, H, W), dtype=torch.uint8)
    for n in range(N):
        cnt = cnt + visible[:, n].to(torch.uint8)
    z2 = z2.view(B, N, Hz, Wz)
    return dict(z2=z2, range=exact_root(z2), visible=visible, n_visible=cnt, splat=splat)


def exact_root(z2) -> torch.Tensor:
    """RN_fp32(sqrt(float64(z2))): the correctly rounded fp32 root (53 bits against 24: the double rounding is harmless)."""
    z = z2.cpu().numpy() if isinstance(z2, torch.Tensor) else np.asarray(z2)
    assert z.dtype == np.float32
    return torch.from_numpy(np.sqrt(z.astype(np.float64)).astype(np.float32))


def build(name: str, footprint: int = 1, mask: str = None, tol: float = TOL) -> dict:
    """A case on the CPU: inputs, views and restatement; asserts the conditions the case exists for."""
    s = spec(name)
    inp = make_inputs(name)
    v = views(inp["inv"], rays(s["hw"]), transforms(RC.poses(s["base"])), s["models"])
    m = None if mask is None else inp[mask]
    r = restate(v, s["zshape"], tol, footprint, m)
    ok = v["valid"] & v["live"].unsqueeze(1)
    occluded = ok & ~r["visible"]
    if mask is None and footprint == 1:
        for b in range(s["B"]):                       # in every frame some point is seen and (but on the widest buffer) some is hidden
            assert bool(r["visible"][b].any()), (name, b)
        assert bool(occluded.any()) or name == "eight", name
    if s["bad"]:
        bad = ~v["live"]
        assert int(bad.sum()) >= len(BAD_INV) and not bool(r["visible"].movedim(1, -1)[bad].any()), name
    return dict(spec=s, inp=inp, views=v, restated=r, occluded=occluded)


# ---- analytic scenes (tests/test_visibility_host.py): three equirectangular cameras on a ring, map 40 x 160 ----
def ring_scene(inv: torch.Tensor, radius: float = 0.1, n_cams: int = 3) -> dict:
    """views() of a [B, H, W] inverse-distance map (bf = 1) seen from n_cams equirectangular cameras on G.ring_poses(n_cams, radius)."""
    assert inv.dim() == 3
    return views(inv, rays(inv.shape[1:]), transforms(G.ring_poses(n_cams, radius)), [False] * n_cams, bf=1.0)
