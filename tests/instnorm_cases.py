"""Seeded cases of the norm_type='instance' goldens, shared by tools/make_instnorm_goldens.py (which runs the REFERENCE's
modules built with norm_type='instance') and tests/test_gpu_instnorm.py (which runs the HIP path on the regenerated,
bit-identical inputs).  Only outputs and input / weight digests are stored."""
from mvs_gi_amd.configs import CONFIGS, DIST_8L, DIST_10, PathConfig

_small = dict(feat_hw=(16, 64), mask_hw=(64, 256), cv_hw=(8, 32))


def _inst(cfg: PathConfig, affine: bool = False) -> PathConfig:
    d = dict(cfg.__dict__)
    d.update(norm_type="instance", norm_affine=affine)
    return PathConfig(**d)


# name -> dict(cfg, seed, batch, grid_kind, grid_mask_dtype, gains)
SMALL_CASES = {
    "instnorm_std": dict(cfg=_inst(CONFIGS["G16V"].scaled(dist_cands=DIST_8L, **_small)), seed=21, batch=2,
                         grid_kind="smooth", grid_mask_dtype="bool", gains=(1.0, 4.0)),
    "instnorm_cat": dict(cfg=_inst(CONFIGS["E8-light"].scaled(dist_cands=DIST_8L, **_small)), seed=22, batch=1,
                         grid_kind="smooth", grid_mask_dtype="bool", gains=(1.0, 4.0)),
    "instnorm_wide_reg": dict(cfg=_inst(PathConfig("G16VV-small", 3, "std", 16, 96, DIST_8L, **_small)), seed=23, batch=1,
                              grid_kind="smooth", grid_mask_dtype="bool", gains=(4.0,)),
    # odd pyramid (D 10/5/3/2, H 12/6/3/2, W 40/20/10/5): the second trilinear resize of common_modules.py:343-350
    "instnorm_odd": dict(cfg=_inst(CONFIGS["G16V"].scaled(feat_hw=(16, 64), mask_hw=(64, 256), cv_hw=(12, 40), dist_cands=DIST_10)),
                         seed=24, batch=1, grid_kind="smooth", grid_mask_dtype="bool", gains=(1.0, 4.0)),
    # nn.InstanceNorm3d(c, affine=True) swapped into the reference's modules, seeded gamma / beta
    "instnorm_affine": dict(cfg=_inst(CONFIGS["G16V"].scaled(dist_cands=DIST_8L, **_small), affine=True), seed=25, batch=1,
                            grid_kind="smooth", grid_mask_dtype="bool", gains=(1.0, 4.0)),
}

FULL_CASES = {
    "instnorm_full_G16V": dict(cfg=_inst(CONFIGS["G16V"]), seed=26, batch=1, grid_kind="smooth", grid_mask_dtype="bool",
                               gains=(0.25, 1.0)),
}

# SimpleFeatExtraction(norm_type='instance') on 64 x 256 images, alone and chained into the instnorm_std path geometry
EXTRACTOR_CASE = dict(cfg=_inst(CONFIGS["G16V"].scaled(dist_cands=DIST_8L, **_small)), seed=27, batch=2)
