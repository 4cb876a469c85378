from .common_modules import NoOp, BaseConvBlk3d, ResConvBlk3d, ResizeConv3d, RELU_TYPE, NORM3D_TYPE  # noqa: F401
from .cost_volume_builder import SphericalSweepStdMasked, SphericalSweep  # noqa: F401
from .cost_volume_regulator import UNetCostVolumeRegulatorBase, UNetCostVolumeRegulator, UNetDownBlk  # noqa: F401
from .distance_regressor import DistanceRegressorWithFixedCandidates  # noqa: F401
from .torch_only import SphericalSweepStereoBase  # noqa: F401
from .feature_extractor import (BaseConvBlk2d, ResConvBlk2d, SimpleFeatExtraction, SphereConvEquirect2d,  # noqa: F401
                                SphereConvBlk, SphereEquirectFeatExtraction)
from .image_sampler import (DoubleSphereToEquirectSampler, NoOpSampler, equirect_surrogate_rays, sample_masks,  # noqa: F401
                            stack_tables)
from .reproject import Reprojector  # noqa: F401
from .cloud import CloudPacker  # noqa: F401
from .photo import PhotoConsistency  # noqa: F401
from .visibility import Visibility  # noqa: F401
from .temporal import TemporalFusion  # noqa: F401
from .tsdf import TsdfVolume  # noqa: F401
from .metrics import (Evaluator, MVSMetric, SSIMMetric, RMSEMetric, MAEMetric, BadPixelRatioMetric,  # noqa: F401
                      InverseMetricWrapper)
from .losses import (LossEvaluator, VolumeCrossEntropy, MaskedSmoothL1Loss, InBoundsBCEDistanceLoss,  # noqa: F401
                     NearFocusDistanceLoss)
from .install import install, uninstall  # noqa: F401
