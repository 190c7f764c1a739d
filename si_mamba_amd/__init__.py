"""si_mamba_amd -- MI355X-native SI-Mamba hot path (selective scan, causal conv1d, spectral ordering).

Importing this package does not load the HIP library; the first op call does, and raises if
``libsimamba_hip.so`` is missing (there is no CPU fallback -- see DESIGN.md).
"""
from .causal_conv1d import causal_conv1d_fn
from .selective_scan import selective_scan_fn
from .mamba_simple import Mamba
from .block import Block, MixerModel, create_block, DropPath
from .rms_norm import RMSNorm
from . import spectral
from .shim import install_shim
from .emd import earth_movers_distance
from .sinkhorn import sinkhorn_divergence
from .seg_metrics import SHAPENETPART, PartSegMetrics, PartTable, part_seg_eval
from .svm import OvOLinearSVC, evaluate_svm
from . import manifold
from .manifold import TSNE
from . import transforms
from .transforms import (AugmentState, Compose, PointcloudJitter, PointcloudRandomInputDropout, PointcloudRotate,
                         PointcloudScale, PointcloudScaleAndTranslate, PointcloudTranslate, RandomHorizontalFlip,
                         sample_and_augment)
from .vote import vote_logits
from . import corruptions
from .corruptions import KINDS, SEVERITY, corrupt, evaluate_robustness
from . import mixing
from .mixing import cutmix, mixed_cross_entropy, mixup, pointwolf
from . import data
from . import optim
from .data import Batch, DeviceDataset, DeviceLoader
from ._lib import deterministic, deterministic_enabled, set_deterministic

__all__ = ["data", "Batch", "DeviceDataset", "DeviceLoader", "transforms", "AugmentState", "Compose", "PointcloudJitter", "PointcloudRandomInputDropout",
           "PointcloudRotate", "PointcloudScale", "PointcloudScaleAndTranslate", "PointcloudTranslate",
           "RandomHorizontalFlip", "sample_and_augment", "vote_logits",
           "corruptions", "KINDS", "SEVERITY", "corrupt", "evaluate_robustness",
"SHAPENETPART", "PartSegMetrics", "PartTable", "part_seg_eval","causal_conv1d_fn", "selective_scan_fn", "Mamba", "Block", "MixerModel", "create_block",
           "DropPath", "RMSNorm", "spectral", "install_shim", "deterministic", "deterministic_enabled",
           "set_deterministic", "earth_movers_distance", "sinkhorn_divergence", "OvOLinearSVC", "evaluate_svm", "manifold",
           "TSNE", "optim", "mixing", "cutmix", "pointwolf", "mixup", "mixed_cross_entropy"]
