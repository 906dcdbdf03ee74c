"""MI355X-native hot path of torch_semantic_segmentation: FastSCNN / ContextNet conv stacks as hand-written
HIP kernels (libtss_hip.so, include/tss_hip.h) behind the reference's nn.Module API."""
from . import models                                         # noqa: F401
from .models import set_compute_dtype                        # noqa: F401
from .ops import CrossEntropyLoss, cross_entropy, argmax_confusion, upsample_cross_entropy  # noqa: F401
from .ops import SyncBatchNorm, convert_syncbn_model, upsample_argmax_confusion  # noqa: F401
from .ops import OHEMLoss, ohem_loss, Upsample  # noqa: F401
from .ops import LovaszSoftmaxFn, LovaszSoftmaxLoss, lovasz_softmax_loss  # noqa: F401
from .ops import FocalFn, FocalLoss, focal_loss, DiceFn, DiceLoss, dice_loss  # noqa: F401
from .ops import upsample_focal_loss, upsample_dice_loss  # noqa: F401
from .ops import UpsampleGroupedCrossEntropyFn, check_sample_groups  # noqa: F401
from .ops import DistillFn, DistillationLoss, distillation_loss  # noqa: F401
from .ops import label_histogram, enet_class_weights  # noqa: F401
from .ops import TrainAugment, augment_batch, remap_labels  # noqa: F401
from .ops import multiscale_argmax_confusion, resize_flip_image  # noqa: F401
from .engine import benchmark_model, GraphedInference, MultiScaleEvaluator  # noqa: F401
from .engine import FlatOptimizer, FlatAdamW, FlatSGD, ModelEMA  # noqa: F401
from .selftrain import upsample_pseudo_labels, classmix_select, mix_batch, SelfTraining  # noqa: F401
from .selftrain import gaussian_taps, StrongAugment, strong_augment  # noqa: F401
from .ops import upsample_pixel_weighted_cross_entropy, UpsamplePixelWeightedCrossEntropyFn  # noqa: F401
from .selftrain import mix_plane  # noqa: F401

__version__ = '0.1.0'
