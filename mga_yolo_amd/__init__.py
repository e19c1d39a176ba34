"""mga_yolo_amd -- MI355X-native (gfx950) implementation of ONE hot path of MGA-YOLO: the mask-guided CBAM block
(reference mga_yolo/nn/modules/masked_cbam.py) forward + backward, behind the reference's own module interface.

    from mga_yolo_amd import MaskCBAM, install
    install()                      # the reference's parse_model now builds this class for "MaskCBAM" YAML layers

Layout: ``csrc/`` hand-written HIP kernels + the C ABI of ``include/mgacbam.h``; ``_lib`` ctypes binding (no fallback);
``functional`` autograd entry points; ``module`` the nn.Module mirror; ``dp`` data-parallel gradient exchange (RCCL).
"""
from .functional import BlockConfig, EcaConfig, HandoffTimeout, handoff_report, mask_cbam, mask_cbam_pyramid, mask_eca, mask_eca_pyramid, mask_head, mask_head_pyramid, prob_mask_gate, resize_nearest  # noqa: F401
from .functional import SpadeConfig, mask_spade, mask_spade_pyramid  # noqa: F401
from .functional import GateConfig, gate_state, prob_mask_gate_pyramid  # noqa: F401
from .functional import mask_pyramid  # noqa: F401
from .install import install, uninstall  # noqa: F401
from .plan import EcaPyramidPlan, PyramidPlan, SpadePyramidPlan  # noqa: F401
from .slice import SlicePlan  # noqa: F401
from .module import MGAMaskHead, MaskCBAM, MaskECA, MaskSPADE, MaskSPADEConfig, ProbMaskGater  # noqa: F401
from .segloss import SegLossConfig, SegmentationLoss, kendall_combine  # noqa: F401
from .optim import BucketOptimizer, OptConfig  # noqa: F401
from .detloss import DetLossPlan, V8DetectionLoss, detection_loss  # noqa: F401
from .detpost import DetPostPlan, detect_postprocess, non_max_suppression  # noqa: F401
from .detmatch import DetMatchPlan, match_detections  # noqa: F401
from .detconfusion import ConfusionPlan, confusion_matrix, reference_conf  # noqa: F401
from .detap import DetApPlan, ap_per_class  # noqa: F401
from .image import ImagePlan, image_batch, multi_scale_size  # noqa: F401

__all__ = ["MaskCBAM", "MaskECA", "MaskSPADE", "MaskSPADEConfig", "SpadeConfig", "mask_spade", "mask_spade_pyramid", "MGAMaskHead", "mask_head", "mask_head_pyramid", "ProbMaskGater", "BlockConfig", "EcaConfig", "mask_cbam", "mask_cbam_pyramid", "mask_eca",
           "mask_eca_pyramid", "prob_mask_gate", "prob_mask_gate_pyramid", "GateConfig", "gate_state", "resize_nearest", "mask_pyramid", "install", "uninstall", "SegLossConfig", "SegmentationLoss", "kendall_combine", "HandoffTimeout", "handoff_report",
           "PyramidPlan", "EcaPyramidPlan", "SpadePyramidPlan", "SlicePlan", "BucketOptimizer", "OptConfig",
           "detection_loss", "V8DetectionLoss", "DetLossPlan", "detect_postprocess", "non_max_suppression", "DetPostPlan",
           "match_detections", "DetMatchPlan",
           "confusion_matrix", "ConfusionPlan", "reference_conf",
           "ap_per_class", "DetApPlan",
           "image_batch", "multi_scale_size", "ImagePlan"]
__version__ = "0.1.0"
