"""Drop-in registration: make the reference engine build THIS MaskCBAM.

``parse_model`` resolves the YAML string "MaskCBAM" with ``globals()[m]`` inside its own module and picks the
``[feat, mask]`` branch by identity ``m is MaskCBAM`` against the same module global (U/nn/tasks.py:1676-1682, 1733-1739), so
rebinding that global -- before ``MGAModel(...)`` / ``YOLO(...)`` is constructed -- is enough.  The reference holds TWO
module objects made from that one file: ``ultralytics.nn.tasks`` (the vendored tree is put on sys.path,
mga_yolo/__init__.py:16-41) and ``mga_yolo.external.ultralytics.ultralytics.nn.tasks`` -- ``MGAModel`` derives from the
``DetectionModel`` of the SECOND (mga_yolo/model/model.py:10), so both are patched: every loaded module of the reference
that binds one of the class names to a class of that name is rebound.  The trainer's alpha logger finds the blocks by
``isinstance`` against ``mga_yolo.nn.modules.masked_cbam.MaskCBAM`` imported at call time (mga_yolo/model/trainer.py:286-295),
``MGAModel.init_criterion`` imports the loss classes at call time (model/model.py:103-117): covered by the same rule.
Nothing else in the reference changes.  ``install(nms=True)`` -- opt-in -- also rebinds ``non_max_suppression`` in the reference's
``ultralytics.utils.ops`` modules: the validator and the predictor look it up through ``ops.`` at call time (U/models/yolo/detect/val.py,
predict.py), so the unchanged ``postprocess`` then runs ``detpost.non_max_suppression``.  ``install(match=True)`` -- opt-in as well -- rebinds
``DetectionValidator.update_metrics`` in the reference's ``ultralytics.models.yolo.detect.val`` modules to ``detmatch.update_metrics``: one matching call
and one read-back per batch; subclasses (``MGAValidator``) reach it through ``super()``.  ``install(ap=True)`` -- opt-in too -- rebinds ``ap_per_class`` in
the reference's ``ultralytics.utils.metrics`` modules (``DetMetrics.process`` finds it as a module global at call time) to ``detap``'s.
``install(preprocess=True)`` -- opt-in too -- rebinds ``DetectionTrainer.preprocess_batch`` and ``DetectionValidator.preprocess`` on the reference's classes to
``image.preprocess_batch`` / ``image.preprocess``: the batch's bytes become the network's input in one launch.  See INTEGRATION.md; ``oracle/check_dropin.py`` runs this against the real factory.
"""
from __future__ import annotations

import importlib
import sys
from typing import Dict, List

from .module import MGAMaskHead, MaskCBAM, MaskECA, MaskSPADE
from .segloss import SegLossConfig, SegmentationLoss

# modules imported (if importable) before the scan, so that install() may run before OR after the reference is imported
_PRELOAD = ("ultralytics.nn.tasks", "mga_yolo.external.ultralytics.ultralytics.nn.tasks",
            "mga_yolo.nn.modules.masked_cbam", "mga_yolo.nn.modules.masked_eca", "mga_yolo.nn.modules.masked_spade", "mga_yolo.nn.modules.segmentation",
            "mga_yolo.nn.losses.segmentation", "mga_yolo.model.model")
_PREFIXES = ("ultralytics", "mga_yolo")
_TASKS_SUFFIX = "ultralytics.nn.tasks"
# name -> replacement.  parse_model treats MaskCBAM, MaskECA and MaskSPADE through the same branch (U/nn/tasks.py:1733)
_CLASSES: Dict[str, type] = {"MaskCBAM": MaskCBAM, "MaskECA": MaskECA, "MaskSPADE": MaskSPADE, "MGAMaskHead": MGAMaskHead,
                             "SegmentationLoss": SegmentationLoss, "SegLossConfig": SegLossConfig}


def register(name: str, cls: type) -> None:
    """Add a (reference class name -> replacement) pair for later install() calls (used by optional rows, e.g. MGAMaskHead)."""
    _CLASSES[name] = cls


def _is_reference_module(name: str) -> bool:
    return any(name == p or name.startswith(p + ".") for p in _PREFIXES) and not name.startswith("mga_yolo_amd")


def install(strict: bool = False, nms: bool = False, match: bool = False, confusion: bool = False, ap: bool = False,
            preprocess: bool = False) -> List[str]:
    """Rebind the block classes in every loaded reference module that exports them.  Returns the module names patched.
    ``strict=True`` raises unless the module whose ``parse_model`` builds ``MGAModel`` (the one providing
    ``mga_yolo.model.model.DetectionModel``; ``ultralytics.nn.tasks`` when mga_yolo is absent) was patched.
    ``nms=True`` also rebinds ``non_max_suppression`` in the reference's ``ultralytics.utils.ops`` modules (see ``_install_nms``),
    ``match=True`` ``DetectionValidator.update_metrics`` in its ``ultralytics.models.yolo.detect.val`` modules (see ``_install_match``).
    ``confusion=True`` -- with ``match=True`` only, else ValueError -- sets the switch under which that ``update_metrics`` forms a plotted
    validation's confusion matrix on the device, one call per batch (``detmatch._CONFUSION_ON``; uninstall() clears it).
    ``ap=True`` also rebinds ``ap_per_class`` in the reference's ``ultralytics.utils.metrics`` modules (see ``_install_ap``).
    ``preprocess=True`` also rebinds ``DetectionTrainer.preprocess_batch`` and ``DetectionValidator.preprocess`` in the reference's
    ``ultralytics.models.yolo.detect.train`` / ``.val`` modules to ``image``'s: one launch for /255, element type and resize (see
    ``_install_preprocess``)."""
    if confusion and not match:
        raise ValueError("install(confusion=True) needs match=True: the confusion matrix is formed by the replacement update_metrics")
    for name in (_PRELOAD + (_OPS_PRELOAD if nms else ()) + (_VAL_PRELOAD if match else ()) + (_METRICS_PRELOAD if ap else ())
                 + (_TRAIN_PRELOAD + _VAL_PRELOAD if preprocess else ())):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except Exception:
                pass
    patched = []
    for name, mod in list(sys.modules.items()):
        if mod is None or not _is_reference_module(name):
            continue
        is_tasks = name.endswith(_TASKS_SUFFIX)
        hit = False
        for cls_name, cls in _CLASSES.items():
            cur = mod.__dict__.get(cls_name, _MISSING) if hasattr(mod, "__dict__") else _MISSING
            if cur is cls:
                hit = True
                continue
            # a class of that name (the reference's own), or the `= None` left by tasks.py's guarded import (U/nn/tasks.py:72-90)
            if (isinstance(cur, type) and cur.__name__ == cls_name) or (is_tasks and cur is None and cls_name in ("MaskCBAM", "MaskECA", "MaskSPADE", "MGAMaskHead")):
                _UNDO.append((name, cls_name, cur))
                setattr(mod, cls_name, cls)
                hit = True
        if hit:
            patched.append(name)
    if nms:
        patched += _install_nms()
    if match:
        patched += _install_match()
    if confusion:
        from . import detmatch
        if not detmatch._CONFUSION_ON:
            _UNDO.append((detmatch.__name__, "_CONFUSION_ON", False))
            detmatch._CONFUSION_ON = True
    if ap:
        patched += _install_ap()
    if preprocess:
        patched += _install_preprocess()
    if strict:
        need = _factory_module_name()
        if need not in patched:
            raise RuntimeError(f"{need} (the module whose parse_model builds the model) could not be patched: "
                               f"patched = {patched}")
    return sorted(patched)


_OPS_PRELOAD = ("ultralytics.utils.ops", "mga_yolo.external.ultralytics.ultralytics.utils.ops")
_OPS_SUFFIX = "ultralytics.utils.ops"


def _install_nms() -> List[str]:
    """Rebind ``non_max_suppression`` in every loaded ``ultralytics.utils.ops`` module of the reference (it holds two module objects of that
    file, as it does of tasks.py).  uninstall() restores them."""
    from .detpost import non_max_suppression
    done = []
    for name, mod in list(sys.modules.items()):
        if mod is None or not _is_reference_module(name) or not name.endswith(_OPS_SUFFIX):
            continue
        cur = mod.__dict__.get("non_max_suppression", _MISSING)
        if cur is _MISSING or cur is non_max_suppression:
            continue
        _UNDO.append((name, "non_max_suppression", cur))
        mod.non_max_suppression = non_max_suppression
        done.append(name)
    return done


_VAL_PRELOAD = ("ultralytics.models.yolo.detect.val", "mga_yolo.external.ultralytics.ultralytics.models.yolo.detect.val")
_VAL_SUFFIX = "ultralytics.models.yolo.detect.val"


def _install_match() -> List[str]:
    """Rebind ``DetectionValidator.update_metrics`` in every loaded ``ultralytics.models.yolo.detect.val`` module of the reference (two module
    objects of that file, as of ops.py).  The class keeps its identity, so subclasses reach the replacement through ``super()``; the method it
    replaces is kept in ``detmatch._ORIGINALS``, where the replacement finds it for what it does not cover (a subclass with a
    ``_process_batch`` of its own: masks, keypoints, rotated boxes).  uninstall() restores it: the undo record names the class,
    ``<module>:DetectionValidator``."""
    from .detmatch import _ORIGINALS, update_metrics
    done = []
    for name, mod in list(sys.modules.items()):
        if mod is None or not _is_reference_module(name) or not name.endswith(_VAL_SUFFIX):
            continue
        cls = mod.__dict__.get("DetectionValidator", _MISSING)
        if not isinstance(cls, type):
            continue
        cur = cls.__dict__.get("update_metrics", _MISSING)
        if cur is _MISSING or cur is update_metrics:
            continue
        _UNDO.append((name + ":DetectionValidator", "update_metrics", cur))
        _ORIGINALS[cls] = cur
        cls.update_metrics = update_metrics
        done.append(name)
    return done


_METRICS_PRELOAD = ("ultralytics.utils.metrics", "mga_yolo.external.ultralytics.ultralytics.utils.metrics")
_METRICS_SUFFIX = "ultralytics.utils.metrics"


def _install_ap() -> List[str]:
    """Rebind ``ap_per_class`` in every loaded ``ultralytics.utils.metrics`` module of the reference (two module objects of that file, as of
    ops.py).  Each module gets a function of its own, so that ``plot=True`` reaches that module's ``plot_pr_curve`` / ``plot_mc_curve``.
    uninstall() restores them."""
    from .detap import reference_replacement
    done = []
    for name, mod in list(sys.modules.items()):
        if mod is None or not _is_reference_module(name) or not name.endswith(_METRICS_SUFFIX):
            continue
        cur = mod.__dict__.get("ap_per_class", _MISSING)
        if cur is _MISSING or getattr(cur, "_mga_replacement", False):
            continue
        _UNDO.append((name, "ap_per_class", cur))
        mod.ap_per_class = reference_replacement(mod)
        done.append(name)
    return done


_TRAIN_PRELOAD = ("ultralytics.models.yolo.detect.train", "mga_yolo.external.ultralytics.ultralytics.models.yolo.detect.train")
_TRAIN_SUFFIX = "ultralytics.models.yolo.detect.train"


def _install_preprocess() -> List[str]:
    """Rebind ``DetectionTrainer.preprocess_batch`` in every loaded ``ultralytics.models.yolo.detect.train`` module of the reference and
    ``DetectionValidator.preprocess`` in every loaded ``...detect.val`` module (two module objects of each file, as of ops.py).  The classes
    keep their identity, so ``MGATrainer`` and ``MGAValidator`` reach the replacements through ``super()``; the methods they replace are kept
    in ``image._ORIGINALS``, where the replacements find them for a batch whose ``img`` is not uint8.  uninstall() restores them."""
    from . import image
    done = []
    for suffix, cls_name, attr, new in ((_TRAIN_SUFFIX, "DetectionTrainer", "preprocess_batch", image.preprocess_batch),
                                        (_VAL_SUFFIX, "DetectionValidator", "preprocess", image.preprocess)):
        for name, mod in list(sys.modules.items()):
            if mod is None or not _is_reference_module(name) or not name.endswith(suffix):
                continue
            cls = mod.__dict__.get(cls_name, _MISSING)
            if not isinstance(cls, type):
                continue
            cur = cls.__dict__.get(attr, _MISSING)
            if cur is _MISSING or cur is new:
                continue
            _UNDO.append((name + ":" + cls_name, attr, cur))
            image._ORIGINALS[(cls, attr)] = cur
            setattr(cls, attr, new)
            done.append(name)
    return done


_MISSING = object()
_UNDO: list = []          # (module name, attribute, previous value) of every rebinding install() made


def uninstall() -> int:
    """Put back what install() replaced (A/B runs against the reference's own classes).  Returns the number of names restored."""
    n = 0
    while _UNDO:
        name, attr, old = _UNDO.pop()
        name, _, member = name.partition(":")                    # "<module>:<class>": an attribute of a class of the module
        owner = sys.modules.get(name)
        if owner is not None and member:
            owner = getattr(owner, member, None)
        if owner is not None:
            setattr(owner, attr, old)
            n += 1
    return n


def _factory_module_name() -> str:
    mm = sys.modules.get("mga_yolo.model.model")
    if mm is None:
        try:
            mm = importlib.import_module("mga_yolo.model.model")
        except Exception:
            mm = None
    dm = getattr(mm, "DetectionModel", None)
    return dm.__module__ if isinstance(dm, type) else "ultralytics.nn.tasks"
