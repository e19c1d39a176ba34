"""What tools/check_dropin_spade.py recorded when the reference's own model factory built ``configs/models/yolov8_spade.yaml`` after
``mga_yolo_amd.install(strict=True)`` (tests/golden/spade_dropin_report.json), and what can be re-checked here without the reference."""
import json
import os

from conftest import GOLDEN


def test_reference_factory_builds_this_maskspade():
    from mga_yolo_amd import MaskSPADE
    R = json.load(open(os.path.join(GOLDEN, "spade_dropin_report.json")))
    assert R["yaml"].endswith("yolov8_spade.yaml") and len(R["spade_layers"]) == 3
    assert R["blocks_are_ours"] and R["late_import_is_ours"] and R["deepcopy_ok"] and R["uninstall_restores"]
    assert R["state_keys_equal"] and R["state_values_equal_same_seed"] and R["cross_load_strict"]
    assert R["eval_forward_rel_diff"] <= 1e-6 and R["train_forward_rel_diff"] <= 1e-6
    assert "mga_yolo.nn.modules.masked_spade" in R["patched_modules"]
    assert any(m.endswith("ultralytics.nn.tasks") for m in R["patched_modules"])
    for i in map(str, R["spade_layers"]):
        L = R["layers"][i]
        assert L["cls"] == "mga_yolo_amd.module.MaskSPADE" and L["np"] == L["ref_np"] and len(L["f"]) == 2
        m = MaskSPADE(**{k: v for k, v in L["cfg"].items()})                 # the recorded constructor state builds the recorded state_dict
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == L["state"]
        assert sum(p.numel() for p in m.parameters()) == L["np"] and m.scale_name == L["scale_name"]
