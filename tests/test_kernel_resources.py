"""tools/kernel_resources.py `diff` on synthetic compiler remarks: the line per kernel, the exit status, an empty selection."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "kernel_resources.py")
TAIL = " [-Rpass-analysis=kernel-resource-usage]"


def _log(path, kernels):
    """kernels: {name: (VGPRs, SGPRs, scratch, LDS, waves/SIMD)}, written the way hipcc prints its remarks"""
    lines = []
    for name, (v, s, scratch, lds, occ) in kernels.items():
        at = "x.cuh:1:1: remark: "
        lines += [at + "Function Name: " + name + TAIL, "    1 | __global__ void k();", at + f"    TotalSGPRs: {s}" + TAIL,
                  at + f"    VGPRs: {v}" + TAIL, at + "    AGPRs: 0" + TAIL, at + f"    ScratchSize [bytes/lane]: {scratch}" + TAIL,
                  at + f"    Occupancy [waves/SIMD]: {occ}" + TAIL, at + f"    LDS Size [bytes/block]: {lds}" + TAIL]
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def _diff(*args):
    return subprocess.run([sys.executable, TOOL, "diff", *args], capture_output=True, text=True)


def test_register_moves_are_listed_and_do_not_fail(tmp_path):
    parent = _log(tmp_path / "p.log", {"k_one": (40, 30, 0, 1024, 8), "k_two": (90, 60, 0, 0, 5)})
    branch = _log(tmp_path / "b.log", {"k_one": (40, 30, 0, 1024, 8), "k_two": (88, 62, 0, 0, 5)})
    r = _diff(parent, branch)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = r.stdout.splitlines()
    assert rows[0].split() == ["k_one", "(40,", "30,", "0,", "1024,", "8)", "parent=(40,", "30,", "0,", "1024,", "8)", "SAME"]
    assert rows[1].startswith("k_two") and "(88, 62, 0, 0, 5)" in rows[1] and "parent=(90, 60, 0, 0, 5)" in rows[1] and rows[1].endswith("DIFFERENT")
    assert rows[2] == "2 kernels; 1 DIFFERENT; 0 differ in scratch, LDS or waves/SIMD"


def test_scratch_lds_occupancy_or_a_missing_kernel_fail(tmp_path):
    base = {"k_one": (40, 30, 0, 1024, 8)}
    parent = _log(tmp_path / "p.log", base)
    for i, fig in enumerate([(40, 30, 16, 1024, 8), (40, 30, 0, 2048, 8), (40, 30, 0, 1024, 7)]):
        r = _diff(parent, _log(tmp_path / f"b{i}.log", {"k_one": fig}))
        assert r.returncode == 1 and "1 differ in scratch, LDS or waves/SIMD" in r.stdout, r.stdout + r.stderr
    r = _diff(parent, _log(tmp_path / "more.log", {**base, "k_new": (10, 10, 0, 0, 8)}))
    assert r.returncode == 1 and "(absent)" in r.stdout, r.stdout + r.stderr


def test_only_selects_and_an_empty_selection_is_no_error(tmp_path):
    parent = _log(tmp_path / "p.log", {"k_one": (40, 30, 0, 1024, 8), "k_two": (90, 60, 0, 0, 5)})
    branch = _log(tmp_path / "b.log", {"k_one": (40, 30, 0, 1024, 8), "k_two": (90, 60, 0, 0, 4)})
    assert _diff(parent, branch).returncode == 1
    r = _diff(parent, branch, "--only", "k_one")
    assert r.returncode == 0 and "k_two" not in r.stdout, r.stdout + r.stderr
    r = _diff(parent, branch, "--only", "no_such_kernel")
    assert r.returncode == 0 and r.stdout.strip() == "0 kernels; 0 DIFFERENT; 0 differ in scratch, LDS or waves/SIMD", r.stdout + r.stderr
    empty = tmp_path / "empty.log"
    empty.write_text("")
    assert _diff(str(empty), str(empty)).returncode == 0
