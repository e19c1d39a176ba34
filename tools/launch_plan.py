#!/usr/bin/env python3
"""The library's launch plan without a GPU: build the host objects of a source tree, link them with clang++ against the recording
stand-in for the HIP runtime (launch_plan_hip.cpp) and run the driver (launch_plan.cpp) -- every entry point over valid and invalid
levels, each launch printed as kernel / grid / block / LDS / stream.  Two revisions compute the same thing when their plans are equal.

  launch_plan.py run TREE OUT [--sanitize] [--resource-log LOG] [--objdir DIR]
                                     build TREE's csrc/api_*.hip (its own build.py flags; objects already in DIR are reused), write the plan
  launch_plan.py diff A B                                         compare two plans: launches (kernels by demangled name and template
                                                                  arguments, whatever their parameter types) and return codes, then messages
"""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def run(tree, out, sanitize=False, resource_log=None, objdir=None):
    spec = importlib.util.spec_from_file_location("tree_build", os.path.join(tree, "mga_yolo_amd", "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    hipcc = B.hipcc_path()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "clang++")
    inc = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "include")
    host = ["-O1", "-g"] + SAN if sanitize else ["-O1"]
    with tempfile.TemporaryDirectory() as tmp:
        def unit(src):
            obj = os.path.join(objdir or tmp, src[:-4] + ".o")
            if os.path.exists(obj):
                return obj
            extra = [f for s in SAN for f in ("-Xarch_host", s)] if sanitize else []
            subprocess.run([hipcc] + B.BASE_FLAGS + B.UNIT_FLAGS.get(src, []) + extra + ["-c", os.path.join(B.CSRC, src), "-o", obj], check=True)
            return obj
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4)) as ex:
            objs = list(ex.map(unit, B.sources()))
        for name in ("launch_plan_hip", "launch_plan"):
            objs.append(os.path.join(tmp, name + ".o"))
            subprocess.run([clang, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", inc, "-I", os.path.join(tree, "include")] + host +
                           ["-c", os.path.join(HERE, name + ".cpp"), "-o", objs[-1]], check=True)
        exe = os.path.join(tmp, "launch_plan")
        subprocess.run([clang] + (SAN if sanitize else []) + objs + ["-o", exe], check=True)
        with open(out, "w") as f:
            for occupancy in ("4", "0"):            # k_gate eligible / never eligible (the answer is cached per process)
                subprocess.run([exe, occupancy], stdout=f, check=True)
    reached = set(re.findall(r"^  launch (\S+)", open(out).read(), re.M))
    print(f"{out}: {sum(1 for _ in open(out))} lines, {len(reached)} distinct kernels launched")
    if resource_log:
        built = set(re.findall(r"Function Name: (\S+)", open(resource_log).read()))
        print(f"{len(reached & built)} of the {len(built)} kernels in {resource_log} reached; not reached:")
        names = subprocess.run(["c++filt"], input="\n".join(sorted(built - reached)), capture_output=True, text=True).stdout
        print("\n".join("  " + n for n in names.split("\n") if n))


def demangled(path):
    """The plan's lines with every kernel as its demangled name and template arguments, without the parameter list: a kernel whose
    argument block changed its type between two revisions is still the same kernel."""
    text = open(path).read()
    names = sorted(set(re.findall(r"^  (?:launch|attribute) (\S+)", text, re.M)))
    plain = subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    table = dict(zip(names, plain))
    return re.sub(r"^(  (?:launch|attribute) )(\S+)", lambda m: m.group(1) + table[m.group(2)], text, flags=re.M).splitlines()


def diff(a, b):
    split = lambda line: re.match(r"(.* -> -?\d+) ?(.*)$", line).groups() if " -> " in line and not line.startswith("  ") else (line, "")
    A, Bl = [split(l) for l in demangled(a)], [split(l) for l in demangled(b)]
    plan = sum(x[0] != y[0] for x, y in zip(A, Bl)) + abs(len(A) - len(Bl))
    msgs = sorted({(x[1], y[1]) for x, y in zip(A, Bl) if x[0] == y[0] and x[1] != y[1]})
    print(f"{len(A)} / {len(Bl)} lines; {plan} differ in kernel, grid, block, LDS, stream or return code; {len(msgs)} distinct message differences")
    for x, y in msgs:
        print(f"  - {x}\n  + {y}")
    return 1 if plan else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "run":
        opt = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None
        run(os.path.abspath(sys.argv[2]), sys.argv[3], "--sanitize" in sys.argv, opt("--resource-log"), opt("--objdir"))
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
