"""Build recipe for libmgacbam.so (hand-written HIP for gfx950, plain C ABI -- include/mgacbam.h).

The library is built IN-TREE with hipcc (no torch C++ extension: the ABI carries no torch types, and the
image's hipcc (ROCm 7.2) differs from torch's bundled HIP (7.0); at run time the .so resolves
``libamdhip64.so.7`` to the copy torch has already loaded, so both share one HIP runtime and streams).

One translation unit per kernel family (csrc/api_*.hip), compiled in parallel into build/obj/<tag>/ and linked into
mga_yolo_amd/libmgacbam.so; a unit is recompiled only when it or a header it includes (transitively) changed.
"""
from __future__ import annotations

import hashlib
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libmgacbam.so")
OBJ_ROOT = os.path.join(ROOT, "build", "obj")
ARCH = "gfx950"
_INC = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)
# -fno-slp-vectorize: clang's SLP vectoriser turns the kernels' per-pixel FMA chains into v_pk_fma_f32 whose scalar operands then need
# v_mov / lane spills (k_head_bwd_act: 342 v_mov + 275 spills).  Without it -- five interleaved A/B pairs on one MI355X -- the
# MaskCBAM step is 1.7 % faster (0.2010 -> 0.1976 ms) and the layer-loop slice 1.6 % (0.3989 -> 0.3926); on the mask-head unit alone: 0.4 %.
# -O2 rather than -O3: the MaskCBAM step is the same (0.1997 / 0.1995 ms), the layer-loop slice 1.9 % faster (0.3941 -> 0.3867 ms, four pairs): the
# mask-head and loss kernels lose what -O3's extra unrolling / hoisting cost them in registers.  (Measured and not adopted: the scheduler
# strategies max-ilp (k_gate +3 us), iterative-minreg (+6 %), max-memory-clause (same); -fno-vectorize (same).)
BASE_FLAGS = ["-O2", "-std=c++17", f"--offload-arch={ARCH}", "-fPIC", "-Wno-pass-failed", "-fno-slp-vectorize"]
INCLUDE = os.path.join(ROOT, "include")
# extra flags per translation unit.  api_match.hip: include/ext/mgamatch.h names "mgatargets.h", which lies one directory above it; its IoU
# is the reference's fp32 expression operation by operation, so no product may be contracted into a fused multiply-add
# api_confusion.hip: the same for include/ext/mgaconfusion.h, which shares that IoU (csrc/match_common.cuh)
# api_ap.hip: the same for include/ext/mgaap.h; its fp64 divisions, products and sums are numpy's operation by operation
# api_image.hip: the same for include/ext/mgaimage.h; the bilinear blend of the image resize is spelled operation by operation, so that both
# destination layouts give the same bits
# api_det.hip, api_nms.hip: include/ext/mgamaps.h names "mgadet.h" and "mganms.h" the same way
UNIT_FLAGS: dict = {"api_match.hip": ["-I", INCLUDE, "-ffp-contract=off"], "api_confusion.hip": ["-I", INCLUDE, "-ffp-contract=off"],
                    "api_ap.hip": ["-I", INCLUDE, "-ffp-contract=off"], "api_image.hip": ["-I", INCLUDE, "-ffp-contract=off"],
                    "api_det.hip": ["-I", INCLUDE], "api_nms.hip": ["-I", INCLUDE]}


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.startswith("api_") and f.endswith(".hip"))


def _includes(path: str, seen: set) -> set:
    """Files `path` includes with quotes, transitively (relative to the including file, else to include/)."""
    if path in seen or not os.path.exists(path):
        return seen
    seen.add(path)
    for inc in _INC.findall(open(path).read()):
        near = os.path.normpath(os.path.join(os.path.dirname(path), inc))
        _includes(near if os.path.exists(near) else os.path.join(INCLUDE, inc), seen)      # (-I include: UNIT_FLAGS)
    return seen


def dependencies(src: str | None = None):
    """Everything a unit (default: the whole library) is compiled from."""
    units = [src] if src else sources()
    deps = set()
    for u in units:
        _includes(os.path.join(CSRC, u), deps)
    return sorted(deps)


def hipcc_path() -> str:
    p = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(p):
        raise RuntimeError("hipcc not found: libmgacbam.so cannot be built on this machine")
    return p


def is_stale(lib: str = LIB) -> bool:
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(d) > t for d in dependencies())


def build(force: bool = False, verbose: bool = False, resource_log: str | None = None, defines=(), out: str | None = None,
          jobs: int | None = None) -> str:
    """Compile csrc/api_*.hip for gfx950 and link mga_yolo_amd/libmgacbam.so (or `out`); returns the library path.
    `defines`: extra -D flags (A/B builds: they get an object directory of their own)."""
    lib = out or LIB
    if not force and not is_stale(lib):
        return lib
    hipcc = hipcc_path()
    flags = BASE_FLAGS + list(defines)
    if resource_log:
        flags.insert(0, "-Rpass-analysis=kernel-resource-usage")
    tag = hashlib.sha1((" ".join(flags) + repr(sorted(UNIT_FLAGS.items()))).encode()).hexdigest()[:10]
    objdir = os.path.join(OBJ_ROOT, tag)
    os.makedirs(objdir, exist_ok=True)

    def compile_one(src: str):
        obj = os.path.join(objdir, src[:-4] + ".o")
        log = obj + ".log"
        deps = dependencies(src)
        if not force and os.path.exists(obj) and all(os.path.getmtime(d) <= os.path.getmtime(obj) for d in deps):
            return obj, (open(log).read() if os.path.exists(log) else ""), 0
        cmd = [hipcc] + flags + UNIT_FLAGS.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            if os.path.exists(obj):
                os.remove(obj)
            return obj, r.stderr, r.returncode
        open(log, "w").write(r.stderr)
        return obj, r.stderr, 0

    srcs = sources()
    with ThreadPoolExecutor(max_workers=jobs or min(len(srcs), os.cpu_count() or 4)) as ex:
        results = list(ex.map(compile_one, srcs))
    if resource_log:
        with open(resource_log, "w") as f:
            f.write("".join(err for _, err, _ in results))
    bad = [(s, err) for s, (_, err, rc) in zip(srcs, results) if rc]
    if bad:
        raise RuntimeError("hipcc failed:\n" + "\n".join(f"--- {s}\n{err[-4000:]}" for s, err in bad))
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", lib] + [o for o, _, _ in results]
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n" + r.stderr[-4000:])
    return lib


if __name__ == "__main__":
    import sys
    print(build(force="--force" in sys.argv, verbose=True))
