"""`hipcc -Rpass-analysis=kernel-resource-usage` output (VGPR / SGPR / scratch / occupancy / LDS per kernel).

  kernel_resources.py LOG [--all]                         one line per kernel (fp32 instantiations only without --all)
  kernel_resources.py diff PARENT.log BRANCH.log [--only REGEX]
                                                          one line per kernel of the branch, by its full demangled name:
                                                          (VGPRs, SGPRs, scratch, LDS, waves/SIMD)  parent=(...)  SAME|DIFFERENT
                                                          exit status 1 when scratch, LDS or waves/SIMD differ anywhere (or a kernel is
                                                          in one log only)
"""
import re
import subprocess
import sys

FIELDS = ("VGPRs", "TotalSGPRs", r"ScratchSize \[bytes/lane\]", r"LDS Size \[bytes/block\]", r"Occupancy \[waves/SIMD\]")


def blocks(path):
    """(demangled name, report text) per kernel of the log, in the log's order."""
    parts = open(path).read().split("Function Name: ")[1:]
    # the mangled name alone: the remark's line goes on with " [-Rpass-analysis=...]", which used to travel through c++filt into the
    # printed name and, in `diff`, would be part of the key
    names = [b.split("\n")[0].split()[0] for b in parts]
    if not names:
        return []
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return list(zip(dem, parts))


def short(name):
    return re.sub(r"\(mgacbam::\w+\)", "", name).replace("mgacbam::", "").replace("void ", "")


def figure(block, key):
    m = re.search(key + r": (\d+)", block)
    return m.group(1) if m else "?"


def summary(path, only_f32=True):
    seen = set()
    for name, b in blocks(path):
        d = short(name)[:64]
        if only_f32 and ("__half" in d or "bfloat" in d):
            continue
        if d in seen:
            continue
        seen.add(d)
        print("%-66s vgpr=%4s agpr=%3s sgpr=%4s scratch=%4s occ=%s lds=%s" % (
            d, figure(b, "VGPRs"), figure(b, "AGPRs"), figure(b, "TotalSGPRs"), figure(b, FIELDS[2]), figure(b, FIELDS[4]),
            figure(b, FIELDS[3])))


def table(path):
    """{full demangled name without the parameter list: (VGPRs, SGPRs, scratch, LDS, waves/SIMD)}"""
    out = {}
    for name, b in blocks(path):
        key = re.sub(r"\(mgacbam::Group<[^()]*>\)$", "", name).replace("mgacbam::", "").replace("void ", "")
        out[key] = tuple(figure(b, f) for f in FIELDS)
    return out


def diff(parent, branch, only=None):
    P, B = table(parent), table(branch)
    names = sorted(n for n in set(P) | set(B) if not only or re.search(only, n))
    width = max((len(n) for n in names), default=0) + 2
    fmt = lambda t: "(" + ", ".join(t) + ")" if t else "(absent)"
    bad = moved = 0
    for n in names:
        p, b = P.get(n), B.get(n)
        same = p == b
        moved += not same
        bad += p is None or b is None or p[2:] != b[2:]
        print("%-*s %-26s parent=%-26s %s" % (width, n, fmt(b), fmt(p), "SAME" if same else "DIFFERENT"))
    print(f"{len(names)} kernels; {moved} DIFFERENT; {bad} differ in scratch, LDS or waves/SIMD")
    return 1 if bad else 0


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) >= 3 and a[0] == "diff":
        sys.exit(diff(a[1], a[2], a[a.index("--only") + 1] if "--only" in a else None))
    elif a:
        summary(a[0], only_f32="--all" not in a)
    else:
        sys.exit(__doc__)
