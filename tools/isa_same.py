#!/usr/bin/env python3
"""Is the device code the same after a translation unit was split?  Compares every kernel of <before.s> with its definition in the
<after.s> files (gfx950 assembly made with the flags of tools/isa_count.py: hipcc ... -S --cuda-device-only): the instructions and
labels of the body (comments dropped, basic-block labels renumbered in order of appearance) and NumVgprs / NumSgprs / ScratchSize /
LDSByteSize / Occupancy.  Prints one markdown row per kernel whose mangled name matches the regular expression <pattern>, a summary
of the others, and exits 1 on any difference, on a kernel defined twice or on one that is missing or new.
   python tools/isa_same.py <pattern> <before.s> <after.s> [<after.s> ...]"""
import os, re, subprocess, sys
FIG = ("NumVgprs", "NumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def kernels(path):
    lines = open(path).read().split("\n")
    names = set(m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel (\S+)", l) for l in lines) if m)
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if m and m.group(1) in names:
            j = i + 1
            while not lines[j].startswith(".Lfunc_end"): j += 1
            body = [t for t in (re.sub(r"\s*;.*$", "", l).rstrip() for l in lines[i + 1:j]) if t]
            order = {}
            text = re.sub(r"\.LBB\d+_\d+", lambda mo: ".LBB_%d" % order.setdefault(mo.group(0), len(order)), "\n".join(body))
            fig = {}
            for l in lines[j:j + 400]:
                mm = re.match(r"^; (?:Total)?(%s)\S*: (\d+)" % "|".join(FIG), l.strip())
                if mm: fig.setdefault(mm.group(1), int(mm.group(2)))
                if l.startswith("_Z"): break
            out[m.group(1)] = (text, tuple(fig.get(f) for f in FIG), len(body))
            i = j
        i += 1
    return out


pat, before = sys.argv[1], kernels(sys.argv[2])
after, bad = {}, 0
for p in sys.argv[3:]:
    for n, v in kernels(p).items():
        if n in after: print("defined twice:", n); bad += 1
        after[n] = v + (os.path.basename(p),)
for n in sorted(set(before) ^ set(after)): print("only before:" if n in before else "only after:", n); bad += 1
demangle = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.split("(")[0].replace("void ", "").strip()
print("| kernel | now in | instructions + labels | body | %s before | after |\n|---|---|---|---|---|---|" % " / ".join(FIG))
rest = same = 0
for n in sorted(set(before) & set(after)):
    eq = before[n][0] == after[n][0] and before[n][1] == after[n][1]
    bad += not eq
    if re.search(pat, n) or not eq:
        print("| `%s` | %s | %d | %s | %s | %s |" % (demangle(n), after[n][3], before[n][2], "equal" if before[n][0] == after[n][0] else "DIFFERS",
                                                   " / ".join(map(str, before[n][1])), " / ".join(map(str, after[n][1]))))
    else: rest += 1; same += eq
print("\n%d other kernels, %d of them equal in body and figures; %d kernels before, %d after" % (rest, same, len(before), len(after)))
sys.exit(1 if bad else 0)
