"""Slow / fast vector instructions on the steady-state path of ONE column step of a myers_edit_kernel instantiation, from its ISA.

    hipcc <otter_amd/build.py's FLAGS without -fPIC> -S --cuda-device-only -o myers_edit.s otter_amd/csrc/myers_edit.hip
    python scripts/isa_step.py myers_edit.s ILi1ELi8 [step] [-v]      (build container, no GPU needed; -v lists the instructions)

The step loop is unrolled by 8; a step starts at the pair of lane rotates of `score` / `hout` (ds_bpermute for 8- and 32-lane groups).  `step`
picks the unrolled copy: 1 (default) and 2 are plain steps, 0 also moves the prefetched text group and 4 loads the next one.  The walk follows
the path a lane takes in the middle of its superblock: every exec-mask branch that skips rare code (moving to the next superblock, first-column
initialisation, the last-column harvest) is taken; the first branch that would skip the whole step (the in-band test) is not.  Instruction
classes and their issue cost come from profiles/r04_valu_peak.json through scripts/isa_mix.py: fast ~2.2 SIMD cycles per wave64 instruction,
slow ~4.2."""
import importlib.util
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(HERE, "isa_mix.py"))
isa_mix = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa_mix)

args = [a for a in sys.argv[1:] if a != "-v"]
verbose = "-v" in sys.argv
path, key = args[0], args[1]
k = int(args[2]) if len(args) > 2 else 1
table = isa_mix.cost_table()
lines = open(path).read().split("\n")
start = [i for i, l in enumerate(lines) if l.startswith("_ZN") and "myers_edit_kernel" + key in l.split(":")[0]][0]
end = [i for i, l in enumerate(lines) if i > start and ".end_amdhsa_kernel" in l][0]
L = lines[start:end]
rot = [i for i, l in enumerate(L) if "ds_bpermute_b32" in l]
pairs = []
i = 0
while i + 1 < len(rot):
    if rot[i + 1] - rot[i] <= 4:
        pairs.append(rot[i]); i += 2
    else:
        i += 1
if len(pairs) < k + 2:
    sys.exit("no ds_bpermute pairs: only the 8- and 32-lane instantiations are handled")
labels = {m.group(1): i for i, l in enumerate(L) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
pc, stop = pairs[k], pairs[k + 1]


def falls_into_next_step(label):
    j = labels[label] + 1
    while j < len(L) and not L[j].startswith(".LBB"):
        if j == stop:
            return True
        j += 1
    return False


slow = fast = guard = 0
cycles = 0.0
in_band_seen = False
while pc < stop and guard < 5000:
    guard += 1
    t = L[pc].split()
    if t and t[0].startswith("v_"):
        c = isa_mix.classify(t[0], table)
        fast += c < 3.0; slow += c >= 3.0; cycles += c
        if verbose:
            print("  %s %s" % ("F" if c < 3.0 else "S", L[pc].strip()))
    elif t and t[0].startswith("ds_") and verbose:
        print("  L %s" % L[pc].strip())
    if t and t[0] == "s_branch":
        pc = labels[t[1]]; continue
    if t and t[0].startswith("s_cbranch"):
        if falls_into_next_step(t[1]) and not in_band_seen:
            in_band_seen = True
        else:
            pc = labels[t[1]]; continue
    pc += 1
print("myers_edit_kernel<%s> step %d: %d vector instructions, %d slow + %d fast, %.0f SIMD cycles" % (key, k, slow + fast, slow, fast, cycles))
