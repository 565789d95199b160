"""Code generation of two trees' kernels side by side, without a GPU.

    python scripts/isa_ab.py PARENT_TREE RESULT_TREE OUT.json file.hip [file.hip ...]

Every file is compiled in both trees by scripts/isa_mix.py's hipcc_S (the library's flags, -S --cuda-device-only) plus
-Rpass-analysis=kernel-resource-usage, and read with its kernel_insts.  Per kernel instantiation: registers, scratch, LDS and occupancy
from the compiler's remarks; static instruction counts by unit and the loop-weighted vector count (8^(loop depth), isa_mix.py's weights)
from the text.  Exit status 1 when a kernel's scratch (where the parent has none), LDS size or occupancy differs from the parent's; the
other figures are recorded, not gated."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_mix import hipcc_S, kernel_insts  # noqa: E402

REMARK = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes", "Occupancy [waves/SIMD]": "occupancy",
          "LDS Size [bytes/block]": "lds_bytes"}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] for n, d in zip(names, out)}


def unit(op):
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    return "valu" if op.startswith("v_") else "salu" if op.startswith("s_") else None


def kernels(tree, f, tmp):
    asm = os.path.join(tmp, os.path.basename(os.path.abspath(tree)) + "_" + f.replace(".hip", ".s"))
    remarks = hipcc_S(os.path.join(tree, "otter_amd", "csrc", f), asm, ["-Rpass-analysis=kernel-resource-usage"])
    res, cur = {}, None
    for ln in remarks.split("\n"):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), dict(valu=0, salu=0, lds=0, vmem=0, valu_loop_weighted=0))
        elif cur is not None and m.group(1) in REMARK:
            cur[REMARK[m.group(1)]] = int(m.group(2))
    for fn, depth, op in kernel_insts(asm):
        u = unit(op)
        if u and fn in res:
            res[fn][u] += 1
            if u == "valu":
                res[fn]["valu_loop_weighted"] += 8 ** depth
    names = demangle(sorted(res))
    return {names[k]: v for k, v in res.items()}


def main():
    parent, result, out = sys.argv[1], sys.argv[2], sys.argv[3]
    tmp = tempfile.mkdtemp(prefix="isa_ab_")
    table, bad = {}, []
    for f in sys.argv[4:]:
        kp, kr = kernels(parent, f, tmp), kernels(result, f, tmp)
        for k in sorted(set(kp) | set(kr)):
            a, b = kp.get(k), kr.get(k)
            table[k] = {"file": f, "parent": a, "result": b}
            if a is None or b is None:
                bad.append(k + ": in one tree only")
                continue
            if (a["scratch_bytes"] == 0 and b["scratch_bytes"] != 0) or a["lds_bytes"] != b["lds_bytes"] or a["occupancy"] != b["occupancy"]:
                bad.append(k + ": scratch, LDS or occupancy differs")
            table[k]["same_text_counts"] = all(a[x] == b[x] for x in ("valu", "salu", "lds", "vmem", "valu_loop_weighted"))
            print("%-64s VGPR %3d -> %3d  SGPR %3d -> %3d  scratch %d -> %d  LDS %6d -> %6d  occ %d -> %d  VALU %5d -> %5d  weighted %8d -> %8d" % (
                k[:64], a["vgprs"], b["vgprs"], a["sgprs"], b["sgprs"], a["scratch_bytes"], b["scratch_bytes"], a["lds_bytes"], b["lds_bytes"],
                a["occupancy"], b["occupancy"], a["valu"], b["valu"], a["valu_loop_weighted"], b["valu_loop_weighted"]))
    shutil.rmtree(tmp)
    json.dump({"what": "hipcc -S --cuda-device-only -Rpass-analysis=kernel-resource-usage with the library's flags, parent and result side by side; "
                       "valu / salu / lds / vmem = static instruction counts, valu_loop_weighted = vector instructions weighted 8^(loop depth)",
               "gate": "scratch stays 0 where the parent's is 0, LDS bytes and occupancy equal", "violations": bad, "kernels": table}, open(out, "w"), indent=1, sort_keys=True)
    print("violations:", bad if bad else "none")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
