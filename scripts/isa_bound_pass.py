"""The score loops of the gap-affine bound pass (wfa_affine_bound1_kernel, wfa_affine.hip), from the ISA: what one score issues.

    python scripts/isa_bound_pass.py                          (compiles this tree's wfa_affine.hip; build container, no GPU needed)
    python scripts/isa_bound_pass.py PARENT_TREE OUT.json     (the same for a second tree, both written to OUT.json: profiles/bound_pass_isa.json)

A score loop is found from the loop structure LLVM annotates on the block labels: a loop whose own blocks (not those of its inner loops) hold
the leader's wave-wide maximum (a DPP `row_bcast:31`).  A kernel has one per probe kind that has its own loop:
the packed loop probes LDS (`ds_read`), the byte loop HBM (`global_load`); a loop that holds both serves both kinds.  Of each loop:
  * scores per trip: the `v_max3_i32` of the recurrence (one per score);
  * the body: every instruction outside the loop's inner loops, every path counted once, by unit; the blocks that move the band (five and more
    whole-wave DPP shifts: taken when the leader left lanes [24, 40)) are reported apart and left out of the per-score figure;
  * the inner loops are the rolled probe loops: the instructions of one trip.  Where the body holds no LDS read of its own the first probe of a
    score is a trip of the inner loop as well (`probe_inline` false);
  * per score = body / scores (+ one inner trip where the probe is not inline); each further probe of a score adds one inner trip;
  * `vmcnt` waits and private-memory accesses of body and inner loops: a packed loop has no reason for either.
Registers, scratch and LDS are the compiler's metadata; waves per SIMD follow from the LDS of a block (160 KB per CU, four SIMDs) and the
vector registers (512 per SIMD lane), capped at 8."""
import importlib.util
import json
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
KERNEL = "wfa_affine_bound1_kernel"
LDS_PER_CU = 160 * 1024


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def metadata(text):
    """{mangled kernel name: {field: int}} from the amdhsa metadata"""
    out, cur, pending = {}, None, {}
    for ln in text.split("\n"):
        m = re.match(r"\s+\.(group_segment_fixed_size|private_segment_fixed_size|sgpr_count|sgpr_spill_count|vgpr_count|vgpr_spill_count|max_flat_workgroup_size):\s+(\d+)", ln)
        if m:
            (cur if cur is not None else pending)[m.group(1)] = int(m.group(2))
            continue
        m = re.match(r"\s+\.name:\s+(_Z\S+)", ln)
        if m:                                   # the fields of one kernel stand in alphabetical order around its name
            cur = out.setdefault(m.group(1), {})
            cur.update(pending); pending = {}
            continue
        if re.match(r"\s+- \.", ln) or ln.startswith("amdhsa."):
            cur, pending = None, {}
    return {k: v for k, v in out.items() if KERNEL in k}


def units(ins):
    c = {"valu": 0, "salu": 0, "lds": 0, "vmem": 0, "branch": 0, "wait": 0, "nop": 0}
    for x in ins:
        op = x.split()[0]
        if op.startswith("s_waitcnt"): c["wait"] += 1
        elif op.startswith("s_nop"): c["nop"] += 1
        elif op.startswith(("s_cbranch", "s_branch")): c["branch"] += 1
        elif op.startswith("s_"): c["salu"] += 1
        elif op.startswith("v_"): c["valu"] += 1
        elif op.startswith("ds_"): c["lds"] += 1
        elif op.startswith(("global_", "flat_", "buffer_", "scratch_")): c["vmem"] += 1
    c["all"] = len(ins)
    return c


def annotated_blocks(L):
    """[(innermost loop header or None, {depth: enclosing header}, [instructions])] per basic block, from LLVM's loop comments on the block labels"""
    out, i = [], 0
    while i < len(L):
        ln = L[i]
        m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)", ln)
        if m:
            label, rest, chain = m.group(1), m.group(2), {}
            j = i
            while True:                                     # a loop header's comment runs over the following lines
                for pm in re.finditer(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", rest):
                    chain[int(pm.group(2))] = pm.group(1)
                hm = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", rest)
                if hm:
                    chain[int(hm.group(1))] = label
                im = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", rest)
                if im:
                    chain[int(im.group(2))] = im.group(1)
                if j + 1 < len(L) and re.match(r"^\s+;\s+(=>|Parent Loop|Child Loop)", L[j + 1]):
                    j += 1; rest = L[j]
                else:
                    break
            i = j
            out.append([chain[max(chain)] if chain else None, chain, []])
        elif out and re.match(r"\s+[a-z][a-z0-9_]+", ln) and not ln.lstrip().startswith((";", ".")):
            out[-1][2].append(ln.strip())
        i += 1
    return out


def score_loops(L):
    blocks = annotated_blocks(L)
    depth_of, parent = {}, {}
    for inner, chain, _ in blocks:
        for d, h in chain.items():
            depth_of[h] = d
    for inner, chain, _ in blocks:                          # a block "in Loop" names its innermost loop only: parents come from the headers' chains
        for d, h in chain.items():
            if d - 1 in chain:
                parent[h] = chain[d - 1]
    own = lambda h: [b for b in blocks if b[0] == h]
    heads = [h for h in depth_of if any("row_bcast:31" in x for b in own(h) for x in b[2])]
    out = []
    for h in sorted(heads, key=lambda x: int(x.split("_")[1])):
        mine = own(h)
        shifts = lambda b: sum(("wave_shl:1" in x or "wave_shr:1" in x) for x in b[2])
        ins_own = [x for b in mine if shifts(b) < 5 for x in b[2]]
        ins_move = [x for b in mine if shifts(b) >= 5 for x in b[2]]
        probes = []
        for h2 in sorted((x for x in depth_of if parent.get(x) == h), key=lambda x: int(x.split("_")[1])):
            ii = [x for b in blocks if h2 in b[1].values() for x in b[2]]
            probes.append({"kind": "lds" if any(x.startswith("ds_read") for x in ii) else "hbm", "trip": units(ii),
                           "vmcnt_waits": sum(x.startswith("s_waitcnt") and "vmcnt" in x for x in ii), "scratch": sum(x.startswith("scratch_") for x in ii)})
        scores = sum(x.startswith("v_max3_i32") for x in ins_own)
        inline = any(x.startswith("ds_read") for x in ins_own)
        kinds = sorted({p["kind"] for p in probes} | ({"lds"} if inline else set()))
        body_u = units(ins_own)
        lds_trip = next((p["trip"] for p in probes if p["kind"] == "lds"), None)
        per = {k: body_u[k] / max(scores, 1) + (0 if inline or lds_trip is None else lds_trip[k]) for k in ("valu", "salu", "lds", "branch", "wait", "nop", "all")}
        out.append({"probes": kinds, "scores_per_trip": scores, "probe_inline": inline, "body": body_u, "band_move_blocks": units(ins_move),
                    "leader_reductions": sum("row_bcast:31" in x for x in ins_own), "inner_loops": probes,
                    "per_score": {k: round(v, 1) for k, v in per.items()}, "further_probe": lds_trip,
                    "vmcnt_waits": sum(x.startswith("s_waitcnt") and "vmcnt" in x for x in ins_own + ins_move),
                    "scratch": sum(x.startswith("scratch_") for x in ins_own + ins_move)})
    return out


def analyse(text):
    """{template arguments: metadata, occupancy, score loops}"""
    R = _load("isa_reg_loop")
    out = {}
    for name, meta in metadata(text).items():
        args = tuple(int(x) for x in re.findall(r"Li(\d+)E", name.split(KERNEL)[1].split("EEv")[0]))
        wpb = meta.get("max_flat_workgroup_size", 256) // 64
        lds = meta.get("group_segment_fixed_size", 0)
        blocks_lds = LDS_PER_CU // lds if lds else 32
        granule = (meta["vgpr_count"] + 7) // 8 * 8
        waves = min(8, 512 // max(granule, 1), blocks_lds * wpb // 4)
        out[args] = {"meta": meta, "waves_per_block": wpb, "blocks_per_cu_by_lds": blocks_lds, "waves_per_simd": waves,
                     "loops": score_loops(R.kernel_lines(text, name))}
    return out


def compile_tree(tree, asm):
    mix = _load("isa_mix")
    return mix.hipcc_S(os.path.join(tree, "otter_amd", "csrc", "wfa_affine.hip"), asm)


def report(tree):
    with tempfile.TemporaryDirectory(prefix="isa_bound_") as tmp:
        asm = os.path.join(tmp, "wfa_affine.s")
        compile_tree(tree, asm)
        return analyse(open(asm).read())


def show(tag, rep):
    for args, r in sorted(rep.items()):
        m = r["meta"]
        print("%s %s<%s>: %d VGPR (%d spilled), %d SGPR (%d spilled), private segment %d bytes, LDS %d bytes per block of %d waves, %d waves per SIMD" % (
            tag, KERNEL, ", ".join(map(str, args)), m["vgpr_count"], m["vgpr_spill_count"], m["sgpr_count"], m["sgpr_spill_count"], m["private_segment_fixed_size"],
            m["group_segment_fixed_size"], r["waves_per_block"], r["waves_per_simd"]))
        for lp in r["loops"]:
            p, f = lp["per_score"], lp["further_probe"]
            print("  %s loop: %d score(s) per trip, first probe %s; per score %.1f instructions (vector %.1f, scalar %.1f, LDS %.1f, branch %.1f, wait %.1f, nop %.1f)%s; "
                  "vmcnt waits %d, private-memory accesses %d" % ("+".join(lp["probes"]), lp["scores_per_trip"], "inline" if lp["probe_inline"] else "in the rolled loop",
                                                                  p["all"], p["valu"], p["salu"], p["lds"], p["branch"], p["wait"], p["nop"],
                                                                  "; each further probe %d (vector %d, scalar %d)" % (f["all"], f["valu"], f["salu"]) if f else "",
                                                                  lp["vmcnt_waits"] + sum(q["vmcnt_waits"] for q in lp["inner_loops"] if q["kind"] == "lds"),
                                                                  lp["scratch"] + sum(q["scratch"] for q in lp["inner_loops"])))


def main():
    root = os.path.dirname(HERE)
    res = {"result": report(root)}
    show("result", res["result"])
    if len(sys.argv) > 2:
        res["parent"] = report(sys.argv[1])
        show("parent", res["parent"])
        doc = {"what": "score loops of %s from hipcc -S with the library's flags (scripts/isa_bound_pass.py): per-score instruction counts are the loop body, every path "
                       "once and the band-move blocks left out, divided by the scores of a trip, plus one trip of the rolled probe loop where the first probe is not inline" % KERNEL}
        for t in res:
            doc[t] = {", ".join(map(str, k)): v for k, v in res[t].items()}
        json.dump(doc, open(sys.argv[2], "w"), indent=1, sort_keys=True)
        print(sys.argv[2])


if __name__ == "__main__":
    main()
