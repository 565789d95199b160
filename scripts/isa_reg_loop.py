"""The score loop of every wfa_affine_reg_kernel instantiation, from its ISA: what one slot visit issues, and what the loop waits for.

    hipcc <otter_amd/build.py's FLAGS without -fPIC> -S --cuda-device-only -o wfa_affine_reg.s otter_amd/csrc/wfa_affine_reg.hip
    python scripts/isa_reg_loop.py wfa_affine_reg.s [ILi1ELi12 ...] [-v]      (build container, no GPU needed; -v lists the loop's waits and spill reads)
    python scripts/isa_reg_loop.py                                            (compiles the file itself)

The score loop is found from the control flow, not from names: it is the smallest natural loop (header, and every block that reaches a back
edge to it without passing the header; a back edge is an edge to a block that dominates its source) that holds at least S2 `global_store_short` — the provenance stores, one per slot visit.  Of that loop:
  * `vmcnt` waits and private-memory (`scratch_*`) accesses: the sweep's provenance stores are never read back, so a score has no reason to wait
    for vector memory; a wait there (a flag or a spilled vector register read back) also waits for every store of the sweep, in order;
  * `v_swap_b32` and `v_mov_b32`: words of the wavefront changing registers (the loop runs two scores per trip, a body per score parity, so that none has to);
  * `v_readlane_b32` / `v_writelane_b32`: SGPR spill traffic, lane reads of the recurrence included (2 to 4 per slot visit are the carries and
    the end cell);
  * one slot visit = the instructions between the provenance stores of the two middle slots, every path of the visit (second probe, both end
    tests, the queue push) counted once: fast-class / slow-class vector instructions as scripts/isa_mix.py classifies them, `v_swap_b32` apart,
    scalar, LDS, waits.
Registers, spill counts and the code size are the compiler's metadata."""
import collections
import importlib.util
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
KERNEL = "wfa_affine_reg_kernel"


def _isa_mix():
    spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(HERE, "isa_mix.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def metadata(text):
    """{mangled kernel name: {field: int}} from the amdhsa metadata"""
    out, cur = {}, None
    for ln in text.split("\n"):
        m = re.match(r"\s+\.name:\s+(_Z\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.match(r"\s+\.(private_segment_fixed_size|sgpr_count|sgpr_spill_count|vgpr_count|vgpr_spill_count|agpr_count):\s+(\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    # the size of each kernel's code (`; codeLenInByte`, in the comment block behind the kernel's body)
    cur = None
    for ln in text.split("\n"):
        m = re.match(r"(_Z\S+):", ln)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r"; codeLenInByte = (\d+)", ln)
        if m and cur in out:
            out[cur].setdefault("code_bytes", int(m.group(1)))
    return {k: v for k, v in out.items() if KERNEL in k}


def kernel_lines(text, name):
    lines = text.split("\n")
    start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if ".end_amdhsa_kernel" in lines[i] or lines[i].startswith(".Lfunc_end"))
    return lines[start + 1:end]


def blocks_of(L):
    """basic blocks [(label, [instruction lines])] and the successor lists, by block index"""
    blocks = [("entry", [])]
    for ln in L:
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            blocks.append((m.group(1), []))
            continue
        if re.match(r"\s+[a-z][a-z0-9_]+", ln) and not ln.lstrip().startswith((";", ".")):
            blocks[-1][1].append(ln.strip())
    index = {b[0]: i for i, b in enumerate(blocks)}
    succ = []
    for i, (_, ins) in enumerate(blocks):
        s, fall = [], True
        for x in ins:
            t = x.split()
            if t[0] == "s_branch":
                s.append(index[t[1]]); fall = False
            elif t[0].startswith("s_cbranch"):
                s.append(index[t[1]])
            elif t[0] in ("s_endpgm", "s_setpc_b64"):
                fall = False
        if fall and i + 1 < len(blocks):
            s.append(i + 1)
        succ.append(s)
    return blocks, succ


def dominators(succ):
    """{block: set of the blocks that dominate it}, block 0 the entry (iterative; a few hundred blocks)"""
    n = len(succ)
    pred = collections.defaultdict(list)
    for a, ss in enumerate(succ):
        for b in ss:
            pred[b].append(a)
    seen, work = {0}, [0]
    while work:
        for b in succ[work.pop()]:
            if b not in seen:
                seen.add(b); work.append(b)
    dom = {b: ({0} if b == 0 else set(seen)) for b in seen}
    changed = True
    while changed:
        changed = False
        for b in sorted(seen):
            if b == 0:
                continue
            ps = [dom[p] for p in pred[b] if p in seen]
            new = set.intersection(*ps) | {b} if ps else {b}
            if new != dom[b]:
                dom[b] = new; changed = True
    return dom


def natural_loops(succ):
    """{header: set of blocks} for every back edge (an edge to a block that dominates its source), loops of one header merged.  (An edge to a block
    above its source in the layout is not enough: with two score bodies per trip the exits of the first are laid out behind the second, and
    the "loop" of such an edge is the whole kernel.)"""
    pred = collections.defaultdict(list)
    for a, ss in enumerate(succ):
        for b in ss:
            pred[b].append(a)
    dom = dominators(succ)
    loops = {}
    for a, ss in enumerate(succ):
        for h in ss:
            if a not in dom or h not in dom[a]:
                continue
            body, work = {h, a}, [a] if a != h else []
            while work:
                x = work.pop()
                for p in pred[x]:
                    if p not in body:
                        body.add(p); work.append(p)
            loops.setdefault(h, set()).update(body)
    return loops


def score_loop(L, s2):
    blocks, succ = blocks_of(L)
    best = None
    for h, body in natural_loops(succ).items():
        ins = [x for b in sorted(body) for x in blocks[b][1]]
        if sum(x.startswith("global_store_short") for x in ins) >= s2 and (best is None or len(ins) < len(best)):
            best = ins
    return best


def loop_report(ins):
    """what the issue of the score loop is about: waits on the vector-memory counter, private-memory accesses, lane reads and writes"""
    return {"instructions": len(ins),
            "vmcnt_waits": [x for x in ins if x.startswith("s_waitcnt") and "vmcnt" in x],
            "scratch": [x for x in ins if x.startswith("scratch_")],
            "v_readlane": sum(x.startswith("v_readlane_b32") for x in ins),
            "v_writelane": sum(x.startswith("v_writelane_b32") for x in ins),
            "v_swap": sum(x.startswith("v_swap_b32") for x in ins),
            "v_mov": sum(x.startswith("v_mov_b32") for x in ins),
            "prov_stores": sum(x.startswith("global_store_short") for x in ins)}


def slot_visit(L, s2, mix, table):
    """instruction classes between the provenance stores of slots S2/2 - 1 and S2/2, in layout order inside the kernel"""
    ins = [ln.strip() for ln in L if re.match(r"\s+[a-z][a-z0-9_]+", ln) and not ln.lstrip().startswith((";", "."))]
    st = [i for i, x in enumerate(ins) if x.startswith("global_store_short")]
    if len(st) < s2:
        return None
    a, b = st[s2 // 2 - 1], st[s2 // 2]
    c = collections.Counter()
    cyc = 0.0
    for x in ins[a + 1:b + 1]:
        op = x.split()[0]
        if op.startswith("v_swap"):
            c["v_swap"] += 1; cyc += 8.1
        elif op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
            c["lane"] += 1; cyc += mix.classify(op, table)
        elif op.startswith("v_"):
            k = mix.classify(op, table)
            c["fast" if k < 3.0 else "slow"] += 1; cyc += k
        elif op.startswith("s_waitcnt"):
            c["wait"] += 1
        elif op.startswith(("s_cbranch", "s_branch")):
            c["branch"] += 1
        elif op.startswith("s_"):
            c["scalar"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith("scratch_"):
            c["scratch"] += 1
        elif op.startswith(("global_", "flat_", "buffer_")):
            c["vmem"] += 1
    c["cycles"] = round(cyc)
    return dict(c)


def shape_of(name):
    m = re.search(KERNEL + r"ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", name)
    return tuple(int(x) for x in m.groups())


def analyse(text, with_visit=True):
    """per instantiation (NW, S2, SEQB, WPEU, QCAP, LB): metadata, score-loop report, slot visit"""
    mix = table = None
    if with_visit:
        mix = _isa_mix(); table = mix.cost_table()
    out = {}
    for name, meta in metadata(text).items():
        shp = shape_of(name)
        L = kernel_lines(text, name)
        loop = score_loop(L, shp[1])
        out[shp] = {"meta": meta, "loop": loop_report(loop) if loop is not None else None,
                    "visit": slot_visit(L, shp[1], mix, table) if with_visit else None}
    return out


def compile_reg(asm):
    mix = _isa_mix()
    return mix.hipcc_S(os.path.join(mix.B.CSRC, "wfa_affine_reg.hip"), asm)


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    verbose = "-v" in sys.argv
    if args and os.path.exists(args[0]):
        text = open(args[0]).read(); keys = args[1:]
    else:
        with tempfile.TemporaryDirectory(prefix="isa_reg_loop_") as tmp:
            compile_reg(os.path.join(tmp, "reg.s"))
            text = open(os.path.join(tmp, "reg.s")).read()
        keys = args
    for shp, r in sorted(analyse(text).items()):
        key = "ILi%dELi%d" % shp[:2]
        if keys and key not in keys:
            continue
        m, lp, v = r["meta"], r["loop"], r["visit"]
        print("%s<%d,%d> seq %d, %d waves/SIMD, queue %d, LB %d" % ((KERNEL,) + shp))
        print("  registers: %d VGPR (%d spilled), %d SGPR (%d spilled), private segment %d bytes, code %d bytes" % (
            m["vgpr_count"], m["vgpr_spill_count"], m["sgpr_count"], m["sgpr_spill_count"], m["private_segment_fixed_size"], m.get("code_bytes", 0)))
        if lp is None:
            print("  score loop not found"); continue
        print("  score loop: %d instructions, %d provenance stores, %d vmcnt waits, %d private-memory accesses, %d v_readlane, %d v_writelane, %d v_swap, %d v_mov" % (
            lp["instructions"], lp["prov_stores"], len(lp["vmcnt_waits"]), len(lp["scratch"]), lp["v_readlane"], lp["v_writelane"], lp["v_swap"], lp["v_mov"]))
        if v:
            print("  slot visit: " + ", ".join("%s %d" % (k, v.get(k, 0)) for k in ("slow", "fast", "lane", "v_swap", "scalar", "branch", "lds", "wait", "vmem", "scratch"))
                  + "; about %d SIMD cycles of vector issue" % v["cycles"])
        if verbose:
            for x in lp["vmcnt_waits"] + lp["scratch"]:
                print("    " + x)


if __name__ == "__main__":
    main()
