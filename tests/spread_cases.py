"""Planted batches for the spread tests: every read is flank + unit-set repeat + flank, so the grouping and the copy numbers are known.
Test infrastructure, shared by tests/test_gpu_spread.py and whoever wants to look at the shapes on the CPU (oracle_lib.assemble_batch gives
the same labels as the device)."""
import numpy as np
from otter_amd import abi, synth
from helpers import mutate, rand_seq

R64 = 64 * 4                                  # 64 SP_REG_STRIDES of otg_spread_core.hpp: the last region size of the register tier


def planted_batch(rng, specs, err=0.005):
    """specs: one per region, dict(units=[bytes], random=bool (random sequence between the flanks, of copies[0] bases), no_set=bool, alleles=[(copies per unit, n_reads, scatter)], partial=n one-sided
    reads, exact=bool (no errors: identical reads per copy number), tail=[extra copies of unit 0, one read each, on allele 0]) ->
    (batch, unit_sets, region_set, planted) with planted[r] = per read (allele, copies per unit) or None for a one-sided read"""
    chunks, reads, regions, planted = [], [], [], []
    unit_sets, region_set = [], []
    pos = 0

    def push(b, spl, spr):
        nonlocal pos
        chunks.append(np.frombuffer(b, dtype=np.uint8))
        reads.append((pos, len(b), spl, spr, 0, -1, -1, 0, len(b)))
        pos += len(b)

    for sp in specs:
        units = sp.get("units")
        fl, fr = rand_seq(rng, int(rng.integers(20, 41))), rand_seq(rng, int(rng.integers(20, 41)))
        first = len(reads)
        mine = []
        for a, (copies, n, scatter) in enumerate(sp["alleles"]):
            extra = sp.get("tail", []) if a == 0 else []
            junk = rand_seq(rng, int(copies[0])) if sp.get("random") else None      # no repeat at all: one sequence per allele
            for i in range(n + len(extra)):
                if junk is not None:
                    body, c = junk, None
                else:
                    c = [max(1, int(k) + (int(rng.integers(-scatter, scatter + 1)) if scatter else 0)) for k in copies]
                    if i >= n:
                        c[0] = int(copies[0]) + int(extra[i - n])
                    body = b"".join(u * k for u, k in zip(units, c))
                s = fl + body + fr
                push(s if sp.get("exact") else mutate(rng, s, err), 1, 1)
                mine.append((a, c))
        for i in range(sp.get("partial", 0)):
            copies = sp["alleles"][0][0]
            s = fl + b"".join(u * int(k) for u, k in zip(units, copies)) + fr
            cut = len(s) // 2
            push(mutate(rng, s[:cut], err), 1, 0) if i % 2 == 0 else push(mutate(rng, s[cut:], err), 0, 1)
            mine.append(None)
        regions.append((first, len(reads) - first, 0, 0, 0, 0))
        planted.append(mine)
        if sp.get("no_set"):
            region_set.append(None)
        else:
            region_set.append(len(unit_sets))
            unit_sets.append(list(units))
    if not unit_sets:
        unit_sets.append([b"CAG"])
    arena = np.concatenate(chunks + [np.zeros(64, dtype=np.uint8)])
    batch = {"arena": arena, "reads": np.array(reads, dtype=abi.read_dt), "regions": np.array(regions, dtype=abi.region_dt)}
    return batch, unit_sets, region_set, planted


EIGHT = [b"CAG", b"CCG", b"AAG", b"AT", b"GGC", b"TTTA", b"AC", b"GAA"]


def table_specs(max_cov):
    """the table of test 1: one region per shape"""
    return [
        dict(units=[b"CAG"], alleles=[((20,), 8, 2), ((45,), 8, 3)]),
        dict(units=[b"CAG", b"CCG"], alleles=[((20, 8), 7, 1), ((40, 12), 9, 2)]),
        dict(units=EIGHT, alleles=[((6, 5, 5, 7, 5, 4, 7, 5), 6, 0), ((12, 5, 9, 7, 5, 8, 7, 5), 6, 0)]),
        dict(units=[b"CAG"], no_set=True, alleles=[((25,), 6, 1)]),
        dict(units=[b"CAG"], random=True, alleles=[((120,), 6, 0)]),
        dict(units=[b"CAG"], alleles=[((5,), max_cov + 1, 0)], exact=True),
        dict(units=[b"CAG"], alleles=[((30,), 8, 0)], partial=4),
        dict(units=[b"CAG"], alleles=[((22,), 9, 0)], exact=True),
    ]


def depth_specs():
    """test 2: one homozygous region per member count, and a deep one"""
    one = [dict(units=[b"CAG"], alleles=[((20 + (i % 5),), m, 0)]) for i, m in enumerate([1, 3, 4, 5, 63, 64, 65, R64, R64 + 1, 300])]
    return one + [dict(units=[b"CAG"], alleles=[((20,), 6, 0), ((45,), 2, 0)])]        # (a region of two reads alone splits into two alleles)


def expansion_specs():
    """test 3: the consensus at the mode, a tail of longer reads"""
    return [dict(units=[b"CAG"], alleles=[((30,), 14, 0)], tail=[2, 3, 5, 8, 12, 17])]


def reads_table(batch, labels, reads_after=None):
    """the otg_spread_read rows the rule prescribes for given labels and (optionally) the descriptors after the run: what the device reports"""
    rd = batch["reads"] if reads_after is None else reads_after
    out = np.zeros(len(rd), dtype=abi.spread_read_dt)
    out["seq_off"] = rd["seq_off"]; out["seq_len"] = rd["seq_len"]; out["label"] = labels; out["task"] = abi.SPREAD_NONE
    return out
