"""The consensus stage of the pipeline plans its launches on the device (poa.hip: capacities from the op strings, their running sums, the LDS
size from a histogram, the two launch lists by a stable radix sort); OTG_POA_HOST_PLAN=1 forces the host planner, which also takes a batch
whose graph images exceed the piece budget.  Every batch below runs in this process with the device plan and in a fresh child process with
the host planner (the switches are read once per process): region results, allele records, sequence bytes and labels must be equal between
the two, and equal the CPU oracle's.

The mixed batch (60-read loci of 100-300 bases next to one 3 kb locus) must fill both launch lists; the child runs under OTG_POA_PROFILE, whose
first line reports the two list lengths of the host planner, and the test asserts both are non-zero.  By the estimate formula
18 (B + alt / 2 + 5) + 8 ((alt + mrun) / 2 + 5) + ~200 a 300-base graph of 30 clean members needs about 7 KB and a 3 kb graph more than 57 KB,
so the percentile (rank 0.97 (n - 1) of more than 40 graphs) falls on a small graph and the 3 kb graphs lie beyond it.

This file is also the child's program: `python tests/test_gpu_poa_device_plan.py OUT.npz NAME...` runs the named batches and saves the results."""
import os
import re
import subprocess
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
from otter_amd import abi, synth  # noqa: E402

OP_LENGTHS = (63, 64, 65, 128, 129)


def _hand_batch(regions_of_reads):
    """A batch from explicit reads: regions_of_reads = [[bytes, ...], ...], every read spanning, untagged."""
    chunks, reads, regions, pos = [], [], [], 0
    for seqs in regions_of_reads:
        first = len(reads)
        for s in seqs:
            chunks.append(np.frombuffer(s, dtype=np.uint8))
            reads.append((pos, len(s), 1, 1, 0, -1, -1, 0, len(s)))
            pos += len(s)
        regions.append((first, len(seqs), 0, 0, 0, 0))
    return {"arena": np.concatenate(chunks + [np.zeros(64, dtype=np.uint8)]), "reads": np.array(reads, dtype=abi.read_dt),
            "regions": np.array(regions, dtype=abi.region_dt), "truth": np.zeros((len(regions), 3), dtype=np.int64)}


def _op_string_reads(n_ops):
    """Backbone A of n_ops - 1 bases and a read that has one base more in front, a substitution at base 40 and another at the last base: its op
    string against A is I M..M X M..M X, n_ops long; the second 'M' run crosses the 64-op boundary when n_ops >= 128 and ends on it when n_ops = 65."""
    rng = np.random.default_rng(1000 + n_ops)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    a = rng.integers(0, 4, n_ops - 1)
    b = a.copy()
    b[40] = (b[40] + 1) & 3
    b[-1] = (b[-1] + 2) & 3
    lead = (a[0] + 1 + (a[1] == ((a[0] + 1) & 3))) & 3          # differs from the two bases that follow it
    return acgt[a].tobytes(), acgt[np.concatenate([[lead], b])].tobytes()


def _stale_member_batch():
    """test_gpu_pipeline.test_stale_cigar_member's case: a labelled member that is longer than the representative and spans neither side is
    not aligned; as its allele's first member its op string is empty."""
    b = synth.make_batch(6, len_range=(300, 500), n_reads=12, err="hifi", seed=77, frac_partial=0.0)
    reads = b["reads"].copy()
    for r in range(len(b["regions"])):
        i = int(b["regions"][r]["first_read"]) + (0 if r % 2 == 0 else 5)
        reads["seq_len"][i] += 12
        reads["spanning_l"][i] = 0
        reads["spanning_r"][i] = 0
    return dict(b, reads=reads)


def _mixed_batch():
    small = synth.make_batch(40, len_range=(100, 300), n_reads=60, err="hifi", seed=501, frac_partial=0.05)
    big = synth.make_batch(1, len_range=(3000, 3000), n_reads=30, err="ont", seed=502, frac_partial=0.0)
    return synth.concat_batches([small, big, synth.make_batch(2, len_range=(100, 300), n_reads=60, err="hifi", seed=503)])


def _single_reads(n, seed):
    return synth.make_batch(n, len_range=(120, 200), n_reads=1, err="hifi", seed=seed, frac_partial=0.0)


def _skipped(seed):
    b = synth.make_batch(1, len_range=(120, 200), n_reads=5, err="hifi", seed=seed, frac_partial=0.0)
    reads = b["reads"].copy()
    reads["spanning_r"][:] = 0
    return dict(b, reads=reads)


# name -> (batch builder, parameters)
BATCHES = {
    # 2 reads (the allele is a copy, no graph) and 3 reads (the smallest graph: two members), one allele per region
    "two_and_three_reads": (lambda: synth.concat_batches([synth.make_batch(4, len_range=(150, 300), n_reads=2, err="hifi", seed=510, frac_partial=0.0),
                                                          synth.make_batch(4, len_range=(150, 300), n_reads=3, err="hifi", seed=511, frac_partial=0.0)]), {"max_alleles": 1}),
    # single-read clusters (allele copied, graph slot empty), a skipped region (no spanning read): no graph is live in the batch
    "no_live_graph": (lambda: synth.concat_batches([_single_reads(3, 520), _skipped(521), _single_reads(2, 522)]), {}),
    # exactly one live graph: one 5-read region under max_alleles = 1 between single-read and skipped regions
    "one_live_graph": (lambda: synth.concat_batches([_single_reads(2, 530), synth.make_batch(1, len_range=(200, 200), n_reads=5, err="hifi", seed=531, frac_partial=0.0),
                                                     _skipped(532), _single_reads(1, 533)]), {"max_alleles": 1}),
    "empty_op_string": (_stale_member_batch, {}),
    # [A, planted read, A] under max_alleles = 1: one allele, the medoid of an all-ones matrix is its first read, A
    "op_string_lengths": (lambda: _hand_batch([[a, b, a] for a, b in map(_op_string_reads, OP_LENGTHS)]), {"max_alleles": 1}),
    "mixed_sizes": (_mixed_batch, {}),
    "two_thousand_slots": (lambda: synth.make_batch(70, len_range=(200, 200), n_reads=30, err="hifi", seed=540), {}),
    # more slots than one scan tile (8 192) and than one sort chunk (4 096): three waves sort, the scans carry a prefix
    "eight_thousand_slots": (lambda: synth.make_batch(420, len_range=(100, 100), n_reads=20, err="hifi", seed=541, frac_partial=0.0), {}),
}


def _run_batches(ctx, names, mark=None):
    out = {}
    for name in names:
        make, kw = BATCHES[name]
        if mark:
            mark(name)
        res = ctx.assemble(abi.default_params(**kw), make())
        n = int(res["alleles"]["seq_len"].astype(np.int64).sum())
        out[name] = {"regions": res["regions"], "alleles": res["alleles"], "labels": res["labels"], "seqs": res["seqs"][:n]}
    return out


if __name__ == "__main__":
    import otter_amd

    def _mark(name):
        sys.stderr.write("## batch %s\n" % name)
        sys.stderr.flush()
    with otter_amd.Context(0) as _ctx:
        _got = _run_batches(_ctx, sys.argv[2:], _mark)
    np.savez(sys.argv[1], **{"%s.%s" % (n, k): v for n, r in _got.items() for k, v in r.items()})
    sys.exit(0)

import pytest  # noqa: E402

pytestmark = pytest.mark.gpu


def _child(tmp_path, tag, switches, names):
    """The named batches in a fresh process under the switches: (results, stderr)."""
    env = dict(os.environ)
    for kv in switches.split():
        k, _, v = kv.partition("=")
        env[k] = v or "1"
    out = str(tmp_path / (tag + ".npz"))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out] + list(names), cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (switches, r.stdout[-2000:], r.stderr[-2000:])
    z = np.load(out)
    return {n: {k: z["%s.%s" % (n, k)] for k in ("regions", "alleles", "labels", "seqs")} for n in names}, r.stderr


def _same(a, b, what):
    for k in ("regions", "alleles", "labels", "seqs"):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.fixture(scope="module")
def host_plan(gpu, tmp_path_factory):
    """Every batch under the host planner, once for the module (one child process), with the planner's profile lines."""
    gpu.trim()
    return _child(tmp_path_factory.mktemp("host_plan"), "host", "OTG_POA_HOST_PLAN OTG_POA_PROFILE", list(BATCHES))


@pytest.mark.parametrize("name", list(BATCHES))
def test_device_plan_equals_host_plan_and_oracle(gpu, oracle, host_plan, name):
    from test_gpu_pipeline import compare
    make, kw = BATCHES[name]
    batch = make()
    got = _run_batches(gpu, [name])[name]
    _same(got, host_plan[0][name], name)
    ora = oracle.assemble_batch(abi.default_params(**kw), batch)
    compare(got, ora, batch)
    al, rg = got["alleles"], got["regions"]
    if name == "no_live_graph":
        assert len(al) == 5 and (al["acov"] <= 2).all() and (rg["status"] != 0).sum() == 1
    if name == "one_live_graph":
        assert (al["acov"] > 2).sum() == 1 and (rg["status"] != 0).sum() == 1
    if name == "two_and_three_reads":
        assert (al["acov"] == 3).sum() == 4 and (al["acov"] == 2).sum() == 4
    if name == "op_string_lengths":
        assert len(al) == len(OP_LENGTHS) and (al["acov"] == 3).all()
    if name == "mixed_sizes":
        assert (al["seq_len"] > 2500).any() and (al["acov"] > 2).sum() > 40
    if name in ("two_thousand_slots", "eight_thousand_slots"):
        assert len(batch["reads"]) in (2100, 8400)


def test_op_string_lengths_are_as_planted(gpu):
    """The planted reads' op strings against their backbones, from the gap-affine aligner the pipeline uses: 63 / 64 / 65 / 128 / 129 ops, 'I' first,
    'X' last, two 'M' runs."""
    from helpers import pair_tasks
    pairs = [_op_string_reads(n) for n in OP_LENGTHS]
    arena, tasks = pair_tasks(pairs)
    _, cigs = gpu.affine_align_batch(arena, tasks)
    for n, c in zip(OP_LENGTHS, cigs):
        c = bytes(c)
        assert len(c) == n and c[:1] == b"I" and c[-1:] == b"X" and c.count(b"X") == 2 and c.count(b"I") == 1 and b"D" not in c, (n, c)
        assert c[41:42] == b"X" and set(c[1:41]) == {ord("M")} and set(c[42:-1]) == {ord("M")}


def test_both_launch_lists_are_filled(host_plan):
    """The mixed batch puts graphs on the LDS list and on the global-memory list (the host planner's counts, which the device plan reproduces)."""
    err = host_plan[1]
    part = err.split("## batch mixed_sizes\n", 1)[1].split("## batch ", 1)[0]
    m = re.search(r"poa profile: (\d+) LDS \+ (\d+) global launches", part)
    assert m, part[:500]
    assert int(m.group(1)) >= 1 and int(m.group(2)) >= 1, m.group(0)


@pytest.mark.parametrize("switches", ["OTG_POA_NO_LDS", "OTG_POA_PIECE_MB=1"], ids=["no_lds", "piece_budget_fallback"])
def test_device_plan_under_switches(gpu, host_plan, tmp_path, switches):
    """The mixed batch in a child without the LDS kernel (device plan, one launch list), and under a 1 MB piece budget, which the images of
    a launch list exceed: the stage must hand the batch to the host planner.  Same bytes as the host planner's run."""
    gpu.trim()
    got, _ = _child(tmp_path, "switch", switches, ["mixed_sizes"])
    _same(got["mixed_sizes"], host_plan[0]["mixed_sizes"], switches)


def test_operator_level_call_keeps_the_host_planner(gpu, oracle):
    """otg_poa_consensus_batch plans on the host as before: the fixtures of test_gpu_poa.py, unchanged results."""
    from helpers import random_poa_specs
    from test_gpu_poa import _check
    _check(gpu, oracle, random_poa_specs(np.random.default_rng(41), oracle, 60, 1, 120, err=0.1))
    _check(gpu, oracle, random_poa_specs(np.random.default_rng(42), oracle, 6, 800, 2500, err=0.07))
