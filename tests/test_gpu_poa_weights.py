"""GPU parity of the POA consensus kernels away from c = 0.4 n, t = 0.3.  otg_poa_graph carries the two adjust_weights arguments per graph and every
edge weight w of the heaviest-path sweep becomes w - max(c, t * w) in FP32 (`damp`, csrc/poa.hip).  Every other POA test sets them as rapid_consensus
does, and there t is a dead operand: t * w > c needs w > 1.33 n, an edge weight is at most n + 1, and the oracle's consensus of every graph of the
fixture sets below is the same under t = 0 (test_t_is_dead_at_the_defaults keeps that finding).  A kernel that ignored t, read it from another
graph's slot or swapped it with c would pass them all.

Every comparison is _check of test_gpu_poa.py: GPU == oracle byte for byte, and == the reference's own PPOA where oracle/_ref is built.  Every value
swept carries a liveness condition stated on the ORACLE's outputs only: its result differs from its result at the defaults in at least one graph of
the set.  Graphs of the oracle's result that differ from the defaults, measured when the tests were written (sets: poa_weights_cases.SETS):

    setting            small (of 120)   kb (of 8)   ldsmix (of 100)   crowded (of 4)   fuzz (of 40)
    c=0,t=0               87             8             12                4               32
    c=0,t=1              120             8            100                4               39
    c=n+2,t=0.3          120             8            100                4               40
    c=1e6,t=0.3          120             8            100                4               40
    c=-3,t=0              87             8             12                4               32
    c=0.15n,t=0.3         69             8              4                1               21
    c=0.15n,t=0.6         72             8              5                1               21
    c=0.2n,t=0.3          56             8              3                -               16
    c=0.8n,t=0.3          91             8              9                2               10
    c=default,t=0.9       14             6              -                -                -
    c=default,t=2        120             8            100                4               40
    c=1.5,t=0.45          52             8              3                1                5
    c=default,t=0          0             0              0                0                0
(a dash: the value moves nothing on that set and is not run there).  t at c = 0.15 n, graphs that differ between two values of t:

    comparison              small (of 120)   kb (of 8)
    t = 0.3 vs t = 0               4             2
    t = 0.6 vs t = 0.3            19             7
One batch with a (c, t) of its own per graph (small + 4 of kb + ldsmix, 224 graphs, default_rng(5)): 143 graphs change when every graph is given its
neighbour's pair (91 of the 120 small ones).  The tests print the counts they see."""
import os
import re
import subprocess
import sys
import pytest
from helpers import build_poa_batch, poa_specs_with_weights
from test_gpu_poa import _check
import poa_weights_cases as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the value-set pairs that move nothing (the dashes of the table)
NOT_RUN = {("ldsmix", "c=default,t=0.9"), ("crowded", "c=0.2n,t=0.3"), ("crowded", "c=default,t=0.9"), ("fuzz", "c=default,t=0.9")}
SWEEP = [(name, s) for name in W.SETS for s in W.SWEPT if (name, s) not in NOT_RUN]


@pytest.mark.parametrize("name,setting", SWEEP, ids=["%s-%s" % p for p in SWEEP])
def test_poa_weights(gpu, oracle, name, setting):
    moved = W.graphs_moved(oracle, name, setting)
    print("%s, %s: %d of %d graphs of the oracle's result differ from the defaults" % (name, setting, moved, len(W.oracle_run(oracle, name, setting))))
    assert moved >= 1, (name, setting)
    got = _check(gpu, oracle, W.specs(oracle, name, setting))
    assert tuple(got) == W.oracle_run(oracle, name, setting)


@pytest.mark.parametrize("name", sorted(W.SETS))
def test_poa_defaults_after_other_weights(gpu, oracle, name):
    """No state carried from batch to batch: behind a run with every damped weight negative, the defaults give the oracle's default result."""
    gpu.poa_consensus_batch(*build_poa_batch(W.specs(oracle, name, "c=n+2,t=0.3")))
    assert tuple(_check(gpu, oracle, W.specs(oracle, name))) == W.oracle_run(oracle, name, W.DEFAULT)


@pytest.mark.parametrize("name", sorted(W.SETS))
def test_t_is_dead_at_the_defaults(oracle, name):
    """A test of the fixtures, not of the kernel: with c = 0.4 n the oracle's consensus of every graph is the same under t = 0 as under t = 0.3,
    which is why the sweep above is needed.  Fails when the fixtures change so that the default-weight tests start to cover t."""
    assert W.graphs_moved(oracle, name, "c=default,t=0") == 0


@pytest.mark.parametrize("name", W.T_LIVE_SETS)
@pytest.mark.parametrize("setting,other", W.T_LIVE, ids=["%s-vs-%s" % p for p in W.T_LIVE])
def test_t_is_live(oracle, name, setting, other):
    """... and the sweep does cover it: at c = 0.15 n two values of t give different results (on the oracle), and both are run above."""
    moved = W.graphs_moved(oracle, name, setting, other)
    print("%s, %s vs %s: %d of %d graphs of the oracle's result differ" % (name, setting, other, moved, len(W.oracle_run(oracle, name, setting))))
    assert moved >= 1 and (name, setting) in SWEEP


def test_poa_weights_differ_per_graph(gpu, oracle):
    """One batch, c drawn from {0, 0.5, 1.5, 0.15 n, 0.4 n, 0.8 n, n + 2} and t from {0, 0.3, 0.45, 0.6, 1} per graph: both launch lists and the redo
    of the graphs that outgrow their LDS block, in an order that is not the batch's.  What makes a mix-up of graph slots visible, on the oracle:
    with its neighbour's (c, t) (index i ^ 1) at least a quarter of the graphs change; and the batch equals its graphs run one at a time."""
    specs = W.mixed_specs(oracle)
    exp = oracle.poa_consensus_batch(*build_poa_batch(specs))
    swapped = oracle.poa_consensus_batch(*build_poa_batch(W.neighbours_weights(specs)))
    moved = sum(1 for x, y in zip(exp, swapped) if x != y)
    print("a (c, t) per graph: %d of %d graphs of the oracle's result change under the neighbour's pair" % (moved, len(specs)))
    assert 4 * moved >= len(specs)
    assert exp == [oracle.poa_consensus_batch(*build_poa_batch([s]))[0] for s in specs]
    assert _check(gpu, oracle, specs) == exp


@pytest.mark.parametrize("setting", [W.DEFAULT, "c=0,t=1", "c=n+2,t=0.3"])
def test_poa_degenerate_graphs(gpu, oracle, setting):
    """No member at all on a backbone of 1, 2, 4, 64, 65 bases and `ACGT`; a one-base backbone with one 'M' member and with two 'X' members; a
    two-base backbone whose only member is insertions and deletions.  Parity with the reference (`ACGT` alone gives `AC`, a one-base backbone
    alone nothing), not a claim about what is right; one graph per call as well, so that none leans on its neighbours in the batch."""
    specs = poa_specs_with_weights(W.degenerate_specs(), W.SETTINGS[setting])
    got = _check(gpu, oracle, specs)
    assert got == [_check(gpu, oracle, [s])[0] for s in specs]
    if setting == W.DEFAULT:
        assert got[5] == b"AC" and got[0] == b"" and got[6] == b""


def test_fixtures_reach_both_kernels_and_the_redo(gpu):
    """A test of the fixtures: under the default launch plan the small, ldsmix and fuzz sets and the batch with a (c, t) per graph fill BOTH launch
    lists, and the LDS kernel gives up some of its graphs half-way (they outgrow the optimistic capacities of its block), which the global-memory
    kernel then redoes from G.  The plan sizes the LDS block for the graph of rank 97 % and uses no LDS at all when that graph needs more than
    16 KB: a set with more than 3 % of large graphs runs on the global-memory kernel alone, whatever its docstring says.  Read from the
    OTG_POA_PROFILE line of each batch in a child process (the switch is read once per process); the switches of test_gpu_alt_paths.py that take
    the LDS kernel away are not passed on.  Seen when written, LDS list + global list (finished in LDS): small 117 + 3 (110), ldsmix 97 + 3 (92),
    fuzz 38 + 2 (31), per graph 217 + 7 (212)."""
    gpu.trim()
    labels = ["small", "ldsmix", "fuzz", "mixed"]
    env = {k: v for k, v in os.environ.items() if k not in ("OTG_POA_NO_LDS", "OTG_POA_V1", "OTG_POA_PIECE_MB", "OTG_POA_HOST_PLAN")}
    env["OTG_POA_PROFILE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "poa_census_child.py")] + labels, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    seen = re.findall(r"== (\w+)\n(?:(?!== ).*\n)*?\[otg\] poa profile: (\d+) LDS \+ (\d+) global launches; (\d+) graphs done \((\d+) in LDS", r.stderr)
    assert [x[0] for x in seen] == labels, r.stderr[-2000:]
    for label, n_lds, n_glob, done, in_lds in seen:
        n_lds, n_glob, done, in_lds = int(n_lds), int(n_glob), int(done), int(in_lds)
        print("%s: %d graphs on the LDS list, %d on the global-memory list; %d finished in LDS, %d redone" % (label, n_lds, n_glob, in_lds, n_lds - in_lds))
        assert done == n_lds + n_glob and n_glob >= 1 and 1 <= in_lds < n_lds, (label, n_lds, n_glob, done, in_lds)
