"""The adjust_weights arguments (c, t) of the POA consensus away from rapid_consensus' c = 0.4 n, t = 0.3: the settings, the fixture sets and the
oracle's runs of them, shared by test_gpu_poa_weights.py and test_poa_weights_golden.py.  Every edge weight w becomes w - max(c, t * w) in FP32.
Not a test module."""
import numpy as np
from helpers import build_poa_batch, poa_specs_with_weights, random_poa_specs

DEFAULT = "default"
# id -> weights(n, c, t) of helpers.poa_specs_with_weights: n = the member count (an edge weight is at most n + 1), (c, t) = rapid_consensus' own
SETTINGS = {
    DEFAULT: lambda n, c, t: (c, t),
    "c=0,t=0": lambda n, c, t: (0.0, 0.0),                      # raw integer weights
    "c=0,t=1": lambda n, c, t: (0.0, 1.0),                      # every damped weight 0: the three tie-breaks decide every node
    "c=n+2,t=0.3": lambda n, c, t: (n + 2.0, 0.3),              # every damped weight negative: below the 0.0f a node weight starts with
    "c=1e6,t=0.3": lambda n, c, t: (1.0e6, 0.3),                # ... and FP32 sums that lose the integer part of the small weights
    "c=-3,t=0": lambda n, c, t: (-3.0, 0.0),
    "c=0.15n,t=0.3": lambda n, c, t: (0.15 * n, 0.3),           # both branches of the max in one graph: t * w on the covered edges, c on the thin ones
    "c=0.15n,t=0.6": lambda n, c, t: (0.15 * n, 0.6),
    "c=0.2n,t=0.3": lambda n, c, t: (0.2 * n, 0.3),
    "c=0.8n,t=0.3": lambda n, c, t: (0.8 * n, 0.3),
    "c=default,t=0.9": lambda n, c, t: (c, 0.9),
    "c=default,t=2": lambda n, c, t: (c, 2.0),
    "c=1.5,t=0.45": lambda n, c, t: (1.5, 0.45),
    # not swept on the GPU: the other side of a liveness statement
    "c=default,t=0": lambda n, c, t: (c, 0.0),
    "c=0.15n,t=0": lambda n, c, t: (0.15 * n, 0.0),
}
SWEPT = [s for s in SETTINGS if s not in (DEFAULT, "c=default,t=0", "c=0.15n,t=0")]
# t is live: (setting, the same c under another t); the oracle's results differ on at least one graph of the set
T_LIVE = [("c=0.15n,t=0.3", "c=0.15n,t=0"), ("c=0.15n,t=0.6", "c=0.15n,t=0.3")]
T_LIVE_SETS = ("small", "kb")


def _small(oracle):
    return random_poa_specs(np.random.default_rng(41), oracle, 120, 1, 160, err=0.1)


def _kb(oracle):
    return random_poa_specs(np.random.default_rng(42), oracle, 8, 800, 2000, err=0.07)


def _ldsmix(oracle):
    from test_gpu_poa import lds_capacity_mix_specs
    return lds_capacity_mix_specs(np.random.default_rng(45), 100, every=10, kinds=(2, 1, 2, 2, 3, 2, 2, 1, 2, 2), noisy_members=(6, 14))


def _crowded(oracle):
    from test_gpu_poa import crowded_anchor_specs
    return crowded_anchor_specs(np.random.default_rng(46), 4)


def _fuzz(oracle):
    from test_gpu_poa import op_string_fuzz_specs
    return op_string_fuzz_specs(np.random.default_rng(44), 40)


# small: LDS graphs.  kb: the global-memory instantiation, second-generation sweep, backbones longer than its 128-node window.  ldsmix: the
# generator of test_poa_lds_capacity_mix with 90 graphs in the crowd, 7 noisy ones of 6-13 members, 2 of 40 members and one long backbone: the
# launch plan sizes the LDS block for the graph of rank 97 %, so with 3 large graphs of 100 that is the largest of the seven, which all start in
# LDS; those that outgrow the block are redone by the global-memory kernel, which reads G.c / G.t again.  crowded: the first 4 graphs of
# test_poa_crowded_anchors_and_long_jumps (anchors with more than 64 subtree edges, landings beyond the window).  fuzz: the first 40 of
# test_poa_op_string_fuzz (op strings past the backbone: no tree property, the Kahn sweep).
SETS = {"small": _small, "kb": _kb, "ldsmix": _ldsmix, "crowded": _crowded, "fuzz": _fuzz}

_specs, _runs = {}, {}


def specs(oracle, name, setting=DEFAULT):
    if name not in _specs:
        _specs[name] = SETS[name](oracle)
    return poa_specs_with_weights(_specs[name], SETTINGS[setting])


def oracle_run(oracle, name, setting):
    """The oracle's consensus of every graph of set `name` under `setting`: computed once per process, never modified."""
    if (name, setting) not in _runs:
        _runs[(name, setting)] = tuple(oracle.poa_consensus_batch(*build_poa_batch(specs(oracle, name, setting))))
    return _runs[(name, setting)]


def graphs_moved(oracle, name, setting, other=DEFAULT):
    """Liveness: how many graphs of the ORACLE's result under `setting` differ from the ORACLE's result under `other`."""
    return sum(1 for x, y in zip(oracle_run(oracle, name, setting), oracle_run(oracle, name, other)) if x != y)


# ---- one batch with a different (c, t) per graph
MIXED_C = [lambda n: 0.0, lambda n: 0.5, lambda n: 1.5, lambda n: 0.15 * n, lambda n: 0.4 * n, lambda n: 0.8 * n, lambda n: n + 2.0]
MIXED_T = [0.0, 0.3, 0.45, 0.6, 1.0]


def mixed_specs(oracle, seed=5):
    """small + the first 4 of kb + ldsmix: no more than 3 % of a batch may be large for its launch plan to use the LDS kernel at all."""
    rng = np.random.default_rng(seed)
    return poa_specs_with_weights(specs(oracle, "small") + specs(oracle, "kb")[:4] + specs(oracle, "ldsmix"),
                                  lambda n, c, t: (MIXED_C[int(rng.integers(0, len(MIXED_C)))](n), MIXED_T[int(rng.integers(0, len(MIXED_T)))]))


def neighbours_weights(sp):
    """Every graph with the (c, t) of the graph at index i ^ 1 (the last of an odd count keeps its own)."""
    return [(bb, mem) + tuple(sp[i ^ 1][2:] if (i ^ 1) < len(sp) else sp[i][2:]) for i, (bb, mem, c, t) in enumerate(sp)]


# ---- degenerate graphs
def degenerate_specs():
    from helpers import rand_seq
    rng = np.random.default_rng(47)
    out = [(rand_seq(rng, B), [], np.float32(1.0), np.float32(0.3)) for B in (1, 2, 4, 64, 65)]      # no member at all
    out.append((b"ACGT", [], np.float32(1.0), np.float32(0.3)))
    out.append((b"A", [(b"A", b"M", True, True)], np.float32(1.0), np.float32(0.3)))
    out.append((b"A", [(b"C", b"X", True, True), (b"G", b"X", True, True)], np.float32(1.0), np.float32(0.3)))
    out.append((b"AC", [(b"GTT", b"IIIDD", True, True)], np.float32(1.0), np.float32(0.3)))
    return out
