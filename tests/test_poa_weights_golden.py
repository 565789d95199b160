"""CPU: pins the oracle's POA consensus under adjust_weights arguments away from c = 0.4 n, t = 0.3 (the sweep of test_gpu_poa_weights.py) to the
reference: against its recorded outputs (tests/golden/poa_weights.json, scripts/make_golden_poa_weights.py) always, and against its own PPOA where
oracle/_ref is built.  The graphs are a part of what the GPU sweep runs, trimmed to keep the fixture small: every 8th graph of its small set from
the 4th on (15 graphs; of the strides of 8 the one on which every liveness statement below still holds: it has graph 59, one of the four small
graphs that t = 0.3 against t = 0 moves at c = 0.15 n) and graphs 0 and 7 of its kilobase set (900 and 1190 bases, 7 members each).  In the file
a member is its run-length coded op string (`120M1X3I`) and the bases of its X and I ops (an M is the backbone's base), and a graph's distinct
consensus strings are listed once, with one index per setting."""
import json
import os
import re
import numpy as np
import pytest
from helpers import build_poa_batch, poa_specs_with_weights
import poa_weights_cases as W

GOLD = os.path.join(os.path.dirname(__file__), "golden", "poa_weights.json")
_cache = {}


def golden_specs(oracle):
    if "specs" not in _cache:
        _cache["specs"] = W.specs(oracle, "small")[3::8] + [W.specs(oracle, "kb")[i] for i in (0, 7)]
    return _cache["specs"]


def run_length(ops):
    return "".join("%d%s" % (len(m.group(0)), m.group(1)) for m in re.finditer(r"(.)\1*", ops.decode()))


def _ops(coded):
    return "".join(op * int(n) for n, op in re.findall(r"(\d+)(.)", coded)).encode()


def pack_member(bb, seq, ops):
    """(run-length op string, the bases of its X and I ops): an 'M' of the aligner's op strings is the backbone's own base."""
    own, r, q = bytearray(), 0, 0
    for op in ops:
        if op == ord("M"):
            assert seq[q] == bb[r]
        elif op != ord("D"):
            own.append(seq[q])
        r += op != ord("I")
        q += op != ord("D")
    assert r == len(bb) and q == len(seq)
    return run_length(ops), own.decode()


def _member(bb, coded, own):
    ops, seq, r, k = _ops(coded), bytearray(), 0, 0
    for op in ops:
        if op == ord("M"):
            seq.append(bb[r])
        elif op != ord("D"):
            seq.append(ord(own[k])); k += 1
        r += op != ord("I")
    return bytes(seq), ops


def _gold():
    if "gold" not in _cache:
        _cache["gold"] = json.load(open(GOLD))
    return _cache["gold"]


def _recorded_specs(setting):
    k = _gold()["settings"].index(setting)
    return [(g["backbone"].encode(), [_member(g["backbone"].encode(), cg, own) + (l, r) for cg, own, l, r in g["members"]], np.float32(g["c"][k]), np.float32(g["t"][k]))
            for g in _gold()["graphs"]]


def _recorded_results(setting):
    k = _gold()["settings"].index(setting)
    return [g["consensus"][g["expected"][k]].encode() for g in _gold()["graphs"]]


def test_recorded_inputs_are_the_generated_ones(oracle):
    """The fixture holds the graphs the GPU sweep runs (op strings from the oracle's aligner included) and every setting of the sweep, with
    the float32 (c, t) that helpers.poa_specs_with_weights gives."""
    gold = _gold()
    assert gold["settings"] == list(W.SETTINGS) and len(gold["graphs"]) == 17
    for setting in W.SETTINGS:
        assert _recorded_specs(setting) == poa_specs_with_weights(golden_specs(oracle), W.SETTINGS[setting]), setting


@pytest.mark.parametrize("setting", list(W.SETTINGS))
def test_oracle_matches_recorded_reference(oracle, setting):
    specs = _recorded_specs(setting)
    exp = _recorded_results(setting)
    assert oracle.poa_consensus_batch(*build_poa_batch(specs)) == exp
    if oracle.ref() is not None:
        assert oracle.poa_consensus_batch(*build_poa_batch(specs), which="ref") == exp


def test_recorded_results_tell_the_settings_apart():
    """On the recorded outputs alone: t = 0 changes nothing at the default c (the dead operand of the default-weight tests), every swept setting
    changes some graph, and at c = 0.15 n both steps of t do."""
    def moved(a, b=W.DEFAULT):
        return sum(1 for x, y in zip(_recorded_results(a), _recorded_results(b)) if x != y)
    assert moved("c=default,t=0") == 0
    for setting in W.SWEPT:
        assert moved(setting) >= 1, setting
    for a, b in W.T_LIVE:
        assert moved(a, b) >= 1, (a, b)
