"""Child process of tests/test_gpu_edit_align_adaptive.py: one adaptive edit_align_heur_batch in a fresh process, for the switches the
library reads once per process (OTG_EDIT_ALIGN_ADAPTIVE_TIERS, OTG_EDIT_ALIGN_BUDGET_MB; set by the parent in this process's
environment).  argv: <input set> <min_wavefront_length> <max_distance_threshold> <steps>.  Prints one JSON line: scores, cells, op
strings and the tasks each tier finished."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import otter_amd                                    # noqa: E402
from otter_amd import abi                           # noqa: E402
import adaptive_align_fixtures as fx                # noqa: E402
from helpers import pair_tasks                      # noqa: E402


def main():
    name, params = sys.argv[1], tuple(int(x) for x in sys.argv[2:5])
    arena, tasks = pair_tasks(fx.input_set(name))
    with otter_amd.Context(0) as ctx:
        scores, cigs, cells = ctx.edit_align_heur_batch(arena, tasks, abi.OTG_HEURISTIC_WFADAPTIVE, *params, want_cells=True)
        tiers = ctx.edit_align_last_tiers()
    print(json.dumps({"scores": scores.tolist(), "cells": cells.tolist(), "cigs": [c.decode() for c in cigs], "tiers": list(tiers)}))


if __name__ == "__main__":
    main()
