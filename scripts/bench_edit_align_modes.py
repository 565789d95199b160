"""GPU box: otg_edit_align_last_ms (score chain ms, provenance pass ms; HIP events) on the MID and LONG pairs of
tests/adaptive_align_fixtures.py and on the pairs of the adaptive compare fixture (tests/test_gpu_compare_adaptive.py), in exact mode and,
where the package has it, under wfadaptive(10,50,1) (DESIGN_LOG, "Adaptive-mode edit traceback").
  bench_edit_align_modes.py [ROOT] [LABEL]    ROOT: the tree whose otter_amd package and build to load (default: this one; e.g. the parent
                                              commit's, to compare the exact mode's times), LABEL: copied into the output
Two warm-up calls per set and mode, then REPS timed ones, the modes alternating; prints one JSON line (median, min, max per pass)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, PKG)
import numpy as np                                  # noqa: E402
import otter_amd                                    # noqa: E402
assert os.path.dirname(os.path.dirname(os.path.abspath(otter_amd.__file__))) == PKG, otter_amd.__file__
from otter_amd import abi                           # noqa: E402
import adaptive_align_fixtures as fx                # noqa: E402
from compare_fixtures import pair_plan              # noqa: E402
from helpers import pair_tasks                      # noqa: E402

REPS = 9


def compare_pairs():
    mid = fx.input_set("MID")
    differ = [9, 16, 17, 19, 21, 36, 38]
    order = differ + [i for i in range(len(mid)) if i not in differ]
    out = []
    for r in range(12):
        x, y = order[2 * r], order[2 * r + 1]
        for t, q in pair_plan([mid[x][0], mid[y][0]], [mid[x][1], mid[y][1]]):
            out.append(fx.oriented(t, q))
    return out


def main():
    sets = {"MID": fx.input_set("MID"), "LONG": fx.input_set("LONG"), "COMPARE": compare_pairs()}
    res = {"label": sys.argv[2] if len(sys.argv) > 2 else "", "reps": REPS}
    with otter_amd.Context(0) as ctx:
        has_heur = hasattr(ctx, "edit_align_heur_batch")
        for name, prs in sets.items():
            arena, tasks = pair_tasks(prs)
            modes = {"exact": lambda: ctx.edit_align_batch(arena, tasks, want_cigars=False)}
            if has_heur:
                modes["adaptive"] = lambda: ctx.edit_align_heur_batch(arena, tasks, abi.OTG_HEURISTIC_WFADAPTIVE, 10, 50, 1, want_cigars=False)
            t = {m: [] for m in modes}
            for rep in range(2 + REPS):
                for m, f in modes.items():
                    f()
                    if rep >= 2:
                        t[m].append(ctx.edit_align_last_ms())
            for m in modes:
                a = np.asarray(t[m])
                res["%s_%s" % (name, m)] = {"n_pairs": len(prs), "score_ms_median": round(float(np.median(a[:, 0])), 4), "score_ms_min": round(float(a[:, 0].min()), 4),
                                            "score_ms_max": round(float(a[:, 0].max()), 4), "prov_ms_median": round(float(np.median(a[:, 1])), 4),
                                            "prov_ms_min": round(float(a[:, 1].min()), 4), "prov_ms_max": round(float(a[:, 1].max()), 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
