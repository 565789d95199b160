"""Child of tests/test_exp_host.py, started with GLIBC_TUNABLES=glibc.cpu.hwcaps=-FMA,-FMA4 so that libm resolves exp() to its non-FMA
build.  Prints one JSON line: whether the tunable took effect (libm now disagrees with the FMA restatement somewhere on the set) and on how
many arguments the non-FMA restatement differs from libm."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["OTG_NO_TORCH_PRELOAD"] = "1"      # host code only: no need for torch's HIP runtime

import otter_amd  # noqa: E402
from exp_args import ARGS, libm_exp, mismatches  # noqa: E402

ref = libm_exp(ARGS)
fma = mismatches(otter_amd.exp_host(ARGS, 1), ref)
nofma = mismatches(otter_amd.exp_host(ARGS, 0), ref)
print(json.dumps({"n": int(ARGS.size), "fma_mismatches": int(fma.size), "nofma_mismatches": int(nofma.size),
                  "first_nofma": [float(v).hex() for v in ARGS[nofma[:5]]], "probe": otter_amd.exp_probe()}))
