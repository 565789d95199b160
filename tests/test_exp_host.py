"""CPU: the host restatement of glibc's exp() (otg_exp_host; the device function is compared with it in test_gpu_exp.py) against libm itself
on the argument set of exp_args.py, bit for bit, in both builds of libm; and the probe otg_create chooses the variant with."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest
import otter_amd
from exp_args import ARGS, PARTS, libm_exp, mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libm_values():
    v = libm_exp(ARGS)
    v.setflags(write=False)
    return v


def test_argument_set():
    assert 1.9e6 <= ARGS.size <= 2.2e6 and PARTS["kde"] >= 1000000 and PARTS["positive"] == 100000 and PARTS["steps"] == 6 * 138240
    assert ARGS[PARTS["specials"] + PARTS["thresholds"]:][:PARTS["steps"]].min() < -748 + 0.01
    assert (ARGS[-PARTS["positive"] - PARTS["kde"]:-PARTS["positive"]] <= 0).all()


def test_selected_variant_equals_libm(libm_values):
    """The restatement of the variant the probe selects on this host == libm exp() on the whole set.  Before the fused `InvLn2N*x + Shift`
    of the FMA variant and the fused large-positive branch this differed on the half-way points and in [512, 709.78)."""
    probe = otter_amd.exp_probe()
    got = otter_amd.exp_host(ARGS, probe["variant"])
    bad = mismatches(got, libm_values)
    print("variant %d: %d of %d arguments differ from libm" % (probe["variant"], bad.size, ARGS.size))
    assert bad.size == 0, [(float(ARGS[i]).hex(), float(got[i]).hex(), float(libm_values[i]).hex()) for i in bad[:5]]


def test_nofma_variant_equals_nofma_libm():
    """The non-FMA restatement == libm exp() with the FMA builds of libm switched off (a fresh child under GLIBC_TUNABLES).  The child first
    shows that the switch took effect: libm then disagrees with the FMA restatement somewhere on the set."""
    env = dict(os.environ, GLIBC_TUNABLES="glibc.cpu.hwcaps=-FMA,-FMA4")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "exp_nofma_child.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    if out["fma_mismatches"] == 0:
        pytest.skip("GLIBC_TUNABLES=glibc.cpu.hwcaps=-FMA,-FMA4 did not move libm off its FMA build of exp() on this host")
    assert out["nofma_mismatches"] == 0, out
    assert out["probe"]["variant"] == 0 and out["probe"]["mismatches_nofma"] == 0 and out["probe"]["mismatches_fma"] > 0


def test_variants_differ_where_expected():
    """The two restatements are different functions (about 5 in 10^4 arguments), and agree on the specials."""
    a, b = otter_amd.exp_host(ARGS, 1), otter_amd.exp_host(ARGS, 0)
    d = mismatches(a, b)
    assert 1000 < d.size < 10000
    assert mismatches(a[:PARTS["specials"]], b[:PARTS["specials"]]).size == 0
    one = np.array([0.0, -0.0, -np.inf, np.inf])
    assert otter_amd.exp_host(one, 1).tolist() == [1.0, 1.0, 0.0, np.inf]


def test_probe_is_decisive():
    """otg_create's probe: its set holds arguments on which the two variants differ (tens of them), and the variant it chooses has no
    mismatch against this host's libm."""
    p = otter_amd.exp_probe()
    print(p)
    assert p["n_args"] >= 100000 and p["n_differ"] >= 20
    chosen = p["mismatches_fma"] if p["variant"] else p["mismatches_nofma"]
    other = p["mismatches_nofma"] if p["variant"] else p["mismatches_fma"]
    assert chosen == 0
    assert other >= 20


def test_exp_host_arguments():
    lib = otter_amd.load()
    x = np.zeros(2)
    assert lib.otg_exp_host(otter_amd.abi.ptr(x), 2, 2, otter_amd.abi.ptr(x)) == otter_amd.abi.OTG_ERR_ARG
    assert lib.otg_exp_host(None, 2, 1, otter_amd.abi.ptr(x)) == otter_amd.abi.OTG_ERR_ARG
    assert lib.otg_exp_probe_mismatches(None) == -1
