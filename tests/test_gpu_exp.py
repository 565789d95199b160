"""GPU: the device exp() of the clustering kernel (otg_exp<FMA>, through otg_exp_device) == its host restatement (otg_exp_host) on the whole
argument set of exp_args.py, bit for bit, in both variants.  With test_exp_host.py (restatement == libm) this ties the device function to
glibc; the non-FMA variant runs here whatever the host libm selects."""
import numpy as np
import pytest
import otter_amd
from exp_args import ARGS, mismatches

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", [1, 0], ids=["fma", "nofma"])
def test_device_exp_equals_host_restatement(gpu, variant):
    want = otter_amd.exp_host(ARGS, variant)
    got = gpu.exp_device(ARGS, variant)
    bad = mismatches(got, want)
    assert bad.size == 0, [(float(ARGS[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]]


def test_probe_on_this_host(gpu):
    """The context's variant is the probe's, and the probe's mismatch count is reported (0: the host libm is one of glibc's two builds)."""
    p = otter_amd.exp_probe()
    assert gpu.exp_variant == p["variant"]
    assert gpu.exp_probe_mismatches == (p["mismatches_fma"] if p["variant"] else p["mismatches_nofma"])
    print("host libm probe: variant %d, %d mismatches over %d arguments (%d discriminating)" % (p["variant"], gpu.exp_probe_mismatches, p["n_args"], p["n_differ"]))
