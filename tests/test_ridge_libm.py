"""exp_libm (cice4_amd/csrc/libm_exact.h) below -512, where ridging takes it (thin ice: exp(-(hR - hrmin)/hrexp) with
hrexp = mu_rdg sqrt(hi)): glibc's specialcase branch for 512 <= |x| < 1024 and zero below.  Here the restatement, compiled
for the host, against the host libm on a dense sweep of [-1100, -500] and random negative arguments.  A guard: the device
side is carried by tests/test_gpu_ridge.py, whose fixture holds denormal and zero areas that come out of this branch."""
import os
import subprocess
import tempfile

import pytest

from test_libm_exact import _host_has_fma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exp_restatement_equals_host_libm_on_the_negative_tail():
    if not _host_has_fma():
        pytest.skip("host CPU without FMA: glibc selects its non-FMA exp build here")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "probe")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma",
                               os.path.join(ROOT, "tests", "libm_probe_neg.cpp"), "-o", exe])
        out = subprocess.run([exe, "2000000"], capture_output=True, text=True, check=True).stdout
    assert "mismatches=0" in out and "checked=4000013" in out, out
