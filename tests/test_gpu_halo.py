"""The device ghost-cell update (cice4_amd/csrc/halo.hip, capi_halo.hip) at every field location, kind and type, against
the one-rank lists applied in numpy -- which tests/test_boundary.py holds equal to the compiled reference.  One child
process per (domain, environment switch): tests/halo_device_case.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = os.path.join(ROOT, "tests", "halo_device_case.py")
FRAME_ENV, SELF_ENV = "CICE4_AMD_HALO_HOST_ON_DEVICE", "CICE4_AMD_SELF_COMM"
FOLD_DOMAINS = ("u2x2", "t2x2", "pad3x3", "tiny", "elim")


def run_child(mode, name, **env):
    """-> (number of checks the child counted, its digest or None)"""
    e = {k: v for k, v in os.environ.items() if k not in (FRAME_ENV, SELF_ENV)}
    e.update(env)
    p = subprocess.run([sys.executable, CASE, mode, name], capture_output=True, text=True, timeout=300, env=e)
    ok = re.search(r"^HALO-OK (\d+)$", p.stdout, re.M)
    assert p.returncode == 0 and ok, p.stdout[-2000:] + p.stderr[-4000:]
    assert int(ok.group(1)) > 0
    print(f"halo_device_case {mode} {name} {sorted(env)}: {ok.group(1)} checks")
    dg = re.search(r"^HALO-DIGEST ([0-9a-f]{64})$", p.stdout, re.M)
    return int(ok.group(1)), dg.group(1) if dg else None


@pytest.mark.parametrize("name", FOLD_DOMAINS + ("closed", "lds-u", "lds-t"))
def test_halo_case_facts_and_host_path(name):
    """No device: the facts the GPU cases rely on (symmetric pairs at the locations a fold has them, folded cells per
    location, the gap an eliminated top-row block leaves, frame sizes, closed == open lists), and the host path of
    cice_halo_update_blocked_* / cice_halo_update_strided_r8 with both fill values against numpy."""
    run_child("facts", name)
    n, digest = run_child("blocked", name)
    assert digest and n > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", FOLD_DOMAINS + ("closed",))
def test_halo_update_on_device(name):
    """cice_halo_update_ex_{r8,r4,i4} and cice_halo_update_dev_ex_r8: float64 / float32 / int32 x four locations x three
    kinds x 1, 3, 65 levels x fill 0 and non-zero; ghost cells, fill cells and folded cells bit for bit, every other cell
    untouched."""
    run_child("device", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FOLD_DOMAINS)
def test_host_array_through_the_frame_path(name):
    """cice_halo_update_blocked_* and cice_halo_update_strided_r8 with CICE4_AMD_HALO_HOST_ON_DEVICE=1: the update runs on
    the gathered frame (a second Halo, lists re-addressed to frame positions, fold lists included) or, where the frame is
    more than half the field ('tiny'), on the whole field through strided copies.  The same calls in a child without the
    variable run on the host and must give the same bits."""
    n_dev, on_device = run_child("blocked", name, **{FRAME_ENV: "1"})
    n_host, on_host = run_child("blocked", name)
    assert n_dev == n_host and on_device and on_device == on_host


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("u2x2", "t2x2", "pad3x3", "elim"))
def test_halo_update_through_messages_to_the_own_rank(name):
    """CICE4_AMD_SELF_COMM=1: copies between blocks travel as pack -> message to the own rank -> unpack, the fold behind
    them; expected values from a context created without the variable."""
    run_child("selfcomm", name, **{SELF_ENV: "1"})


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("lds-u", "lds-t"))
def test_fold_path_switch(name):
    """Halo::update_fold runs the one-workgroup LDS kernel while fold_rows * nxg * nlev * itemsize <= 64 KB and four
    kernels above: the last level count below and the first above, every type x location x kind (float64 under the U-fold:
    32 levels = the LDS kernel's largest allocation), and an LDS call straight after a four-kernel call that grew the
    buffer."""
    run_child("switch", name)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", (3, 4), ids=("tripole", "tripoleT"))
def test_fold_between_ranks(ns):
    """Ranks as threads of one process (cice_comm_init_local): two ranks that both hold top-row blocks, and four ranks of
    which two hold none -- fold rows travel between ranks into the fold buffer.  Every block == the block of the same
    global id of the one-rank domain updated in numpy."""
    run_child("ranks", str(ns))
