"""The fit's matrix-product and eigen-solver kernels, one by one, against host references.

tests/native/kernel_units.cpp links the product objects (`make kernel_units`) and calls the
internal launchers of csrc/ef_linalg.hpp directly: the tall fp64 / fp32 GEMMs and transposes,
the split-bf16 coarse product, the int8 digit-split product in its full and medium forms, the
Cholesky factorisation and triangular inverse of CholQR, both Jacobi solvers, the exact int8
covariance / Gram with its transposes and finalize (against __int128 references) and the int8
digit training projection.  Each group
runs as a child process that prints one line per case and exits non-zero on any FAIL; exact
(small-integer) cases must be bit-equal, rounding cases stay inside a bound written out in
the program (DESIGN.md "Kernel-level numerics" lists them with the measured ratios).
`kernel_units --host` checks the references against their own bounds and needs no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PKG = os.path.join(ROOT, "face-detection-recognization-pca_amd")
BIN = os.path.join(PKG, "build", "kernel_units")

# set once a child ended on a signal or hit its time limit: nothing more is started
_dead = []


@pytest.fixture(scope="module")
def kernel_units():
    jobs = str(min(8, os.cpu_count() or 4))
    r = subprocess.run(["make", "-C", PKG, "-j", jobs, "kernel_units"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("kernel_units build failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    return BIN


def _run(exe, arg):
    if _dead:
        pytest.fail("not started: an earlier kernel_units child " + _dead[0])
    try:
        r = subprocess.run([exe, arg], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        _dead.append(f"({arg}) hit its time limit")
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        print(out[-4000:])
        pytest.fail(f"kernel_units {arg}: time limit")
    bad = [ln for ln in r.stdout.splitlines() if "FAIL" in ln]
    if r.returncode != 0 or bad:
        print(r.stdout[-20000:], r.stderr[-4000:])
    if r.returncode < 0:
        _dead.append(f"({arg}) ended on signal {-r.returncode}")
    elif r.returncode == 2:  # the program's exit status after a failed HIP call
        _dead.append(f"({arg}) stopped at a HIP error")
    assert r.returncode == 0, f"kernel_units {arg}: exit status {r.returncode}\n" + "\n".join(bad[:40])
    assert not bad, "\n".join(bad[:40])
    assert "case=" in r.stdout
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["tall", "s3", "cq", "chol", "jacobi", "cov", "proj"])
def test_kernel_group(kernel_units, group):
    out = _run(kernel_units, group)
    assert f"kernel_units {group}: ok" in out


def test_host_references_meet_their_bounds(kernel_units):
    out = _run(kernel_units, "--host")
    assert "kernel_units --host: ok" in out
