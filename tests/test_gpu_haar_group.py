"""Rectangle grouping on the GPU (ef_haar_group, Engine.haar_group) against
oracle/haar_oracle.group_rectangles, exactly, on the written lists of haar_group_cases.py."""
import numpy as np
import pytest

import haar_group_cases as hc
from oracle import haar_oracle as ho

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected():
    want = hc.check_cases_reach_their_branches()  # every written case reaches its branch of the oracle
    want["big"] = ho.group_rectangles(*hc.BIG)
    assert len(want["big"]) == 7
    return want


def _rects(case):
    rects, thr = hc.BIG if case == "big" else hc.CASES[case]
    return np.array(rects, np.int32).reshape(-1, 4), thr


@pytest.mark.parametrize("case", list(hc.CASES) + ["big"])
def test_group_equals_the_oracle(eng, expected, case):
    rects, thr = _rects(case)
    got = eng.haar_group(rects, thr)
    assert got.dtype == np.int32 and [tuple(int(v) for v in r) for r in got] == expected[case]
    again = eng.haar_group(rects, thr)  # no order of arrival reaches the result: the same bits
    np.testing.assert_array_equal(got, again)


@pytest.mark.parametrize("case", ["interleaved", "margin_out", "jitter_65", "big", "empty"])
def test_device_pointers(eng, expected, case):
    import torch
    rects, thr = _rects(case)
    want = np.array(expected[case], np.int32).reshape(-1, 4)
    out, cnt = eng.haar_group(torch.as_tensor(rects, device="cuda"), thr, max_rects=len(want) + 2)
    torch.cuda.synchronize()
    assert int(cnt.cpu()[0]) == len(want)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:len(want)], want)
    assert not got[len(want):].any()  # zero rectangles behind the grouped ones


def test_truncated_output_reports_the_total(eng, expected):
    import ctypes
    rects, thr = _rects("big")
    out = np.full((3, 4), -1, np.int32)
    n = ctypes.c_int32(-1)
    eng._chk(eng._lib.ef_haar_group(eng._h, rects.ctypes.data, len(rects), thr, out.ctypes.data, 3, ctypes.byref(n), 0))
    assert n.value == 7 and [tuple(int(v) for v in r) for r in out] == expected["big"][:3]


def test_overflow_and_argument_errors(eng, expected):
    from eigenface import EigenfaceError, _native as N
    rects, thr = _rects("chain")
    with pytest.raises(EigenfaceError, match="EF_E_INVALID"):  # the host function returns its input there
        eng.haar_group(rects, 0)
    with pytest.raises(EigenfaceError, match="EF_E_INVALID"):
        eng.haar_group(rects, -1)
    # one rectangle more than the kernels take: nothing is grouped, the status is reported
    many = np.tile(np.array([[5, 6, 30, 40]], np.int32), (N.EF_HAAR_GROUP_MAX + 1, 1))
    with pytest.raises(EigenfaceError, match="EF_HAAR_SCAN_OVERFLOW"):
        eng.haar_group(many, 2)
    got = eng.haar_group(many[:-1], 2)  # the capacity itself: one class of 16384 duplicates
    assert [tuple(int(v) for v in r) for r in got] == [(5, 6, 30, 40)]
    # and the next call is unaffected
    assert [tuple(int(v) for v in r) for r in eng.haar_group(rects, thr)] == expected["chain"]
