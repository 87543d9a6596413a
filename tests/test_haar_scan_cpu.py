"""Host side of the Haar route in one call (no GPU): the three labelling rules against literal
restatements of useless/scan.py:130-166, :205-213, the four new entry points in the header and
the library, argument errors that need no device, and the written grouping cases against the
oracle's branches."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ("ef_haar_group", "ef_haar_scan_prepare", "ef_haar_scan_info", "ef_haar_scan_frame")


def _ref_recognize_face(person_name, similarities, similarity_threshold):
    """useless/scan.py:126-132."""
    max_similarity = max(similarities)
    is_recognized = max_similarity >= similarity_threshold
    return person_name, max_similarity, is_recognized


def _ref_dual(dark, light, similarity_threshold):
    """useless/scan.py:147-166; dark, light: (person_name, similarities)."""
    dark_name, dark_similarity, dark_recognized = _ref_recognize_face(*dark, similarity_threshold)
    light_name, light_similarity, light_recognized = _ref_recognize_face(*light, similarity_threshold)
    is_recognized = dark_recognized or light_recognized
    best_confidence = max(dark_similarity, light_similarity)
    person_name = dark_name if dark_similarity >= light_similarity else light_name
    return person_name, best_confidence, is_recognized


SIMS = [0.0, 0.3, 0.6999999, 0.7, 0.7000001, 0.95, 1.0, -0.2]


def test_label_one_is_the_single_model_rule():
    from eigenface import label_one
    for s in SIMS:
        for thr in (0.7, 0.3, 1.0):
            assert label_one("ann", np.float32(s), thr) == _ref_recognize_face("ann", [-1.0, float(np.float32(s))], thr)
    name, conf, flag = label_one("ann", np.float32(0.7), 0.7)
    assert isinstance(conf, float) and flag is False  # float32(0.7) < 0.7: the comparison is in double
    assert label_one("ann", float("nan"), 0.7)[2] is False  # an empty gallery is never recognised


def test_label_pair_is_the_dual_model_rule():
    from eigenface import label_pair
    for d in SIMS:
        for l in SIMS:
            want = _ref_dual(("dark", [d]), ("light", [l]), 0.7)
            assert label_pair("dark", d, "light", l, 0.7) == want, (d, l)
    assert label_pair("dark", 0.5, "light", 0.5, 0.7) == ("dark", 0.5, False)  # the dark name on a tie
    assert label_pair("dark", 0.2, "light", 0.8, 0.7) == ("light", 0.8, True)  # OR of the flags
    assert label_pair("dark", 0.9, "light", 0.1, 0.7) == ("dark", 0.9, True)


def test_label_bank_is_the_banks_rule_in_the_haar_layout():
    from eigenface import ModelBank, label_bank
    bank = object.__new__(ModelBank)  # the labelling needs no engine
    bank.names = ["ann", "bob"]
    bank.face_labels = [[0, 0], [7, 7, 7]]
    bank.person_id_maps = [{"ann": 0}, {"robert": 7}]
    idx = np.array([[1, 2], [0, 0], [0, -1], [1, 1]])
    sim = np.array([[0.9, 0.95], [0.5, 0.4], [0.0, np.nan], [0.85, 0.85]], np.float32)
    want = [("robert", float(np.float32(0.95)), True),   # the later model wins with a greater similarity
            ("ann", 0.5, False),                          # below the threshold: the model's own name, not recognised
            ("unknown", 0.0, False),                      # nothing above 0
            ("ann", float(np.float32(0.85)), True)]      # a tie: the first model
    assert label_bank(bank, idx, sim, 0.8) == want
    allowed = np.array([[True, False], [True, True], [True, True], [False, True]])
    got = label_bank(bank, idx, sim, 0.8, allowed)
    assert got[0] == ("ann", float(np.float32(0.9)), True) and got[3] == ("robert", float(np.float32(0.85)), True)


def test_pca_model_dicts_are_read_in_the_banks_layout():
    from eigenface.scanner import _bank_layout
    md = {"eigenfaces": np.zeros((16, 3), np.float32), "mean_face": np.zeros(16, np.float32),
          "projected_data": np.ones((5, 3), np.float32), "person_name": "ann", "face_dimensions": 16}
    out = _bank_layout(md, "key")
    assert out["face_features"] is not None and out["face_features"].shape == (5, 3)
    assert list(out["face_labels"]) == [0] * 5 and out["person_id_map"] == {"ann": 0}
    assert "face_features" not in md  # the caller's dict is left alone
    other = {"pca": object(), "face_features": 1}
    assert _bank_layout(other, "key") is other and _bank_layout(None, "key") is None


def test_header_declares_and_library_exports_the_new_symbols():
    from eigenface import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eigenface.h")).read(), flags=re.S)
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for n in NEW_SYMBOLS:
        assert re.search(rf"\bint {n}\s*\(", src), n
        assert n in _native.EXPORTED_SYMBOLS and hasattr(lib, n)
        assert re.search(rf"\bT {n}$", out, re.M), n
    assert "typedef struct ef_haar_scan_head" in src
    for name, value in (("EF_HAAR_GROUP_MAX", _native.EF_HAAR_GROUP_MAX), ("EF_HAAR_SCAN_OVERFLOW", 1),
                        ("EF_HAAR_SCAN_UNCONVERGED", 2), ("EF_KERNEL_HAAR_SCAN", _native.EF_KERNEL_HAAR_SCAN)):
        m = re.search(rf"#define {name} (\w+)", src)
        assert m and int(m.group(1), 0) == value, name
    assert _native.EF_HAAR_GROUP_MAX >= 4096
    assert np.dtype(_native.HAAR_SCAN_HEAD_DTYPE).itemsize == 16


def test_argument_errors_that_need_no_device():
    from eigenface import Engine, _native
    lib = _native.lib()
    n = ctypes.c_int32(0)
    r = np.zeros((2, 4), np.int32)
    assert lib.ef_haar_group(None, r.ctypes.data, 2, 3, r.ctypes.data, 2, ctypes.byref(n), 0) == -1
    assert lib.ef_haar_scan_prepare(None, 120, 160, 1.1, 5, 30, 30, 0, 0, 64, 64, 8, 4096) == -1
    assert lib.ef_haar_scan_info(None, None, None, None, None) == -1
    assert lib.ef_haar_scan_frame(None, None, 0, 1, 1, None, None, None, None, None, None, None, None, 0) == -1
    e = object.__new__(Engine)  # no context: the shape checks run before any C call
    e._lib, e._h = lib, ctypes.c_void_p()
    for bad in (np.zeros((3, 3), np.int32), np.zeros(8, np.int32)):
        with pytest.raises(ValueError):
            e.haar_group(bad, 3)
    with pytest.raises(KeyError):
        e.timing_get("no_such_timer")


def test_written_grouping_cases_reach_their_branches():
    import haar_group_cases as hc
    got = hc.check_cases_reach_their_branches()
    assert set(got) == set(hc.CASES)
