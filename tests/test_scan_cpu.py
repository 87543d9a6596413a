"""The frame scanner's host rules (eigenface.scanner.decide, corner_integers) against the
restatement of scan-template-v4.py:351-401 in tests/scan_util.py.  No GPU."""
import itertools

import numpy as np
import pytest

import scan_util
from oracle import image_oracle as io


def _det(person, w, h, conf, x=50, y=40):
    return {"x": x, "y": y, "width": w, "height": h, "person_name": person, "confidence": conf, "scale": 1.0}


def _check(dets, pca):
    from eigenface.scanner import decide
    before = [dict(d) for d in dets]
    got = decide(dets, pca)
    assert dets == before  # pure: the inputs are not written to
    want = scan_util.records_from_lists(dets, pca)
    assert got == want
    for g, w in zip(got, want):
        assert list(g) == list(w)  # the reference's key order
    return got


def test_single_detection_keeps_template_name_when_names_agree():
    got = _check([_det("alice", 60, 60, 0.9)], [(3, "alice", 0.95)])
    assert got == [{"person_name": "alice", "template_confidence": 0.9, "pca_confidence": 0.95,
                    "final_confidence": 0.9, "x": 50, "y": 40, "width": 60, "height": 60}]


def test_empty_list():
    assert _check([], []) == []


def test_selection_by_size_and_by_pca_confidence():
    # equal PCA confidence: the larger rectangle wins (second); sizes above 200 x 200 saturate
    got = _check([_det("a", 50, 50, 0.9), _det("b", 120, 100, 0.9, x=70)], [(0, "a", 0.9), (1, "b", 0.9)])
    assert len(got) == 1 and got[0]["x"] == 70
    # equal size: the higher PCA confidence wins (first)
    got = _check([_det("a", 80, 80, 0.9), _det("b", 80, 80, 0.9, x=70)], [(0, "a", 0.97), (1, "b", 0.85)])
    assert len(got) == 1 and got[0]["x"] == 50
    # a small face with a high PCA confidence beats a large one with a low confidence
    got = _check([_det("a", 200, 200, 0.9), _det("b", 40, 40, 0.9, x=70)], [(0, "a", 0.1), (1, "b", 0.99)])
    assert got[0]["x"] == 50  # 0.5 + 0.05 > 0.02 + 0.495: size still wins here
    got = _check([_det("a", 100, 100, 0.9), _det("b", 40, 40, 0.9, x=70)], [(0, "a", 0.1), (1, "b", 0.99)])
    assert got[0]["x"] == 70  # 0.125 + 0.05 < 0.02 + 0.495
    # both saturated (> 200 x 200): PCA confidence alone decides
    got = _check([_det("a", 300, 300, 0.9), _det("b", 210, 200, 0.9, x=70)], [(0, "a", 0.5), (1, "b", 0.6)])
    assert got[0]["x"] == 70


def test_exact_tie_in_the_combined_score_keeps_the_first():
    dets = [_det("a", 100, 100, 0.9), _det("b", 100, 100, 0.9, x=70), _det("c", 100, 100, 0.9, x=90)]
    got = _check(dets, [(0, "a", 0.75), (1, "b", 0.75), (2, "c", 0.75)])
    assert len(got) == 1 and got[0]["x"] == 50
    # a different split of the same sum: 0.25 * 0.5 + 0.875 * 0.5 == 1.0 * 0.5 + 0.125 * 0.5 exactly
    got = _check([_det("a", 100, 100, 0.9), _det("b", 200, 200, 0.9, x=70)], [(0, "a", 0.875), (1, "b", 0.125)])
    assert got[0]["x"] == 50


@pytest.mark.parametrize("pca_conf", [0.49, 0.5, 0.51, 0.79, 0.8, 0.81])
@pytest.mark.parametrize("pca_name", ["alice", "bob"])
def test_name_and_confidence_branches_around_0_5_and_0_8(pca_name, pca_conf):
    got = _check([_det("alice", 60, 60, 0.9)], [(1, pca_name, pca_conf)])[0]
    takes_template = pca_name == "alice" or pca_conf < 0.5
    assert got["final_confidence"] == (0.9 if takes_template else pca_conf)
    if pca_conf < 0.8:
        assert got["person_name"] == "unknown"
    else:
        assert got["person_name"] == ("alice" if takes_template else "bob")


@pytest.mark.parametrize("template_conf", [0.69, 0.7, 0.71])
def test_template_confidence_around_0_7(template_conf):
    got = _check([_det("alice", 60, 60, template_conf)], [(1, "alice", 0.9)])[0]
    assert got["person_name"] == ("unknown" if template_conf < 0.7 else "alice")
    assert got["final_confidence"] == template_conf


def test_float32_confidences_compare_as_the_reference_does():
    """Confidences arrive as Python floats made from float32 values: 0.8 as float32 is above
    0.8, 0.7 as float32 is below 0.7."""
    c8, c7 = float(np.float32(0.8)), float(np.float32(0.7))
    assert c8 > 0.8 and c7 < 0.7
    assert _check([_det("alice", 60, 60, 0.9)], [(1, "alice", c8)])[0]["person_name"] == "alice"
    assert _check([_det("alice", 60, 60, c7)], [(1, "alice", 0.9)])[0]["person_name"] == "unknown"


@pytest.mark.parametrize("fw,fh,want", [(640, 480, (96, 72, 32, 24)), (240, 180, (36, 27, 12, 9))])
def test_corner_integers_reproduce_is_detection_in_corner(fw, fh, want):
    """The four integers, and the rule built on them (the selection kernel's form: border, or a
    centre in a corner), against io.is_detection_in_corner on every rectangle position around
    the thresholds."""
    from eigenface.scanner import corner_integers
    cw, ch, bw, bh = corner_integers(fw, fh)
    assert (cw, ch, bw, bh) == want

    def rule(x, y, w, h):
        cx, cy = x + w // 2, y + h // 2
        border = x < bw or y < bh or x + w > fw - bw or y + h > fh - bh
        return border or ((cx < cw or cx > fw - cw) and (cy < ch or cy > fh - ch))

    n = 0
    for w, h in [(20, 20), (35, 41), (64, 48)]:
        xs = sorted({v for b in (bw, cw - w // 2, fw - cw - w // 2, fw - bw - w) for v in range(b - 2, b + 3)
                     if 0 <= v <= fw - w})
        ys = sorted({v for b in (bh, ch - h // 2, fh - ch - h // 2, fh - bh - h) for v in range(b - 2, b + 3)
                     if 0 <= v <= fh - h})
        for x, y in itertools.product(xs, ys):
            assert rule(x, y, w, h) == scan_util.in_corner(x, y, w, h, fw, fh), (x, y, w, h)
            n += 1
    assert n > 300
    assert io.is_detection_in_corner({"x": 0, "y": 0, "width": 20, "height": 20}, fw, fh)
