"""Frame scan (ef_scan_prepare / ef_scan_frame, eigenface.scanner.FrameScanner): one call per
frame against the oracle's template_match_all_models, the oracle's preprocess of the crops, the
bank's own recognise call on the returned rows, and the restated host rules of
scan-template-v4.py:351-401."""
import numpy as np
import pytest

import parity_util
import scan_util
from oracle import image_oracle as io

pytestmark = pytest.mark.gpu

PERSONS = ["alice", "bob", "carol"]


@pytest.fixture(scope="module")
def case():
    """The 180 x 240 case of test_template_localiser_matches_reference_loop as a BGR frame:
    alice's first template is cut from the grey of the frame, bob matches nothing above 0.6,
    carol's best match sits in the border.  Plus the frame rolled by 7 columns, the oracle's
    detections of both, and three tiny trained models."""
    rng = np.random.default_rng(12)
    bgr = rng.integers(0, 256, (180, 240, 3), dtype=np.uint8)
    grey = io.bgr2gray(bgr)
    templates = {
        "alice": [grey[60:100, 90:125].copy(), rng.integers(0, 256, (30, 30), dtype=np.uint8)],
        "bob": [rng.integers(0, 256, (25, 40), dtype=np.uint8)],
        "carol": [grey[2:40, 3:40].copy()],
    }
    models = {}
    for i, (p, n) in enumerate(zip(PERSONS, (60, 56, 52))):
        _, md = scan_util.trained(p, n, 40 + i)
        models[p] = {"model_data": md, "template_images": [{"image": t} for t in templates[p]],
                     "detection_data": {"faces": [{}]}}
    frames = [bgr, np.roll(bgr, 7, axis=1)]
    refs = [io.template_match_all_models(io.bgr2gray(f), templates) for f in frames]
    assert [d["person_name"] for d in refs[0]] == ["alice"] and (refs[0][0]["x"], refs[0][0]["y"]) == (90, 60)
    return {"frames": frames, "refs": refs, "templates": templates, "models": models}


@pytest.fixture(scope="module")
def scanner(case):
    from eigenface import FrameScanner
    return FrameScanner(case["models"], (180, 240))


def _check_dets(scanner, dets, frame, ref):
    by_person = {d["person_name"]: d for d in ref}
    grey = io.bgr2gray(frame)
    want_rows = np.zeros((len(PERSONS), 4096), np.uint8)
    for g, person in enumerate(PERSONS):
        d = dets[g]
        r = by_person.get(person)
        if r is None:
            assert all(int(d[f]) == 0 for f in ("found", "problem", "x", "y", "w", "h", "pad")), (person, d)
            assert np.float32(d["confidence"]).view(np.int32) == 0
            continue
        assert int(d["found"]) == 1
        assert (int(d["x"]), int(d["y"]), int(d["w"]), int(d["h"])) == (r["x"], r["y"], r["width"], r["height"])
        assert scanner.localiser.meta[int(d["problem"])][:2] == (person, r["scale"])
        assert np.float32(d["confidence"]).view(np.int32) == np.float32(r["confidence"]).view(np.int32)
        want_rows[g] = io.preprocess(grey[r["y"]:r["y"] + r["height"], r["x"]:r["x"] + r["width"]].copy())
    return want_rows


@pytest.mark.parametrize("which", [0, 1])
def test_scan_matches_the_oracle_and_the_bank(case, scanner, which):
    from eigenface import decode_keys, get_engine
    frame, ref = case["frames"][which], case["refs"][which]
    dets, keys, best, rows = scanner.scan_raw(frame)
    assert keys.shape == (3, 3) and best.shape == (3,) and rows.shape == (3, 4096)
    want_rows = _check_dets(scanner, dets, frame, ref)
    np.testing.assert_array_equal(rows, want_rows)
    # the bank's own call on the returned rows, the same b
    eng = get_engine(0)
    keys2, _, best2, feats = eng.bank_recognize_raw(rows, "cosine", features=True)
    np.testing.assert_array_equal(keys, keys2)
    np.testing.assert_array_equal(best, best2)
    # every key outside the tie window is the fp64 first arg-best
    found = np.flatnonzero(dets["found"])
    assert len(found) == len(ref)
    off = 0
    for m, person in enumerate(PERSONS):
        g = np.ascontiguousarray(case["models"][person]["model_data"]["face_features"], dtype=np.float32)
        k = g.shape[1]
        f = np.ascontiguousarray(feats[found, off:off + k])
        off += k
        idx, _ = decode_keys(np.ascontiguousarray(keys[found, m]), "cosine")
        parity_util.assert_exact_argbest(f, g, idx, "cosine")
    # the records: the restated host rules on the oracle's detections and the bank's labels of
    # the same rows (all of them: the bank's K-split depends on the batch size)
    labels = scanner.bank.recognize_rows(rows)
    pca = [labels[g] for g in found]
    want = scan_util.records_from_lists(ref, pca)
    got = scanner.scan_frame(frame)
    assert got == want and len(got) == (1 if ref else 0)
    dd, pp = scanner.scan(frame)
    assert [{k: d[k] for k in r} for d, r in zip(dd, ref)] == ref and pp == pca
    recs = list(scanner.process_frames([frame, frame]))
    assert recs == [{"frame_number": n, **r} for n in (0, 1) for r in want]


def test_grey_frame_and_device_form_equal_the_host_form(case, scanner):
    import torch
    from eigenface import get_engine
    frame = case["frames"][0]
    host = scanner.scan_raw(frame)
    # a grey frame and its BGR replication (the BT.601 weights sum to 2^14)
    grey = io.bgr2gray(frame)
    for other in (scanner.scan_raw(grey), scanner.scan_raw(np.repeat(grey[:, :, None], 3, axis=2)),
                  scanner.scan_raw(np.ascontiguousarray(frame[..., ::-1]), rgb=True),
                  scanner.scan_raw(np.concatenate([frame, frame[..., :1]], axis=2))):
        for a, b in zip(host, other):
            np.testing.assert_array_equal(a.view(np.uint8) if a.dtype.names else a,
                                          b.view(np.uint8) if b.dtype.names else b)
    # device tensors: a row-strided view, nothing waits on the host
    eng = get_engine(0)
    wide = torch.zeros((180, 250, 3), dtype=torch.uint8, device="cuda")
    wide[:, :240] = torch.as_tensor(frame, device="cuda")
    dets, keys, best, rows = eng.scan_frame(wide[:, :240])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dets.cpu().numpy().reshape(-1), host[0].view(np.int32).reshape(-1))
    np.testing.assert_array_equal(keys.cpu().numpy(), host[1])
    np.testing.assert_array_equal(best.cpu().numpy(), host[2])
    np.testing.assert_array_equal(rows.cpu().numpy(), host[3])


def test_odd_frame_width(case):
    """A 70 x 101 frame: the grey kernel's groups of four pixels straddle row ends and the rows
    of a BGR frame start at every alignment; one template cut from the frame, one of noise."""
    from eigenface import FrameScanner
    rng = np.random.default_rng(77)
    bgr = rng.integers(0, 256, (70, 101, 3), dtype=np.uint8)
    grey = io.bgr2gray(bgr)
    templates = {"alice": [grey[20:46, 30:58].copy()], "bob": [rng.integers(0, 256, (24, 24), dtype=np.uint8)]}
    models = {p: {"model_data": case["models"][p]["model_data"], "template_images": templates[p]} for p in templates}
    sc = FrameScanner(models, (70, 101))
    ref = io.template_match_all_models(grey, templates)
    assert [(d["person_name"], d["x"], d["y"]) for d in ref] == [("alice", 30, 20)]
    dets, keys, best, rows = sc.scan_raw(bgr)
    assert [int(v) for v in dets["found"]] == [1, 0]
    assert (int(dets["x"][0]), int(dets["y"][0]), int(dets["w"][0]), int(dets["h"][0])) == (30, 20, 28, 26)
    assert np.float32(dets["confidence"][0]).view(np.int32) == np.float32(ref[0]["confidence"]).view(np.int32)
    np.testing.assert_array_equal(rows[0], io.preprocess(grey[20:46, 30:58].copy()))
    assert not rows[1].any()
    for other in (sc.scan_raw(grey), sc.scan_raw(np.concatenate([bgr, bgr[..., :1]], axis=2))):
        np.testing.assert_array_equal(other[0].view(np.uint8), dets.view(np.uint8))
        np.testing.assert_array_equal(other[3], rows)
        np.testing.assert_array_equal(other[1], keys)


# 120 x 160 frame: corner 24 x 18, border 8 x 6.  Top-left corners of a 20 (h) x 24 (w)
# template that is_detection_in_corner rejects (one comparison each), and the nearest ones it
# accepts.
REJECTED = {"corner_tl": (9, 6), "corner_tr": (126, 6), "corner_bl": (9, 93), "corner_br": (126, 93),
            "border_left": (7, 50), "border_top": (60, 5), "border_right": (129, 50), "border_bottom": (60, 95)}
ACCEPTED = {"edge_tl": (12, 8), "edge_br": (124, 92), "edge_right": (128, 50), "edge_bottom": (60, 94),
            "edge_tr_x": (124, 6), "edge_bl_y": (9, 92)}


def test_corner_rule_and_ties_on_the_device(case):
    """Every comparison of the corner / border rule in the selection kernel, and ties in v.
    Each person's first template is cut from the frame at one of the positions above (v = 1
    there); its second is a noisy copy of a patch in the middle (0.6 < v < 1).  A rejected first
    template must not shadow the second; an accepted one wins.  Two persons hold the same
    template twice (alone, and behind a rejected one): the first of the equal problems wins."""
    from eigenface import FrameScanner
    rng = np.random.default_rng(5)
    grey = rng.integers(0, 256, (120, 160), dtype=np.uint8)
    for name, (x, y) in {**REJECTED, **ACCEPTED}.items():
        assert io.is_detection_in_corner({"x": x, "y": y, "width": 24, "height": 20}, 160, 120) == (name in REJECTED)
    mid = grey[50:70, 70:94]
    templates = {}
    for name, (x, y) in {**REJECTED, **ACCEPTED}.items():
        noisy = np.clip(mid.astype(np.int32) + rng.integers(-40, 41, mid.shape), 0, 255).astype(np.uint8)
        templates[name] = [grey[y:y + 20, x:x + 24].copy(), noisy]
    templates["tie"] = [mid.copy(), mid.copy()]
    templates["tie_behind_corner"] = [grey[6:26, 9:33].copy(), mid.copy(), mid.copy()]
    mds = [case["models"][p]["model_data"] for p in PERSONS]
    models = {p: {"model_data": mds[i % 3], "template_images": t} for i, (p, t) in enumerate(templates.items())}
    sc = FrameScanner(models, grey.shape)
    ref = {d["person_name"]: d for d in io.template_match_all_models(grey, templates)}
    assert set(ref) == set(templates)  # every person is found, by one template or the other
    dets, _, _, rows = sc.scan_raw(grey)
    meta = sc.localiser.meta
    for g, person in enumerate(sc.persons):
        d, r = dets[g], ref[person]
        got = (int(d["found"]), int(d["x"]), int(d["y"]), int(d["w"]), int(d["h"]), meta[int(d["problem"])][1])
        assert got == (1, r["x"], r["y"], r["width"], r["height"], r["scale"]), person
        assert np.float32(d["confidence"]).view(np.int32) == np.float32(r["confidence"]).view(np.int32), person
        first = (r["x"], r["y"]) != (70, 50)
        if person in REJECTED:
            assert not first and 0.6 < r["confidence"] < 1.0, person
        elif person in ACCEPTED:
            assert first and r["confidence"] == 1.0, person
        np.testing.assert_array_equal(
            rows[g], io.preprocess(grey[r["y"]:r["y"] + r["height"], r["x"]:r["x"] + r["width"]].copy()))
    # equal v: the lowest problem index (the problems of a person are consecutive, templates in order)
    first_of = {p: [m[0] for m in meta].index(p) for p in ("tie", "tie_behind_corner")}
    assert int(dets[sc.persons.index("tie")]["problem"]) == first_of["tie"]
    assert int(dets[sc.persons.index("tie_behind_corner")]["problem"]) == first_of["tie_behind_corner"] + 2


def test_scan_timer(case, scanner):
    from eigenface import get_engine
    eng = get_engine(0)
    scanner.scan_raw(case["frames"][0])
    eng.timing(True)
    eng.timing_reset()
    try:
        scanner.scan_raw(case["frames"][0])
        scanner.scan_raw(case["frames"][1])
        ms, n = eng.timing_get("scan")
        assert n == 2 and 0 < ms < 1000
        assert eng.timing_get("tmatch")[1] == 0  # the localiser's own timer belongs to ef_tm_match
        assert eng.timing_get("ingest")[1] == 0
        # the bank's launches inside a scan count under its own two timers as well
        assert eng.timing_get("project")[1] == 2 and eng.timing_get("search")[1] == 2
    finally:
        eng.timing(False)
        eng.timing_reset()


def test_states_and_recovery(case):
    """EF_E_STATE without a plan, after a new ef_tm_prepare, with an empty bank and with a bank
    of another d; the next good call is correct."""
    from eigenface import EigenfaceError, Engine
    from eigenface.compat import _folded
    frame, ref = case["frames"][0], case["refs"][0]
    tm = [t for p in PERSONS for t in case["templates"][p]]
    probs, groups = [], []
    gi = 0
    ti = 0
    for p in PERSONS:
        for t in case["templates"][p]:
            for _, nw, nh in io.scaled_sizes(t.shape[0], t.shape[1], 180, 240):
                probs.append((ti, nh, nw))
                groups.append(gi)
            ti += 1
        gi += 1

    def fill(e):
        e.bank_clear()
        for p in PERSONS:
            md = case["models"][p]["model_data"]
            mu, w = _folded(md)
            e.bank_add(mu, w, np.ascontiguousarray(md["face_features"], dtype=np.float32))

    with Engine(0) as e:
        fill(e)
        with pytest.raises(EigenfaceError, match="EF_E_STATE"):  # no localiser at all
            e.scan_frame(frame)
        with pytest.raises(EigenfaceError, match="EF_E_STATE"):
            e.scan_prepare(groups, 3)
        e.tm_prepare(tm, probs, (180, 240))
        with pytest.raises(EigenfaceError, match="EF_E_STATE"):  # a localiser, no plan
            e.scan_frame(frame)
        with pytest.raises(EigenfaceError, match="EF_E_INVALID"):
            e.scan_prepare([3] * len(groups), 3)
        e.scan_prepare(groups, 3)
        good = e.scan_frame(frame)
        assert [int(v) for v in good[0]["found"]] == [1, 0, 0]
        assert (int(good[0]["x"][0]), int(good[0]["y"][0])) == (ref[0]["x"], ref[0]["y"])
        # a new ef_tm_prepare drops the plan: the library refuses real arguments too
        plan = e._scan
        e.tm_prepare(tm, probs, (180, 240))
        e._scan = plan
        with pytest.raises(EigenfaceError, match="EF_E_STATE"):
            e.scan_frame(frame)
        e.scan_prepare(groups, 3)
        e.bank_clear()
        with pytest.raises(EigenfaceError, match="EF_E_STATE"):  # empty bank
            e.scan_frame(frame)
        e.bank_add(np.zeros(100, np.float32), np.zeros((100, 4), np.float32), np.ones((2, 4), np.float32))
        with pytest.raises(EigenfaceError, match="EF_E_STATE"):  # bank d != 64 * 64
            e.scan_frame(frame)
        with pytest.raises(EigenfaceError, match="EF_E_INVALID"):  # (and a bad frame stride)
            fill(e)
            e._chk(e._lib.ef_scan_frame(e._h, frame.ctypes.data, 240, 3, 1, good[0].ctypes.data,
                                        good[1].ctypes.data, None, None, 0))
        again = e.scan_frame(frame)
        for a, b in zip(good, again):
            np.testing.assert_array_equal(a.view(np.uint8) if a.dtype.names else a,
                                          b.view(np.uint8) if b.dtype.names else b)
