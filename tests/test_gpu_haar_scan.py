"""Haar route in one call (ef_haar_scan_prepare / ef_haar_scan_frame, eigenface.scanner.HaarScanner)
against the separate calls it fuses: CascadeClassifier.detect on the grey frame, preprocess_rois of
its rectangles, and the bank's own recognise call on the returned rows with the same b."""
import numpy as np
import pytest

import haar_scan_util as u
from oracle import image_oracle as io

pytestmark = pytest.mark.gpu

THRESHOLD = 0.999  # a known face scores 1, the nearest stranger 0.9965 (the crops of one frame are alike)


def _detect(clf_cascade, grey):
    from eigenface.haar import CascadeClassifier
    return CascadeClassifier(cascade=clf_cascade).detect(grey, 1.1, 5, (30, 30), return_candidates=True)


@pytest.fixture(scope="module")
def case():
    """The frame, its grey plane, the detector's own rectangles on it (which the oracle gives too:
    tests/test_gpu_haar.py) and three models that know some of the four faces."""
    from eigenface import get_engine
    bgr = u.bgr_frame()
    grey = io.bgr2gray(bgr)
    rects, cand = _detect(u.cascade(), grey)
    assert [tuple(int(v) for v in r) for r in rects] == [(41, 40, 51, 51), (107, 15, 47, 47), (104, 64, 44, 44),
                                                       (5, 78, 36, 36)]
    face_rows = get_engine(0).preprocess_rois(grey, rects, (u.FACE, u.FACE))
    return {"bgr": bgr, "grey": grey, "rects": rects, "n_cand": len(cand), "models": u.models_for(face_rows)}


def _scanner(case, models=None, **kw):
    from eigenface import HaarScanner
    if models is None:
        models = {m["person_name"]: m for m in case["models"]}
    kw.setdefault("threshold", THRESHOLD)
    return HaarScanner(kw.pop("cascade", u.cascade()), models, u.SHAPE, **u.DETECT, **kw)


@pytest.fixture(scope="module")
def scanner(case):
    return _scanner(case)


def _check_against_separate_calls(sc, out, grey, rects, n_cand, gate=None):
    """head, rects, rows, keys and best slot of one scan against the separate calls on `grey`."""
    from eigenface import get_engine
    eng = get_engine(0)
    head, got_rects, keys, best, rows = out[:5]
    F, nf = sc.max_faces, min(len(rects), sc.max_faces)
    assert (int(head["n_rects"]), int(head["n_faces"]), int(head["n_candidates"])) == (len(rects), nf, n_cand)
    np.testing.assert_array_equal(got_rects[:nf], rects[:nf])
    assert not got_rects[nf:].any()
    want_rows = np.zeros((F, u.FACE * u.FACE), np.uint8)
    if nf:
        want_rows[:nf] = eng.preprocess_rois(grey, rects[:nf], (u.FACE, u.FACE))
    np.testing.assert_array_equal(rows, want_rows)
    if gate is None:
        keys2, _, best2, _ = eng.bank_recognize_raw(rows, "cosine")
    else:
        keys2, _, best2, _, eps2, en2 = eng.bank_recognize_gated_raw(rows, gate, "cosine", relative=True)
        np.testing.assert_array_equal(out[5].view(np.int32), eps2.view(np.int32))
        np.testing.assert_array_equal(out[6].view(np.int32), en2.view(np.int32))
    np.testing.assert_array_equal(keys, keys2)
    np.testing.assert_array_equal(best, best2)


def test_scan_equals_the_separate_calls(case, scanner):
    out = scanner.scan_raw(case["bgr"])
    assert int(out[0]["status"]) == 0 and out[2].shape == (8, 3) and out[4].shape == (8, u.FACE * u.FACE)
    _check_against_separate_calls(scanner, out, case["grey"], case["rects"], case["n_cand"])
    again = scanner.scan_raw(case["bgr"])
    assert tuple(again[0]) == tuple(out[0])
    for a, b in zip(out[1:], again[1:]):
        np.testing.assert_array_equal(a, b)


def test_input_forms(case, scanner):
    """RGB order, BGRA, a grey frame, row-strided host views and device tensors give the host BGR
    form's results (the grey frame: those of its own grey plane, which is the same plane)."""
    import torch
    from eigenface import get_engine
    bgr, grey = case["bgr"], case["grey"]
    host = scanner.scan_raw(bgr)
    wide = np.zeros((u.SHAPE[0], u.SHAPE[1] + 11, 3), np.uint8)
    wide[:, :u.SHAPE[1]] = bgr
    wide_grey = np.zeros((u.SHAPE[0], u.SHAPE[1] + 7), np.uint8)
    wide_grey[:, :u.SHAPE[1]] = grey
    others = [scanner.scan_raw(np.ascontiguousarray(bgr[..., ::-1]), rgb=True),
              scanner.scan_raw(np.concatenate([bgr, bgr[..., :1]], axis=2)),
              scanner.scan_raw(grey), scanner.scan_raw(wide[:, :u.SHAPE[1]]), scanner.scan_raw(wide_grey[:, :u.SHAPE[1]])]
    for other in others:
        assert tuple(other[0]) == tuple(host[0])
        for a, b in zip(host[1:], other[1:]):
            np.testing.assert_array_equal(a, b)
    eng = get_engine(0)
    for frame in (torch.as_tensor(wide, device="cuda")[:, :u.SHAPE[1]], torch.as_tensor(wide_grey, device="cuda")[:, :u.SHAPE[1]],
                  torch.as_tensor(bgr, device="cuda")):
        dev = eng.haar_scan_frame(frame)
        torch.cuda.synchronize()
        assert tuple(int(v) for v in dev[0].cpu()) == tuple(int(v) for v in host[0])
        for a, b in zip(host[1:], dev[1:]):
            np.testing.assert_array_equal(a, b.cpu().numpy())


def test_gated_scan_equals_the_gated_bank_call(case):
    sc = _scanner(case, face_gate=0.5)
    out = sc.scan_raw(case["bgr"])
    assert len(out) == 7 and out[5].shape == (8, 3) and np.isfinite(out[5][:4]).all()
    _check_against_separate_calls(sc, out, case["grey"], case["rects"], case["n_cand"], gate=sc.bank.gate)
    assert len(sc.scan(case["bgr"])) == 4


def _same(host, dev):
    """Host-form results against device-form ones, bit for bit."""
    assert len(dev) == len(host)
    assert tuple(int(v) for v in dev[0].cpu()) == tuple(int(v) for v in host[0])
    for a, b in zip(host[1:], dev[1:]):
        np.testing.assert_array_equal(a.view(np.uint8), b.cpu().numpy().view(np.uint8))


def test_gated_device_form_equals_the_host_form(case):
    """A device frame with the gate as a device tensor, and as a NumPy array (uploaded by the
    wrapper), against the gated host form."""
    import torch
    sc = _scanner(case, face_gate=0.5)
    host = sc.scan_raw(case["bgr"])
    assert len(host) == 7
    eng = sc._prepare()
    frame = torch.as_tensor(case["bgr"], device="cuda")
    for gate in (torch.as_tensor(sc.bank.gate, device="cuda"), sc.bank.gate):
        dev = eng.haar_scan_frame(frame, "cosine", gate=gate, relative=True)
        torch.cuda.synchronize()
        _same(host, dev)


def test_device_form_without_the_optional_outputs(case):
    """ef_haar_scan_frame on device pointers, gated, with best_slot, rows and energy left out (the
    rows and the energy then live in the plan's result block): head, rects, keys and dffs2 are byte
    for byte those of the call that is given every output, and those of the host form."""
    import torch
    from eigenface import _native as N
    sc = _scanner(case, face_gate=0.5)
    host = sc.scan_raw(case["bgr"])
    eng = sc._prepare()
    F, M, d = sc.max_faces, 3, u.FACE * u.FACE
    frame = torch.as_tensor(case["bgr"], device="cuda")
    gate = torch.as_tensor(sc.bank.gate, device="cuda")

    def ptr(t):
        return None if t is None else t.data_ptr()

    def call(optional):
        t = {"device": "cuda"}
        head = torch.zeros(4, dtype=torch.int32, **t)
        rects = torch.zeros((F, 4), dtype=torch.int32, **t)
        keys = torch.zeros((F, M), dtype=torch.int64, **t)
        eps = torch.zeros((F, M), dtype=torch.float32, **t)
        best = torch.zeros(F, dtype=torch.int32, **t) if optional else None
        rows = torch.zeros((F, d), dtype=torch.uint8, **t) if optional else None
        en = torch.zeros((F, M), dtype=torch.float32, **t) if optional else None
        with eng._torch_order(frame, gate, head, rects, keys, eps, best, rows, en):
            eng._chk(eng._lib.ef_haar_scan_frame(eng._h, frame.data_ptr(), u.SHAPE[1] * 3, 3, N.EF_METRIC_COSINE,
                                                 ptr(gate), ptr(head), ptr(rects), ptr(keys), ptr(best), ptr(rows),
                                                 ptr(eps), ptr(en), N.EF_BANK_GATE_RELATIVE | N.EF_MEM_DEVICE))
        torch.cuda.synchronize()
        return [head, rects, keys, best, rows, eps, en]

    bare, full = call(False), call(True)
    for i in (0, 1, 2, 5):
        np.testing.assert_array_equal(bare[i].cpu().numpy().view(np.uint8), full[i].cpu().numpy().view(np.uint8))
    _same(host, full)


def test_host_gate_is_uploaded_again_when_its_values_change(case):
    """Three host frames with gate A, gate B, then A again: the gate stays resident between calls,
    and each frame's best slots, dffs2 and energy are the bank's own gated call on the returned
    rows with that frame's gate.  B rejects the two slots A accepts the known faces in, so a gate
    left over from the frame before would change the best slots."""
    sc = _scanner(case, face_gate=0.5)
    eng = sc._prepare()
    gate_a = sc.bank.gate
    gate_b = np.array([-1.0, np.inf, -1.0], np.float32)
    outs = []
    for gate in (gate_a, gate_b, gate_a):
        out = eng.haar_scan_frame(case["bgr"], "cosine", gate=gate, relative=True)
        _, _, best2, _, eps2, en2 = eng.bank_recognize_gated_raw(out[4], gate, "cosine", relative=True)
        np.testing.assert_array_equal(out[3], best2)
        np.testing.assert_array_equal(out[5].view(np.int32), eps2.view(np.int32))
        np.testing.assert_array_equal(out[6].view(np.int32), en2.view(np.int32))
        outs.append(out)
    assert not np.array_equal(outs[0][3], outs[1][3])
    assert tuple(outs[2][0]) == tuple(outs[0][0])
    for a, b in zip(outs[0][1:], outs[2][1:]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


def test_frame_without_a_detection(case, scanner):
    flat = np.full(u.SHAPE + (3,), 117, np.uint8)
    head, rects, keys, best, rows = scanner.scan_raw(flat)
    assert (int(head["status"]), int(head["n_candidates"]), int(head["n_rects"]), int(head["n_faces"])) == (0, 0, 0, 0)
    assert not rects.any() and not rows.any()
    _check_against_separate_calls(scanner, (head, rects, keys, best, rows), flat[..., 0], np.zeros((0, 4), np.int32), 0)
    assert scanner.scan(flat) == []


def test_more_rectangles_than_max_faces(case):
    sc = _scanner(case, max_faces=1)
    out = sc.scan_raw(case["bgr"])
    assert int(out[0]["n_rects"]) == 4 and int(out[0]["n_faces"]) == 1 and out[1].shape == (1, 4)
    _check_against_separate_calls(sc, out, case["grey"], case["rects"], case["n_cand"])
    assert len(sc.scan(case["bgr"])) == 1


def test_overflow_falls_back_to_the_separate_calls(case, scanner):
    """1611 candidates against max_candidates = 64: the kernels group nothing and say so; the
    scanner redoes the frame through the separate calls and returns what the fused call returns
    when the candidates fit."""
    from eigenface import _native as N, get_engine
    fits = scanner.scan_raw(case["bgr"])
    sc = _scanner(case, max_candidates=64)
    eng = sc._prepare()
    head, rects, keys, best, rows = eng.haar_scan_frame(case["bgr"])
    assert int(head["status"]) == N.EF_HAAR_SCAN_OVERFLOW and int(head["n_candidates"]) == case["n_cand"]
    assert int(head["n_rects"]) == 0 and int(head["n_faces"]) == 0 and not rects.any() and not rows.any()
    keys2, _, best2, _ = get_engine(0).bank_recognize_raw(rows, "cosine")
    np.testing.assert_array_equal(keys, keys2)
    out = sc.scan_raw(case["bgr"])
    assert int(out[0]["status"]) == N.EF_HAAR_SCAN_OVERFLOW
    _check_against_separate_calls(sc, out, case["grey"], case["rects"], case["n_cand"])
    for a, b in zip(fits[1:], out[1:]):
        np.testing.assert_array_equal(a, b)
    assert sc.scan(case["bgr"]) == scanner.scan(case["bgr"])
    # 30 candidates fit 64: the fused path again
    few = _scanner(case, cascade=u.cascade(loose=0.5), max_candidates=64)
    rects_few, cand_few = _detect(u.cascade(loose=0.5), case["grey"])
    assert len(cand_few) == 30 and [tuple(int(v) for v in r) for r in rects_few] == [(44, 42, 57, 57)]
    out = few.scan_raw(case["bgr"])
    assert int(out[0]["status"]) == 0
    _check_against_separate_calls(few, out, case["grey"], rects_few, 30)


def test_ordered_cascade(case):
    """A cascade whose stage sums depend on the order of adding: the thread-per-window kernel."""
    from haar_util import order_free
    c = u.cascade(ordered=True)
    assert not order_free(c) and order_free(u.cascade())
    rects, cand = _detect(c, case["grey"])
    assert len(rects) == 4 and len(cand) != case["n_cand"]  # the changed leaf changes the candidates
    sc = _scanner(case, cascade=c)
    _check_against_separate_calls(sc, sc.scan_raw(case["bgr"]), case["grey"], rects, len(cand))


def _labels(case, rows):
    """name, flag of the existing per-model functions on the same rows."""
    from eigenface import recognize_faces, recognize_faces_dual_model
    dark, light, _ = case["models"]
    one = recognize_faces(rows, dark, THRESHOLD)
    pair = recognize_faces_dual_model(rows, dark, light, THRESHOLD)
    return one, pair


def test_scanner_labels_for_one_model_a_pair_and_a_bank(case):
    from eigenface import decode_keys
    dark, light, third = case["models"]
    grey, rects = case["grey"], [tuple(int(v) for v in r) for r in case["rects"]]
    # one model
    sc = _scanner(case, models=dark)
    got = sc.scan(case["bgr"])
    raw = sc.scan_raw(case["bgr"])
    _, sim = decode_keys(np.ascontiguousarray(raw[2][:4]).reshape(-1), "cosine")
    sim = sim.reshape(4, -1)
    assert np.abs(sim - THRESHOLD).min() > 1e-4  # no flag hangs on the last bits of a similarity
    one, pair = _labels(case, raw[4][:4])
    assert [g[:4] for g in got] == rects
    assert [(g[4], g[6]) for g in got] == [(n, f) for n, _, f in one] == [("dark_person", f) for f in (True, True, False, False)]
    assert [g[5] for g in got] == [float(s) for s in sim[:, 0]]
    # a (dark, light) pair
    sc = _scanner(case, models=(dark, light))
    got = sc.scan(case["bgr"])
    raw = sc.scan_raw(case["bgr"])
    _, sim = decode_keys(np.ascontiguousarray(raw[2][:4]).reshape(-1), "cosine")
    sim = sim.reshape(4, 2)
    assert [(g[4], g[6]) for g in got] == [(n, f) for n, _, f, _, _ in pair]
    assert [g[4] for g in got] == ["dark_person", "dark_person", "light_person", "dark_person"]
    assert [g[6] for g in got] == [True, True, True, False]
    assert [g[5] for g in got] == [float(max(a, b)) for a, b in sim]
    # a bank of three
    sc = _scanner(case)
    got = sc.scan(case["bgr"])
    raw = sc.scan_raw(case["bgr"])
    want = sc.bank.recognize_rows(raw[4], THRESHOLD)[:4]  # all max_faces rows: the same b
    assert [(g[4], g[5], g[6]) for g in got] == [(name, conf, pid != -1) for pid, name, conf in want]
    assert [g[4] for g in got] == ["dark_person", "dark_person", "light_person", "dark_person"]
    assert [g[6] for g in got] == [True, True, True, False]


def test_timer_counts_the_fused_span(case, scanner):
    from eigenface import get_engine
    eng = get_engine(0)
    scanner.scan_raw(case["bgr"])
    eng.timing(True)
    eng.timing_reset()
    try:
        scanner.scan_raw(case["bgr"])
        scanner.scan_raw(case["grey"])
        ms, n = eng.timing_get("haar_scan")
        assert n == 2 and 0 < ms < 1000
        assert eng.timing_get("haar")[1] == 0 and eng.timing_get("ingest")[1] == 0
        assert eng.timing_get("project")[1] == 2 and eng.timing_get("search")[1] == 2
    finally:
        eng.timing(False)
        eng.timing_reset()


def test_states_lifecycle_and_recovery(case):
    """EF_E_STATE without a cascade, without a plan, after a new cascade, with an empty bank and
    with a bank of another d; argument errors; the next good call is correct."""
    from eigenface import EigenfaceError, Engine
    from eigenface.haar import CascadeClassifier
    bgr = case["bgr"]

    def fill(e):
        e.bank_clear()
        for m in case["models"]:
            e.bank_add(m["mean_face"], m["eigenfaces"], m["projected_data"])

    with Engine(0) as e:
        fill(e)
        with pytest.raises(EigenfaceError, match="EF_E_STATE"):  # no cascade
            e.haar_scan_prepare(u.SHAPE, face_size=(u.FACE, u.FACE))
        with pytest.raises(EigenfaceError, match="EF_E_STATE"):
            e.haar_scan_frame(bgr)
        with pytest.raises(EigenfaceError, match="EF_E_STATE"):
            e.haar_scan_info()
        clf = CascadeClassifier(cascade=u.cascade(), engine=e)
        with pytest.raises(EigenfaceError, match="EF_E_STATE"):  # a cascade, no plan
            e.haar_scan_frame(bgr)
        for bad in (dict(min_neighbors=0), dict(max_faces=0), dict(max_faces=4097), dict(max_candidates=0),
                    dict(max_candidates=16385), dict(scale_factor=1.0)):
            with pytest.raises(EigenfaceError, match="EF_E_INVALID"):
                e.haar_scan_prepare(u.SHAPE, face_size=(u.FACE, u.FACE), **bad)
        e.haar_scan_prepare(u.SHAPE, face_size=(u.FACE, u.FACE))
        nl, visitable, mf, mc = e.haar_scan_info()
        assert nl > 3 and visitable > 1611 and (mf, mc) == (8, 4096)
        good = e.haar_scan_frame(bgr)
        np.testing.assert_array_equal(good[1][:4], case["rects"])
        # the separate detector in between rewrites its own tables, not the plan's
        rects, _ = clf.detect(case["grey"][:100, :130], 1.2, 3)
        again = e.haar_scan_frame(bgr)
        for a, b in zip(good[1:], again[1:]):
            np.testing.assert_array_equal(a, b)
        # a new cascade drops the plan: the library refuses real arguments too
        plan = e._haar_scan
        clf.set_cascade(u.cascade(ordered=True))
        assert e._haar_scan is None
        e._haar_scan = plan
        with pytest.raises(EigenfaceError, match="EF_E_STATE"):
            e.haar_scan_frame(bgr)
        clf.set_cascade(u.cascade())
        e.haar_scan_prepare(u.SHAPE, face_size=(u.FACE, u.FACE))
        e.bank_clear()
        with pytest.raises(EigenfaceError, match="EF_E_STATE"):  # empty bank
            e.haar_scan_frame(bgr)
        e.bank_add(np.zeros(100, np.float32), np.zeros((100, 4), np.float32), np.ones((2, 4), np.float32))
        with pytest.raises(EigenfaceError, match="EF_E_STATE"):  # bank d != 32 * 32
            e.haar_scan_frame(bgr)
        fill(e)
        with pytest.raises(EigenfaceError, match="EF_E_INVALID"):  # a row stride below the row's bytes
            e._chk(e._lib.ef_haar_scan_frame(e._h, bgr.ctypes.data, 160, 3, 1, None, good[1].ctypes.data,
                                             good[1].ctypes.data, good[2].ctypes.data, None, None, None, None, 0))
        with pytest.raises(ValueError):
            e.haar_scan_frame(bgr[:100])
        again = e.haar_scan_frame(bgr)
        assert tuple(again[0]) == tuple(good[0])
        for a, b in zip(good[1:], again[1:]):
            np.testing.assert_array_equal(a, b)
