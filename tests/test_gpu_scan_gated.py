"""Gated frame scan (ef_scan_frame_gated, FrameScanner(face_gate=...)): everything but the choice
over models equals ef_scan_frame bit for bit, the gate's outputs equal the bank's own gated call on
the returned rows, and a template-matched patch that is no face comes out as "unknown"."""
import numpy as np
import pytest

import scan_util
from oracle import image_oracle as io

pytestmark = pytest.mark.gpu

PERSONS = ["alice", "bob", "carol"]


@pytest.fixture(scope="module")
def case():
    """The frame of tests/test_gpu_scan_frame.py: uniform noise, alice's first template cut from its
    grey, so the localiser finds alice at (90, 60) and the crop it hands to the bank is noise: a
    planted non-face.  Three tiny trained models."""
    rng = np.random.default_rng(12)
    bgr = rng.integers(0, 256, (180, 240, 3), dtype=np.uint8)
    grey = io.bgr2gray(bgr)
    templates = {
        "alice": [grey[60:100, 90:125].copy(), rng.integers(0, 256, (30, 30), dtype=np.uint8)],
        "bob": [rng.integers(0, 256, (25, 40), dtype=np.uint8)],
        "carol": [grey[2:40, 3:40].copy()],
    }
    models, faces = {}, {}
    for i, (p, n) in enumerate(zip(PERSONS, (60, 56, 52))):
        faces[p], md = scan_util.trained(p, n, 40 + i)
        models[p] = {"model_data": md, "template_images": [{"image": t} for t in templates[p]],
                     "detection_data": {"faces": [{}]}}
    return {"frame": bgr, "models": models, "faces": faces}


def _bytes(a):
    return a.view(np.uint8) if a.dtype.names else a


def test_gated_scan_equals_the_plain_scan_and_the_bank_s_gated_call(case):
    import torch
    from eigenface import FrameScanner, get_engine
    frame = case["frame"]
    plain = FrameScanner(case["models"], (180, 240)).scan_raw(frame)
    sc = FrameScanner(case["models"], (180, 240), face_gate=0.1)
    dets, keys, best, rows, eps2, energy = sc.scan_raw(frame)
    assert eps2.shape == (3, 3) and energy.shape == (3, 3) and eps2.dtype == np.float32
    assert int(dets["found"][0]) == 1 and (int(dets["x"][0]), int(dets["y"][0])) == (90, 60)
    for a, b in zip(plain, (dets, keys, best, rows)):
        if a is not plain[2]:  # everything but the best slots, which the gate may change
            np.testing.assert_array_equal(_bytes(a), _bytes(b))
    # the bank's own gated call on the returned rows, the same b
    eng = get_engine(0)
    for gate, relative in ((sc.bank.gate, True), (np.full(3, np.inf, np.float32), True),
                           (np.array([5e5, np.inf, 1.0], np.float32), False)):
        d2, k2, b2, r2, e2, n2 = eng.scan_frame_gated(frame, gate, "cosine", relative=relative)
        kk, _, bb, _, ee, nn = eng.bank_recognize_gated_raw(r2, gate, "cosine", relative=relative)
        np.testing.assert_array_equal(_bytes(d2), _bytes(dets))
        np.testing.assert_array_equal(r2, rows)
        np.testing.assert_array_equal(k2, kk)
        np.testing.assert_array_equal(k2, keys)
        np.testing.assert_array_equal(b2, bb)
        np.testing.assert_array_equal(e2, ee)
        np.testing.assert_array_equal(n2, nn)
        np.testing.assert_array_equal(e2, eps2)
        if not np.isfinite(gate).any():
            np.testing.assert_array_equal(b2, plain[2])  # nothing gated: ef_scan_frame's choice
    # the plain call still answers as before with the gate's state resident
    for a, b in zip(plain, eng.scan_frame(frame, "cosine")):
        np.testing.assert_array_equal(_bytes(a), _bytes(b))
    # device tensors: nothing waits on the host
    out = eng.scan_frame_gated(torch.as_tensor(frame, device="cuda"), torch.as_tensor(sc.bank.gate, device="cuda"))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[0].cpu().numpy().reshape(-1), dets.view(np.int32).reshape(-1))
    for got, want in zip(out[1:], (keys, best, rows, eps2, energy)):
        np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_device_form_without_the_optional_outputs(case):
    """ef_scan_frame_gated on device pointers with best_slot, rows and energy left out (the rows and
    the energy then live in the plan's result block): dets, keys and dffs2 are byte for byte those of
    the call that is given every output, and those of the host form."""
    import torch
    from eigenface import FrameScanner, _native as N
    sc = FrameScanner(case["models"], (180, 240), face_gate=0.1)
    host = sc.scan_raw(case["frame"])
    eng = sc._prepare()
    G, M, d = 3, 3, 64 * 64
    frame = torch.as_tensor(case["frame"], device="cuda")
    gate = torch.as_tensor(sc.bank.gate, device="cuda")

    def ptr(t):
        return None if t is None else t.data_ptr()

    def call(optional):
        t = {"device": "cuda"}
        dets = torch.zeros((G, 8), dtype=torch.int32, **t)
        keys = torch.zeros((G, M), dtype=torch.int64, **t)
        eps = torch.zeros((G, M), dtype=torch.float32, **t)
        best = torch.zeros(G, dtype=torch.int32, **t) if optional else None
        rows = torch.zeros((G, d), dtype=torch.uint8, **t) if optional else None
        en = torch.zeros((G, M), dtype=torch.float32, **t) if optional else None
        with eng._torch_order(frame, gate, dets, keys, eps, best, rows, en):
            eng._chk(eng._lib.ef_scan_frame_gated(eng._h, frame.data_ptr(), 240 * 3, 3, N.EF_METRIC_COSINE, ptr(gate),
                                                  ptr(dets), ptr(keys), ptr(best), ptr(rows), ptr(eps), ptr(en),
                                                  N.EF_BANK_GATE_RELATIVE | N.EF_MEM_DEVICE))
        torch.cuda.synchronize()
        return [None if a is None else a.cpu().numpy() for a in (dets, keys, best, rows, eps, en)]

    bare, full = call(False), call(True)
    for i in (0, 1, 4):
        np.testing.assert_array_equal(bare[i].view(np.uint8), full[i].view(np.uint8))
    np.testing.assert_array_equal(full[0].reshape(-1), host[0].view(np.int32).reshape(-1))
    for got, want in zip(full[1:], host[1:]):
        np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))


def test_a_matched_patch_that_is_no_face_is_unknown(case):
    from eigenface import FrameScanner
    frame = case["frame"]
    plain = FrameScanner(case["models"], (180, 240))
    want_plain = plain.scan_frame(frame)
    dd, pp = plain.scan(frame)
    assert len(want_plain) == 1 and [d["person_name"] for d in dd] == ["alice"]
    gated = FrameScanner(case["models"], (180, 240), face_gate=0.1)
    # the crop is noise: no model's face space explains a tenth of its energy away
    _, _, best, rows, eps2, energy = gated.scan_raw(frame)
    assert np.all(eps2[0] > 0.4 * energy[0]), eps2[0] / energy[0]
    assert best[0] == -1
    dets, labels = gated.scan(frame)
    assert dets == dd and labels == [(-1, "unknown", 0.0)]
    got = gated.scan_frame(frame)
    assert got == scan_util.records_from_lists(dets, labels)
    assert got[0]["person_name"] == "unknown" and got[0]["pca_confidence"] == 0.0
    assert {k: got[0][k] for k in ("x", "y", "width", "height", "template_confidence")} == \
        {k: want_plain[0][k] for k in ("x", "y", "width", "height", "template_confidence")}
    # a face the model was trained on keeps its label under a gate.  The tiny models explain such a
    # face to about 5 % of its energy, so this part uses a bound of 0.25: the face a factor 4 inside
    # it, the noise crop (at most all of its energy is unexplained) a factor 3 outside, both asserted
    # on fp64 before the gated calls
    import recon_util as ru
    from eigenface import ModelBank
    from eigenface.bank import _operands
    from eigenface.pca import reconstruction_operands
    mu, w, comps, scale = _operands(case["models"]["alice"]["model_data"])
    R, s = reconstruction_operands(comps, scale)
    two = np.stack([case["faces"]["alice"][5], rows[0]])
    r = ru.residual_ref(two, ru.centred_ref(two, mu) @ ru.f64(w), R, mu, s)
    ratio = (r * r).sum(axis=1) / (ru.centred_ref(two, mu, s) ** 2).sum(axis=1)
    print(f"fp64 eps2 / E under alice's model: a training face {ratio[0]:.3g}, the noise crop {ratio[1]:.3g}")
    assert ratio[0] < 0.25 / 4 and ratio[1] > 0.25 * 3
    wide = ModelBank(case["models"], face_gate={"alice": 0.25})
    assert wide.is_face(two).tolist() == [True, False]
    got_rows = wide.recognize_rows(two)
    want_rows = plain.bank.recognize_rows(two)
    assert got_rows[0] == want_rows[0] and got_rows[0][1] == "alice"
    # and face_gate=None gives the parent's record again
    assert FrameScanner(case["models"], (180, 240)).scan_frame(frame) == want_plain
