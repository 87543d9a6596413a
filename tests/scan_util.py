"""Test helpers of the frame scanner: the live loop's host rules (scan-template-v4.py:351-401)
restated without any product code, and tiny trained models."""
from oracle import eigenface_oracle as orc
from oracle import image_oracle as io

FACE_AREA_CAP = 200 * 200  # the area at which the size term of the selection score saturates


def selection_scores(detections, pca_results):
    """The selection score of every detection of a frame (scan-template-v4.py:363-369): half the
    rectangle's area as a fraction of FACE_AREA_CAP (at most 1), half the PCA confidence."""
    return [0.5 * min(d["width"] * d["height"] / FACE_AREA_CAP, 1.0) + 0.5 * r[2]
            for d, r in zip(detections, pca_results)]


def kept(detections, pca_results):
    """Indices of the detections the loop reports (:351-377): all of a frame with at most one,
    else the single best selection score, the earliest among equals."""
    if len(detections) <= 1:
        return list(range(len(detections)))
    scores = selection_scores(detections, pca_results)
    return [scores.index(max(scores))]


def verdict(template_name, template_conf, pca_name, pca_conf):
    """(reported name, final confidence) of one detection (:393-401).  The template's answer
    stands when the PCA agrees with it or is weak (< 0.5), else the PCA's does; either way the
    name is withheld unless the PCA reaches 0.8 and the template 0.7."""
    trust_template = pca_name == template_name or pca_conf < 0.5
    name, conf = (template_name, template_conf) if trust_template else (pca_name, pca_conf)
    confident = pca_conf >= 0.8 and template_conf >= 0.7
    return (name if confident else "unknown"), conf


def records_from_lists(detections, pca_results):
    """The result records of one frame (:413-420, without frame_number) for the detections of
    io.template_match_all_models and, parallel to them, the (person_id, name, confidence)
    tuples recognize_face_all_models gives for their crops."""
    out = []
    for i in kept(detections, pca_results):
        d, (_, pca_name, pca_conf) = detections[i], pca_results[i]
        name, final = verdict(d["person_name"], d["confidence"], pca_name, pca_conf)
        out.append({"person_name": name, "template_confidence": d["confidence"], "pca_confidence": pca_conf,
                    "final_confidence": final, "x": d["x"], "y": d["y"], "width": d["width"],
                    "height": d["height"]})
    return out


def in_corner(x, y, w, h, frame_width, frame_height):
    return io.is_detection_in_corner({"x": x, "y": y, "width": w, "height": h}, frame_width, frame_height)


def trained(person, n, seed):
    """(pixel rows, model dict) of a tiny 64 x 64 model, as tests/test_gpu_bank.py::_trained."""
    from eigenface.compat import FaceTrainer
    x, _ = orc.synth_faces(n, 64, r=32, seed=seed)
    tr = FaceTrainer()
    tr.face_images = x
    tr.face_info = [{"face_id": i} for i in range(n)]
    tr.assign_labels_interactive(person)
    assert tr.train_pca_model()
    return x, tr.model_dict()
