"""Inputs of the Haar frame-scan tests: a BGR frame on which the synthetic cascade finds four
faces, and tiny per-person models in the ``models/*_pca_model.pkl`` layout (useless/scan.py)."""
import numpy as np

from haar_util import synth_cascade, synth_frame

SEED = 3            # synth_cascade(3) on synth_frame(3): 1612 candidates, 4 rectangles at minNeighbors 5
SHAPE = (120, 160)
FACE = 32           # face side: d = 32 * 32
DETECT = dict(scale_factor=1.1, min_neighbors=5, min_size=(30, 30))


def cascade(ordered=False, loose=0.0):
    """The test cascade; ordered: one leaf of 1e-12 makes its stage sum depend on the order of
    adding, so the detector takes the thread-per-window kernel instead of the split one."""
    c = synth_cascade(SEED, loose=loose)
    if ordered:
        thr, stumps = c["stages"][2]
        f, t, _, right = stumps[0]
        stumps[0] = (f, t, float(np.float32(1e-12)), right)
    return c


def bgr_frame():
    """The synthetic grey frame with the blue channel lifted and the red one lowered, so the
    channel order matters to the grey plane."""
    g = synth_frame(SEED, SHAPE).astype(np.int32)
    return np.stack([np.clip(g + 9, 0, 255), g, np.clip(g - 12, 0, 255)], -1).astype(np.uint8)


def pca_model(name, known_rows, seed, n=16):
    """A ``*_pca_model.pkl`` dict trained (plain PCA, all n components) on n face rows: the rows of
    known_rows and random images for the rest.  A known row projects onto its own gallery row."""
    rng = np.random.default_rng(seed)
    d = FACE * FACE
    x = rng.integers(0, 256, (n, d)).astype(np.float64)
    x[:len(known_rows)] = known_rows
    mean = x.mean(0)
    _, _, vt = np.linalg.svd(x - mean, full_matrices=False)
    eig = np.ascontiguousarray(vt.T, dtype=np.float32)  # (d, n); the last direction is numerically null
    mean = mean.astype(np.float32)
    proj = ((x.astype(np.float32) - mean) @ eig).astype(np.float32)
    return {"eigenfaces": eig, "mean_face": mean, "projected_data": proj, "person_name": name,
            "face_dimensions": d, "image_filenames": [f"{name}_{i}.jpg" for i in range(n)]}


def models_for(rows):
    """dark knows faces 0 and 1, light face 2, third none; face 3 is a stranger to all."""
    return [pca_model("dark_person", rows[0:2], 50), pca_model("light_person", rows[2:3], 51),
            pca_model("third_person", rows[0:0], 52)]
