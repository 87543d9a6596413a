"""Synthetic HAAR cascades and frames for the detector tests (no OpenCV cascade file
exists here: haarcascade_frontalface_default.xml ships inside OpenCV, which is absent)."""
import numpy as np


def _third_feature(rng, ww, wh):
    """One feature with a live third rectangle, sum(weight * area) == 0 as in OpenCV's
    cascades.  Families (corners of rect 0 that rect 1 / rect 2 reuse):
      diag    whole 2w x 2h * -1, two opposite quadrants * 2 (either diagonal, either
              order): rect 1 and rect 2 share one corner each with rect 0 — over the four
              variants every corner index occurs for rect 1 and for rect 2;
      inner   4a x 3b * -1, two cells strictly inside * 4 and * 8: no shared corner;
      half    4w x h * -1, its right half * 1 (two corners), an inner quarter * 2 (none);
      same    2w x h * -1 twice (four corners), its right half * 4 (two corners)."""
    fam = ("diag", "inner", "half", "same")[int(rng.integers(0, 4))]
    if fam == "diag":
        w, h = int(rng.integers(1, ww // 2 + 1)), int(rng.integers(1, wh // 2 + 1))
        x, y = int(rng.integers(0, ww - 2 * w + 1)), int(rng.integers(0, wh - 2 * h + 1))
        var = int(rng.integers(0, 4))
        q = [(x, y, w, h, 2.0), (x + w, y + h, w, h, 2.0)] if var < 2 else [(x + w, y, w, h, 2.0), (x, y + h, w, h, 2.0)]
        if var & 1:
            q.reverse()
        return [(x, y, 2 * w, 2 * h, -1.0)] + q
    if fam == "inner":
        a, b = int(rng.integers(1, ww // 4 + 1)), int(rng.integers(1, wh // 3 + 1))
        x, y = int(rng.integers(0, ww - 4 * a + 1)), int(rng.integers(0, wh - 3 * b + 1))
        return [(x, y, 4 * a, 3 * b, -1.0), (x + a, y + b, a, b, 4.0), (x + 2 * a, y + b, a, b, 8.0)]
    if fam == "half":
        w, h = int(rng.integers(1, ww // 4 + 1)), int(rng.integers(2, wh // 2 + 1))
        x, y = int(rng.integers(0, ww - 4 * w + 1)), int(rng.integers(0, wh - h + 1))
        return [(x, y, 4 * w, h, -1.0), (x + 2 * w, y, 2 * w, h, 1.0), (x + w, y, w, h, 2.0)]
    w, h = int(rng.integers(1, ww // 2 + 1)), int(rng.integers(2, wh // 2 + 1))
    x, y = int(rng.integers(0, ww - 2 * w + 1)), int(rng.integers(0, wh - h + 1))
    return [(x, y, 2 * w, h, -1.0), (x, y, 2 * w, h, -1.0), (x + w, y, w, h, 4.0)]


def synth_cascade(seed=0, win=(24, 24), n_feat=40, stages=(3, 5, 7, 9), loose=0.0, third=0.0):
    """Random 2/3-rectangle edge/line features with OpenCV-style weights; stump
    thresholds ~ typical normalised feature values; stage thresholds permissive enough
    that every stage both passes and rejects windows on structured frames.  `third` is
    the share of features replaced by ones with a live third rectangle (_third_feature),
    drawn from a generator of their own: third=0 leaves every seed's cascade as it was.
    `loose` raises every stage threshold, or each stage's by its own entry of a sequence."""
    rng = np.random.default_rng(seed)
    ww, wh = win
    feats = []
    for _ in range(n_feat):
        w = int(rng.integers(2, ww // 2)) * 2 // 2
        h = int(rng.integers(2, wh // 2))
        x = int(rng.integers(0, ww - 2 * w + 1))
        y = int(rng.integers(0, wh - h + 1))
        if rng.random() < 0.5:  # two-rectangle edge feature: whole * -1 + half * 2
            feats.append([(x, y, 2 * w, h, -1.0), (x + w, y, w, h, 2.0)])
        else:  # three-rectangle line feature (x3 weight on the middle third)
            w3 = max(1, (2 * w) // 3)
            feats.append([(x, y, 3 * w3, h, -1.0), (x + w3, y, w3, h, 3.0), (0, 0, 0, 0, 0.0)][:2 + int(rng.random() < 0.3)])
    st = []
    fi = 0
    for si, n in enumerate(stages):
        stumps = []
        for _ in range(n):
            thr = float(np.float32(rng.normal(0.0, 0.02)))
            left, right = float(np.float32(rng.uniform(-1, 0.2))), float(np.float32(rng.uniform(-0.2, 1)))
            stumps.append((fi % n_feat, thr, left, right))
            fi += 1
        st.append((float(np.float32(-0.35 * n + (loose[si] if np.ndim(loose) else loose))), stumps))
    if third > 0:  # that share of the features the stumps use, so each one is evaluated
        rng3 = np.random.default_rng([seed, 3])
        n_used = min(n_feat, fi)
        for i in rng3.choice(n_used, int(np.ceil(third * n_used)), replace=False):
            feats[int(i)] = _third_feature(rng3, ww, wh)
    return {"win": win, "features": feats, "stages": st}


def shared_corners(feat):
    """Per rectangle 1.. of a feature, for each of its corners (x, y), (x + w, y),
    (x, y + h), (x + w, y + h): the index of the equal corner of rectangle 0, or -1 —
    the corner-sharing table the split cascade kernel is given per stump."""
    def corners(r):
        x, y, w, h = r[:4]
        return [(x, y), (x + w, y), (x, y + h), (x + w, y + h)]
    c0 = corners(feat[0])
    return [[c0.index(p) if p in c0 else -1 for p in corners(r)] for r in feat[1:]]


def order_free(c):
    """The detector's rule for summing a stage's leaves in any order (the split kernel):
    with u the smallest float ulp among a stage's nonzero leaves, sum(max |leaf|) <= 2^53 u,
    so every partial sum is an exact double."""
    for _, stumps in c["stages"]:
        lv = np.array([[np.float32(l), np.float32(r)] for _, _, l, r in stumps], np.float64)
        nz = np.abs(lv[lv != 0])
        if not np.isfinite(lv).all():
            return False
        if nz.size and np.abs(lv).max(1).sum() > np.ldexp(1.0, 53) * np.ldexp(1.0, np.frexp(nz)[1] - 24).min():
            return False
    return True


def long_stage_cascade(seed=0, win=(24, 24), n_long=300, n_feat=40):
    """Stages of 3, n_long and 5 stumps; the long one reuses the features round-robin (more
    stumps than the 256 records the split kernel stages into LDS at a time).  Its threshold
    is the sum of its leaves' midpoints, near the median stage sum (the -0.35 n rule of
    synth_cascade would pass every window at this length)."""
    c = synth_cascade(seed, win, n_feat, stages=(3, n_long, 5), third=0.25)
    _, stumps = c["stages"][1]
    c["stages"][1] = (float(np.float32(sum(0.5 * (np.float32(l) + np.float32(r)) for _, _, l, r in stumps))), stumps)
    return c


def walk_cascade(win=(24, 24)):
    """One stage, one stump, feature value p(x + 1, y) - p(x, y) of the window origin:
    the window passes exactly when its second pixel is the brighter one."""
    return {"win": win, "features": [[(0, 0, 2, 1, -1.0), (1, 0, 1, 1, 2.0)]], "stages": [(0.0, [(0, 0.0, -1.0, 1.0)])]}


def walk_frame(bits, win=(24, 24), seed=0):
    """Frame on which walk_cascade's stage-0 result at scale 1 (step 2) is bits[r, i] (1 pass,
    0 reject) for the window at x = 2 i, y = 2 r: every visited origin has its own pixel
    pair.  Uniform noise in 40..215 everywhere keeps each window's deviation far above the
    variance gate.  Detect with minSize = maxSize = win, so only that layer exists."""
    bits = np.asarray(bits).astype(bool)
    rows, npos = bits.shape
    ww, wh = win
    rng = np.random.default_rng(seed)
    f = rng.integers(40, 216, (2 * (rows - 1) + wh, 2 * (npos - 1) + ww)).astype(np.uint8)
    lo = rng.integers(40, 128, bits.shape).astype(np.uint8)
    hi = rng.integers(128, 216, bits.shape).astype(np.uint8)
    f[0:2 * rows:2, 0:2 * npos:2] = np.where(bits, lo, hi)
    f[0:2 * rows:2, 1:2 * npos:2] = np.where(bits, hi, lo)
    return f


def walk_expected(bits, win=(24, 24)):
    """The invoker's sequential walk over bits: a rejected position skips the next one."""
    out = []
    for r, row in enumerate(np.asarray(bits).astype(bool)):
        i = 0
        while i < len(row):
            if row[i]:
                out.append((2 * i, 2 * r, win[0], win[1]))
            i += 1 if row[i] else 2
    return out


def directed_walk_rows(npos, seed=0):
    """Reject/pass rows (1 pass, 0 reject) that force the scan walk's carries between
    chunks of 64 positions: constant and alternating rows, single rejects and a pair at
    63/64, reject runs of every length 1..70 from even and from odd starts placed at
    position 63/64 and at 127/128 (every length 3..70 of either parity lies across the edge;
    an even start of length 1 or 2 ends on it), a run over 61..130, a rejected last position,
    and random rows.  Patterns are cut to npos positions; those wholly outside are left out."""
    rng = np.random.default_rng(seed)
    rows = []

    def rejects(*spans):
        row = np.ones(npos, bool)
        for a, b in spans:
            row[a:b] = False
        return row

    rows += [np.zeros(npos, bool), np.ones(npos, bool), np.arange(npos) % 2 == 1, np.arange(npos) % 2 == 0]
    rows += [rejects((63, 64)), rejects((64, 65)), rejects((63, 65)), rejects((61, 131)), rejects((npos - 1, npos))]
    for edge in (64, 128):
        for parity in (0, 1):
            for n in range(1, 71):
                a = edge - (n + 1) // 2  # the run straddles the chunk edge (from 3 positions on)
                if a % 2 != parity:
                    a += 1 if a + 1 < edge else -1
                if max(a, 0) < npos:
                    rows.append(rejects((max(a, 0), a + n)))
    rows += [rng.random(npos) >= d for d in (0.1, 0.5, 0.9)]
    return np.array(rows)


def walk_rows_for_count(nrows, npos=200):
    """nrows rows for the row-count tests, chosen so that a lost row shows.  The first is
    the random row of density 0.5 with reject runs written across 63/64 and 127/128, the
    last the random row of density 0.1: both emit windows from every chunk and skip in every
    chunk.  Between them the run over 61..130, then directed_walk_rows' run rows, spread."""
    rows = directed_walk_rows(npos)
    first = rows[-2].copy()
    first[62:66] = first[125:130] = False
    mid = [7] * (nrows > 2) + list(np.linspace(9, len(rows) - 4, max(nrows - 3, 0)).astype(int))
    return np.concatenate([first[None], rows[mid], rows[-3:-2][:nrows > 1]])


def synth_frame(seed=0, shape=(120, 160)):
    """Grey frame with smooth background, bright/dark boxes and noise (structure for the
    features, flat patches for the variance rejection)."""
    rng = np.random.default_rng(seed)
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    f = 90 + 40 * np.sin(xx / 17.0) * np.cos(yy / 23.0)
    for _ in range(8):
        y0, x0 = rng.integers(0, H - 20), rng.integers(0, W - 20)
        h, w = rng.integers(10, 40), rng.integers(10, 40)
        f[y0:y0 + h, x0:x0 + w] += rng.uniform(-60, 60)
    f += rng.normal(0, 6, f.shape)
    f[: H // 6, : W // 6] = 128  # flat corner: low-variance windows
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def cascade_xml(c):
    """Write a cascade dict in OpenCV's opencv-cascade-classifier XML layout."""
    ww, wh = c["win"]
    out = ['<?xml version="1.0"?>', "<opencv_storage>", '<cascade type_id="opencv-cascade-classifier">',
           "<stageType>BOOST</stageType>", "<featureType>HAAR</featureType>", f"<height>{wh}</height>",
           f"<width>{ww}</width>", f"<stageNum>{len(c['stages'])}</stageNum>", "<stages>"]
    for thr, stumps in c["stages"]:
        out += ["<_>", f"<maxWeakCount>{len(stumps)}</maxWeakCount>", f"<stageThreshold>{thr!r}</stageThreshold>",
                "<weakClassifiers>"]
        for fi, t, l, r in stumps:
            out.append(f"<_><internalNodes>\n 0 -1 {fi} {t!r}</internalNodes><leafValues>\n {l!r} {r!r}</leafValues></_>")
        out += ["</weakClassifiers>", "</_>"]
    out += ["</stages>", "<features>"]
    for f in c["features"]:
        out.append("<_><rects>" + "".join(f"<_>\n {x} {y} {w} {h} {wt!r}</_>" for x, y, w, h, wt in f) + "</rects></_>")
    out += ["</features>", "</cascade>", "</opencv_storage>"]
    return "\n".join(out)


def stage_census(layer, c):
    """(variance rejects, rejects per stage, windows passing every stage) of the oracle's
    eval_layer over every origin of one layer.  eval_layer codes a stage-1 reject as -1 like
    a variance reject; a one-stump cascade that passes everything tells them apart."""
    from oracle import haar_oracle as ho
    res = ho.eval_layer(layer, c)
    lowvar = ho.eval_layer(layer, {"win": c["win"], "features": c["features"],
                                   "stages": [(-1e30, c["stages"][0][1][:1])]}) == -1
    rej = [int((res == 0).sum()), int(((res == -1) & ~lowvar).sum())]
    rej += [int((res == -s).sum()) for s in range(2, len(c["stages"]))]
    return int(lowvar.sum()), rej[:len(c["stages"])], int((res == 1).sum())


# ---------------------------------------------------------------- shared test inputs
# Seeds and `loose` values were searched on the CPU so that, on the scale-1 layer, every
# stage rejects windows that reached it, windows pass every stage and the variance gate
# rejects some (tests/test_haar_cpu.py asserts it for each pair).
THIRD_WINS = [(24, 24), (20, 20), (18, 30), (32, 16)]
# the stage groups are 1-3, 4-7, 8-13, 14-: one stage launches no group, the others end a
# cascade on a group's last stage or one stage into the next group
STAGE_COUNTS = (1, 2, 4, 5, 8, 9, 14, 15)
# per stage, so that about a fifth of the windows reaching a stage is rejected by it (one
# value for all stages leaves some of fifteen stages rejecting nothing, at every seed tried)
_STAGE_LOOSE = [1.27, 2.53, 3.47, 3.06, 5.7, 5.27, 4.0, 7.34, 13.08, 9.34, 9.72, 16.25, 12.23, 10.73, 19.36]


def third_case(win):
    """Half of the features with a live third rectangle, on a 100 x 330 frame."""
    return synth_cascade(11, win=win, third=0.5, loose=0.6), synth_frame(11, (100, 330))


def stage_count_case(n):
    """The first n stages (3, 5, 7, ... stumps) of one cascade, on a 96 x 128 frame."""
    c = synth_cascade(20, n_feat=60, stages=tuple(range(3, 33, 2)), third=0.25, loose=_STAGE_LOOSE)
    c["stages"] = c["stages"][:n]
    return c, synth_frame(20, (96, 128))


def long_stage_case():
    return long_stage_cascade(0), synth_frame(0, (96, 128))


def wide_case():
    """The standard cascade on a 640-wide frame: its step-1 layers (scale >= 2) have rows
    of more than 256 positions, five chunks of the scan walk."""
    return synth_cascade(39), synth_frame(39, (80, 640))


def bright_case():
    """A 300 x 420 frame lifted by 110 grey levels: the sum of squares of the frame, and of
    its first pyramid layers, passes 2^32, so the uint32 integral of squares wraps."""
    f = synth_frame(39, (300, 420)).astype(np.int32) + 110
    return synth_cascade(39), np.clip(f, 0, 255).astype(np.uint8)


BRIGHT_FINE = (1.03, (0, 0), (27, 27))  # scale factor, minSize, maxSize: five near-full-size layers
