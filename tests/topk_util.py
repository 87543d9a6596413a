"""What the top-m search guarantees (include/eigenface.h ef_search_topk), as an fp64 checker
in numpy.

Per probe the engine returns m slots, best first: rank 0 is ef_search's answer (the lowest
row within the 1e-12 tie window of the minimum), ranks 1.. are the other rows in (fp64
score, row) order, rows are distinct, and slots past the gallery's rows are empty.

The checker scores every (probe, row) pair in fp64 as parity_util.top2 does (expanded form;
its own evaluation error is ~1e-15 of the scale, 1000x below the window, which the 1.1x
margin absorbs) and orders them with np.lexsort's rule (score, then row).  The chosen rows
are re-scored in the difference form of parity_util.chosen_scores.
"""
import numpy as np

from oracle import eigenface_oracle as orc
from parity_util import MARGIN, WINDOW, gmax2_of

M_MAX = 64


class Reference:
    """The M_MAX best (score, row) per probe in lexsort order, computed once per
    (probes, gallery, metric) and shared by every m / scan option checked against it."""

    def __init__(self, q, g, metric, ranks=M_MAX):
        self.metric = metric
        self.q64 = np.asarray(q, np.float64)
        self.g = np.asarray(g)
        b, n = len(self.q64), len(self.g)
        self.n = n
        qn2 = (self.q64 ** 2).sum(1)
        self.scale = qn2 + gmax2_of(self.g) if metric == "l2" else np.ones(b)
        keep = min(ranks + 1, n)  # one more: the neighbour after the last rank
        if n == 0:
            self.rows = np.zeros((b, 0), np.int64)
            self.scores = np.zeros((b, 0))
            return
        g64 = self.g.astype(np.float64)
        if metric == "l2":
            s = qn2[:, None] + (g64 ** 2).sum(1)[None, :] - 2.0 * (self.q64 @ g64.T)
        else:
            s = -(orc._unit_rows(self.q64) @ orc._unit_rows(g64).T)
        order = np.argsort(s, axis=1, kind="stable")[:, :keep]  # stable: ties by row = lexsort
        self.rows = order
        self.scores = np.take_along_axis(s, order, axis=1)

    def window(self, at):
        """The engine's tie window at score(s) `at` (b, ...), in the checker's units."""
        sc = self.scale.reshape((-1,) + (1,) * (np.ndim(at) - 1))
        return WINDOW * (np.abs(at) + sc)

    def chosen(self, idx):
        """fp64 scores (difference form) of rows idx (b, j)."""
        gi = self.g[idx].astype(np.float64)
        if self.metric == "l2":
            return ((self.q64[:, None, :] - gi) ** 2).sum(-1)
        uq = orc._unit_rows(self.q64)
        ug = orc._unit_rows(gi.reshape(-1, gi.shape[-1])).reshape(gi.shape)
        return -(uq[:, None, :] * ug).sum(-1)

    def clear(self, m):
        """(b, min(m, n)) mask: the rank's score is separated from both neighbours by more
        than the window, so the checker alone fixes its row."""
        nv = min(m, self.n)
        s = self.scores
        b = len(s)
        pad = np.concatenate([np.full((b, 1), -np.inf), s, np.full((b, 1), np.inf)], axis=1)
        w = MARGIN * self.window(s[:, :nv])
        return ((pad[:, 1:nv + 1] - pad[:, :nv]) > w) & ((pad[:, 2:nv + 2] - pad[:, 1:nv + 1]) > w)


def check_topk(ref, m, idx, best=None, records=None):
    """Assert the contract for one result: idx (b, m) rows (-1 = empty slot), optional decoded
    fp32 scores best (b, m) and optional match records (b, m) of N.MATCH_DTYPE with LOCAL row
    keys.  Returns the clear mask (b, min(m, n))."""
    idx = np.asarray(idx)
    b = len(ref.q64)
    assert idx.shape == (b, m), idx.shape
    nv = min(m, ref.n)
    # empty slots exactly where the gallery runs out
    assert (idx[:, nv:] == -1).all(), "slots past the gallery's rows must be empty"
    if best is not None:
        assert np.isnan(np.asarray(best)[:, nv:]).all()
    if nv == 0:
        return np.zeros((b, 0), bool)
    got = idx[:, :nv]
    assert ((got >= 0) & (got < ref.n)).all(), "row out of range"
    srt = np.sort(got, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "rows of one probe must be distinct"
    want_s = ref.scores[:, :nv]
    mine = ref.chosen(got)
    w = MARGIN * ref.window(want_s)
    bad = ~(np.abs(mine - want_s) <= w)
    assert not bad.any(), f"{ref.metric} m={m}: {bad.sum()} ranks are outside the tie window of the rank's " \
                          f"fp64 score (first {np.argwhere(bad)[:3].tolist()})"
    clear = ref.clear(m)
    miss = clear & (got != ref.rows[:, :nv])
    assert not miss.any(), f"{ref.metric} m={m}: {miss.sum()} of {clear.sum()} clear ranks differ from the fp64 " \
                           f"lexsort (first {np.argwhere(miss)[:3].tolist()})"
    # duplicate rows (bitwise equal neighbouring scores): ascending index
    dup = want_s[:, 1:] == want_s[:, :-1]
    assert (got[:, 1:][dup] > got[:, :-1][dup]).all(), "equal scores must come out in ascending row order"
    if best is not None:
        val = mine if ref.metric == "l2" else -mine
        v32 = val.astype(np.float32)
        got32 = np.asarray(best, np.float32)[:, :nv]
        assert (np.abs(got32 - v32) <= 2 * np.spacing(np.abs(v32))).all(), "decoded scores beyond 2 fp32 ulps"
    if records is not None:
        rec = np.asarray(records)
        assert rec.shape == (b, m)
        assert ((rec["key"][:, :nv] & 0xFFFFFFFF) == got).all()
        assert (np.abs(rec["score"][:, :nv] - mine) <= 1e-12 * ref.scale[:, None]).all(), "record scores"
        assert np.isinf(rec["score"][:, nv:]).all() and (rec["key"][:, nv:] == np.iinfo(np.int64).max).all()
    return clear
