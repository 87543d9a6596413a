"""Range search: every gallery row within a threshold of each probe.

``Engine.search`` answers "which row is nearest", ``search_topk`` "which m <= 64 rows are nearest".
An enrolment desk, a watch-list or a de-duplication job asks another question: for each of these
new faces, which gallery rows lie within the threshold, all of them (scikit-learn's
``radius_neighbors``, faiss's ``range_search``).  ``Engine.search_range`` / ``radius_neighbors``
answer it on the GPU (``ef_search_range``: the census's distance GEMM with an epilogue that decides
every membership as in fp64 and writes a CSR list in ascending row order, the same bytes on every
run).

The threshold is the one ``equal_error_threshold`` / ``pair_equal_error`` give on labelled data: a
squared L2 distance (a hit at or below it) or a cosine similarity (a hit at or above it).

``merge_range`` joins the results of row shards, ``label_votes`` is the k-NN vote over a probe's
hits; both run on the host.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native as N


def _np(x):
    """A host array of a NumPy array or a device tensor (the latter waits for the device)."""
    return x.cpu().numpy() if hasattr(x, "data_ptr") else np.asarray(x)


@dataclass
class RangeResult:
    """Outcome of ``Engine.search_range``: probe p's hits are entries ``lims[p] .. lims[p + 1] - 1``
    of ``rows`` (int64 global row indices, ascending inside a segment) and ``scores`` (float32:
    squared L2 distance or cosine similarity).  ``lims`` int64 (b + 1,) is always exact, whatever
    the capacity; a segment is written only when it fits whole (``lims[p + 1] <= capacity``).
    ``info`` int64 (4,): hits, pairs settled in fp64, hits not written, 0.  The members are NumPy
    arrays, or device tensors when the probes were (``host()`` copies them)."""

    lims: object
    rows: object
    scores: object
    info: object
    metric: str
    capacity: int

    @property
    def on_device(self):
        return hasattr(self.lims, "data_ptr")

    @property
    def n_probes(self):
        return int(self.lims.shape[0]) - 1

    @property
    def counts(self):
        """Hits per probe, int64 (b,)."""
        return self.lims[1:] - self.lims[:-1]

    @property
    def complete(self):
        """Whether every segment was written: ``lims[-1] <= capacity``.  None for a device result,
        where knowing it means waiting for the device: ``host().complete`` does."""
        if self.on_device:
            return None
        return bool(self.lims[-1] <= self.capacity)

    def host(self):
        """The same result as NumPy arrays (waits for the device when the members are tensors);
        rows / scores cut to the written prefix."""
        lims, info = _np(self.lims), _np(self.info)
        written = _written(lims, self.capacity)
        return RangeResult(lims, _np(self.rows)[:written], _np(self.scores)[:written], info, self.metric,
                           self.capacity)

    def of(self, i):
        """(rows, scores) of probe i."""
        lo, hi = int(self.lims[i]), int(self.lims[i + 1])
        if hi > self.capacity:
            raise ValueError(f"probe {i}'s segment ends at {hi}, past the capacity {self.capacity}: it was not written")
        return self.rows[lo:hi], self.scores[lo:hi]

    def pairs(self):
        """(probe, row, score) of every written hit, as host arrays in segment order."""
        r = self.host() if self.on_device else self
        written = _written(r.lims, r.capacity)
        probe = np.repeat(np.arange(r.n_probes, dtype=np.int64), np.diff(r.lims))[:written]
        return probe, r.rows[:written], r.scores[:written]

    def by_score(self):
        """A host copy with each written segment re-ordered best first (lowest distance, highest
        similarity), ties by row."""
        r = self.host() if self.on_device else self
        probe, rows, scores = r.pairs()
        key = scores if r.metric == "l2" else -scores
        order = np.lexsort((rows, key, probe))
        return RangeResult(r.lims, rows[order], scores[order], r.info, r.metric, r.capacity)


def _written(lims, capacity):
    """Entries of rows / scores that were written: the segments that fit are a prefix."""
    fit = lims[lims <= capacity]
    return int(fit[-1]) if fit.size else 0


def radius_neighbors(G, Q, threshold, metric="l2", exclude_rows=None, device=0, engine=None):
    """All rows of the gallery ``G`` (n, k) within ``threshold`` of each probe of ``Q`` (b, k), as
    a complete RangeResult.  ``engine``: an ``Engine`` whose resident gallery is replaced by G (G
    None: the gallery it already holds is searched); otherwise the pooled engine of ``device``."""
    if engine is None:
        from .pca import get_engine
        engine = get_engine(device, pool="neighbors")
    if G is not None:
        engine.set_gallery(np.ascontiguousarray(G, dtype=np.float32))
    return engine.search_range(Q, threshold, metric, exclude_rows)


def merge_range(parts):
    """Per-probe concatenation of the complete RangeResults of row shards, given in ascending
    global-offset order (each shard searched on an engine of its own with ``global_offset`` set):
    the merged segments stay ascending.  Runs on the host."""
    parts = [p.host() if p.on_device else p for p in parts]
    if not parts:
        raise ValueError("merge_range needs at least one part")
    b, metric = parts[0].n_probes, parts[0].metric
    for p in parts:
        if p.n_probes != b or p.metric != metric:
            raise ValueError("the parts must hold the same probes under the same metric")
        if not p.complete:
            raise ValueError("a part is incomplete (lims[-1] > capacity): search it again with enough capacity")
    counts = np.stack([np.diff(p.lims) for p in parts])  # (parts, b)
    lims = np.zeros(b + 1, np.int64)
    np.cumsum(counts.sum(axis=0), out=lims[1:])
    total = int(lims[-1])
    rows, scores = np.empty(total, np.int64), np.empty(total, np.float32)
    start = lims[:-1].copy()  # where the next part's hits of each probe go
    for p, c in zip(parts, counts):
        # entry i of the part belongs to probe pr[i] and is number i - lims[pr[i]] of its segment
        pr = np.repeat(np.arange(b, dtype=np.int64), c)
        dst = start[pr] + (np.arange(pr.shape[0], dtype=np.int64) - p.lims[:-1][pr])
        rows[dst] = p.rows[:pr.shape[0]]
        scores[dst] = p.scores[:pr.shape[0]]
        start += c
    for a, z in zip(parts[:-1], parts[1:]):
        if a.rows.size and z.rows.size and a.rows.max() >= z.rows.min():
            raise ValueError("the parts are not in ascending global-offset order")
    info = np.sum([p.info for p in parts], axis=0).astype(np.int64)
    return RangeResult(lims, rows, scores, info, metric, total)


def label_votes(result, gallery_labels):
    """The k-NN vote over each probe's hits: ``(label, votes, hits)``, int64 (b,) each: the label
    with the most hits, its vote count and the probe's hit count.  A tie goes to the label of the
    best-scoring hit among the tied labels (then to the lower row); a probe without hits gets
    label -1 and 0 votes.  ``gallery_labels``: one integer label per GLOBAL row index."""
    r = result.host() if result.on_device else result
    if not r.complete:
        raise ValueError("the result is incomplete (lims[-1] > capacity)")
    lab = np.asarray(gallery_labels).astype(np.int64)
    b = r.n_probes
    out_label, out_votes = np.full(b, -1, np.int64), np.zeros(b, np.int64)
    hits = np.diff(r.lims).astype(np.int64)
    best = r.by_score()
    for p in np.flatnonzero(hits):
        rows = best.rows[best.lims[p]:best.lims[p + 1]]  # best first
        labels, first, votes = np.unique(lab[rows], return_index=True, return_counts=True)
        tied = np.flatnonzero(votes == votes.max())
        w = tied[np.argmin(first[tied])]  # the tied label whose first (best) hit comes earliest
        out_label[p], out_votes[p] = labels[w], votes[w]
    return out_label, out_votes, hits


def search_range_plan(b, n, kp):
    """ef_search_range_plan (host only): ``(n_chunks, tiles_per_item)`` of a range search with b
    probes over n rows of padded length kp: the gallery's 128-row tiles are cut into n_chunks
    chunks of tiles_per_item tiles, and a work item is one chunk against 128 probes."""
    import ctypes as C
    nc, tpi = C.c_int64(0), C.c_int64(0)
    rc = N.lib().ef_search_range_plan(int(b), int(n), int(kp), C.byref(nc), C.byref(tpi))
    if rc != N.EF_OK:
        raise N.EigenfaceError(rc, "ef_search_range_plan: bad arguments")
    return int(nc.value), int(tpi.value)
