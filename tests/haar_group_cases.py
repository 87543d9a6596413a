"""Written rectangle lists for the grouping tests (ef_haar_group against
oracle/haar_oracle.group_rectangles), with the check that each one reaches the branch of the
oracle it is written for.  20 x 20 rectangles are similar up to 4 pixels apart (eps = 0.2)."""
import numpy as np

from oracle import haar_oracle as ho


def _sq(x, y=0, s=20):
    return (x, y, s, s)


# name -> (rectangles in list order, min_neighbors)
CASES = {
    # A ~ B ~ C with A !~ C: one class of three
    "chain": ([_sq(0), _sq(4), _sq(8)], 2),
    # four separate rectangles that later members of the list join into one class
    "late_join": ([_sq(0), _sq(8), _sq(16), _sq(24), _sq(4), _sq(12), _sq(20)], 2),
    # three classes whose first members come in the order Q, P, R (not the order of x)
    "interleaved": ([_sq(100), _sq(0), _sq(200), _sq(1), _sq(101), _sq(201), _sq(2), _sq(202), _sq(102)], 1),
    # count == min_neighbors is dropped, min_neighbors + 1 is kept
    "threshold": ([_sq(0)] * 3 + [_sq(100)] * 4, 3),
    # nested, n2 > max(3, n1): the inner class (3) goes, the outer (4) stays
    "nested_more": ([(30, 30, 20, 20)] * 3 + [(20, 20, 60, 60)] * 4, 2),
    # nested, n1 < 3: the inner class (2) goes although the outer has only 2
    "nested_few": ([(30, 30, 20, 20)] * 2 + [(20, 20, 60, 60)] * 2, 1),
    # nested but n2 == n1 == 3: neither branch, both stay
    "nested_equal": ([(30, 30, 20, 20)] * 3 + [(20, 20, 60, 60)] * 3, 2),
    # dx = cvRound(60 * 0.2) = 12: x = 8 is inside the margin, x = 7 just outside
    "margin_in": ([(8, 30, 20, 20)] * 3 + [(20, 20, 60, 60)] * 4, 2),
    "margin_out": ([(7, 30, 20, 20)] * 3 + [(20, 20, 60, 60)] * 4, 2),
    # averages on .5: 0.5 -> 0, 101.5 -> 102, widths 20.5 -> 20 and 21.5 -> 22
    "half_even": ([(0, 0, 20, 20), (1, 0, 21, 20), (101, 0, 21, 20), (102, 0, 22, 20)], 1),
    "duplicates": ([(5, 6, 30, 40)] * 5, 4),
    "empty": ([], 3),
    "single": ([_sq(3)], 1),
}


def jittered(n, n_base, seed):
    """n copies, jittered by up to 2 pixels, of n_base well-separated squares, shuffled."""
    rng = np.random.default_rng(seed)
    base = [(60 * b, 45 * (b % 3), 24 + 4 * (b % 4), 24 + 4 * (b % 4)) for b in range(n_base)]
    which = rng.integers(0, n_base, n)
    jit = rng.integers(-2, 3, (n, 4))
    return [tuple(int(v) for v in np.array(base[w]) + j) for w, j in zip(which, jit)]


for _n in (63, 64, 65):
    CASES[f"jitter_{_n}"] = (jittered(_n, 3, _n), 3)
BIG = (jittered(1100, 7, 7), 5)  # five 256-rectangle tiles: every pair of workgroups of the union kernel


def check_cases_reach_their_branches():
    eps = ho.GROUP_EPS
    g = {k: ho.group_rectangles(r, t) for k, (r, t) in CASES.items()}
    a, b, c = CASES["chain"][0]
    assert ho._similar(a, b, eps) and ho._similar(b, c, eps) and not ho._similar(a, c, eps)
    assert ho.partition(CASES["chain"][0], eps) == ([0, 0, 0], 1) and g["chain"] == [_sq(4)]
    lj = CASES["late_join"][0]
    assert ho.partition(lj[:4], eps)[1] == 4 and ho.partition(lj, eps)[1] == 1 and g["late_join"] == [_sq(12)]
    assert ho.partition(CASES["interleaved"][0], eps)[0] == [0, 1, 2, 1, 0, 2, 1, 2, 0]
    assert g["interleaved"] == [_sq(101), _sq(1), _sq(201)]  # list order of the first members, not x order
    assert g["threshold"] == [_sq(100)]
    assert g["nested_more"] == [(20, 20, 60, 60)] and g["nested_few"] == [(20, 20, 60, 60)]
    assert g["nested_equal"] == [(30, 30, 20, 20), (20, 20, 60, 60)]
    assert g["margin_in"] == [(20, 20, 60, 60)] and g["margin_out"] == [(7, 30, 20, 20), (20, 20, 60, 60)]
    assert g["half_even"] == [(0, 0, 20, 20), (102, 0, 22, 20)]
    assert g["duplicates"] == [(5, 6, 30, 40)] and g["empty"] == [] and g["single"] == []
    for n in (63, 64, 65):
        assert ho.partition(CASES[f"jitter_{n}"][0], eps)[1] == 3 and len(g[f"jitter_{n}"]) == 3
    return g
