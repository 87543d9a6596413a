"""The arithmetic facts the split projection (EF_OPT_PROJECT_SPLIT_BF16) rests on, restated in
NumPy: w = hi + mid + lo with each piece the round-to-nearest-even bf16 of the running
remainder.  No GPU: the kernel's guard evaluates the same conditions on the device."""
import numpy as np

MIN_NORMAL = 2.0 ** -126


def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32; finite inputs."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def split3(w):
    w = np.ascontiguousarray(w, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        hi = bf16_rne(w)
        r1 = w - hi
        mid = bf16_rne(r1)
        lo = bf16_rne(r1 - mid)
    return hi, mid, lo


def sums_exactly(w):
    hi, mid, lo = split3(w)
    with np.errstate(invalid="ignore"):
        return hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64) == w.astype(np.float64)


def guard_ok(w):
    """Per element: what the device-side guard requires."""
    hi, mid, lo = split3(w)
    ok = np.isfinite(w) & np.isfinite(hi) & sums_exactly(w)
    with np.errstate(invalid="ignore"):
        for piece in (hi, mid, lo):
            ok &= (piece == 0) | (np.abs(piece) >= MIN_NORMAL)
    return ok


def _random_bits(rng, n):
    w = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return w[np.isfinite(w)]


def test_byte_differences_are_exact_in_bf16():
    v = np.arange(-255, 256).astype(np.float32)
    np.testing.assert_array_equal(bf16_rne(v), v)
    # and the kernel's conversion, the high half of the fp32 value, is that same number
    np.testing.assert_array_equal(((v.view(np.uint32) >> 16) << 16).view(np.float32), v)


def test_products_are_exact_in_fp32():
    """An integer of at most 8 bits times a bf16 piece (8-bit significand) needs 16 bits."""
    rng = np.random.default_rng(1)
    piece = bf16_rne(rng.standard_normal(4096).astype(np.float32))
    a = rng.integers(-255, 256, 4096).astype(np.float32)
    np.testing.assert_array_equal((a * piece).astype(np.float64), a.astype(np.float64) * piece.astype(np.float64))


def test_split_exact_for_eigenface_weights():
    rng = np.random.default_rng(2)
    for d in (4096, 16384, 65536):
        w = (rng.standard_normal(200000) / np.sqrt(d)).astype(np.float32)
        assert guard_ok(w).all()
    assert guard_ok(np.zeros(8, np.float32)).all()  # padded columns


def test_split_exact_over_the_guards_domain():
    rng = np.random.default_rng(3)
    w = _random_bits(rng, 2_000_000)
    hi = bf16_rne(w)
    inside = (np.abs(w) >= 2.0 ** -110) & np.isfinite(hi)
    assert inside.sum() > 1_000_000
    assert sums_exactly(w[inside]).all()
    # ... and from 2^-102 up (a piece is at least one ulp of w, 2^-23 |w|) every piece is normal
    assert guard_ok(w[inside & (np.abs(w) >= 2.0 ** -102)]).all()
    # a value whose hi rounds to infinity is outside it
    top = np.array([3.4e38, -3.4e38], np.float32)
    assert not np.isfinite(bf16_rne(top)).any() and not guard_ok(top).any()


def test_guard_trips_below_the_domain():
    rng = np.random.default_rng(4)
    w = _random_bits(rng, 4_000_000)
    tiny = w[(np.abs(w) < 2.0 ** -112) & (w != 0)]
    assert tiny.size > 10_000
    # there the split loses bits or a piece is subnormal (the few that pass have low bits of zero)
    assert (~sums_exactly(tiny)).any()
    assert (~guard_ok(tiny)).mean() > 0.9
    # a subnormal piece appears only below about 9.9e-32
    sub = np.zeros(w.shape, bool)
    for piece in split3(w):
        sub |= (piece != 0) & (np.abs(piece) < MIN_NORMAL)
    assert np.abs(w[sub]).max() < 1e-31
    # the three guarded models of the GPU test: one 1e-35, inf or NaN element rules a model out
    assert not guard_ok(np.array([1e-35, np.inf, np.nan], np.float32)).any()
