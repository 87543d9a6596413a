"""Split projection of uint8 probes with an fp32 model (EF_OPT_PROJECT_SPLIT_BF16, the default):
F = (p - round(mean)).(W_hi + W_mid + W_lo) - (mean - round(mean)).W on bf16 MFMA, the three
bf16 pieces summing to the fp32 W exactly.  Bit-exact cases where the arithmetic allows them,
the project's own bound elsewhere, and bit-equality with the fp32 kernel (option 0) on every
input the form does not cover."""
import numpy as np
import pytest

from oracle import eigenface_oracle as orc

pytestmark = pytest.mark.gpu

OPT = "project_split_bf16"


@pytest.fixture
def split_eng(eng):
    """The shared engine with the option at its default, restored afterwards."""
    eng.set_option(OPT, 1)
    yield eng
    eng.set_option(OPT, 1)


def _bits(f):
    return np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    np.testing.assert_array_equal(_bits(a), _bits(b))


def _project_opt(eng, p, opt):
    eng.set_option(OPT, opt)
    try:
        return eng.project(p)
    finally:
        eng.set_option(OPT, 1)


def _full_w(rng, d, k):
    """fp32 weights with full 24-bit significands, magnitudes over 2^-20 .. 2^4, random signs."""
    man = rng.integers(0, 1 << 23, (d, k), dtype=np.int64)
    exp = rng.integers(-20, 4, (d, k))
    sig = 1.0 + man.astype(np.float64) / float(1 << 23)
    w = (np.ldexp(sig, exp) * rng.choice([-1.0, 1.0], (d, k))).astype(np.float32)
    assert np.all(w.astype(np.float64) == np.ldexp(sig, exp) * np.sign(w))  # nothing was rounded
    return w


# ---- 1. impulses: every element of W comes back bit for bit ---------------------------------
@pytest.mark.parametrize("d", [128, 192])
@pytest.mark.parametrize("k", [128, 200])
def test_impulse_bit_exact(split_eng, d, k):
    rng = np.random.default_rng(1000 + d + k)
    mu = rng.integers(1, 255, d).astype(np.float32)
    w = _full_w(rng, d, k)
    sign = np.where(np.arange(d) % 2 == 0, 1, -1)
    p = np.repeat(mu[None, :], d, 0).astype(np.int32)
    p[np.arange(d), np.arange(d)] += sign
    assert p.min() >= 0 and p.max() <= 255
    split_eng.set_model(mu, w)
    f = split_eng.project(p.astype(np.uint8))
    _same_bits(f, w * sign[:, None].astype(np.float32))


# ---- 2. integer sums: exact in any summation order ------------------------------------------
@pytest.mark.parametrize("d,k,b", [(64, 16, 1), (4160, 128, 300), (1024, 512, 129), (192, 200, 257),
                                   (4160, 1024, 4096)])  # the last: enough tiles that the K-split is set by
def test_integer_sums_bit_exact(split_eng, d, k, b):      # the 2048 pixels of round(mean) a split keeps in LDS
    rng = np.random.default_rng(2000 + d + k + b)
    wi = rng.integers(-3, 4, (d, k))
    mu = rng.integers(0, 256, d)
    mu[0], mu[d - 1] = 255, 0
    p = rng.integers(0, 256, (b, d))
    p[:, 0], p[:, d - 1] = 0, 255          # p - mean = -255 and +255
    p[0, :] = np.where(mu >= 128, 0, 255)  # one probe as far from the mean as a byte can be
    c = (p - mu[None, :]).astype(np.float64)  # (integers: the fp64 products and sums are exact)
    want = (c @ wi.astype(np.float64)) / 128.0
    assert (np.abs(c) @ np.abs(wi).astype(np.float64)).max() < 1 << 24
    split_eng.set_model(mu.astype(np.float32), (wi / 128.0).astype(np.float32))
    f = split_eng.project(p.astype(np.uint8))
    _same_bits(f, want.astype(np.float32))


# ---- 3. the project's bound with a non-integer mean -----------------------------------------
@pytest.mark.parametrize("d,k,b", [(16384, 128, 1), (16384, 128, 300), (4096, 200, 1), (4096, 200, 300),
                                   (8192, 512, 1), (8192, 512, 300), (4160, 128, 300)])
def test_tolerance_noninteger_mean(split_eng, d, k, b):
    rng = np.random.default_rng(d + k + b)
    mu = rng.uniform(60, 200, d).astype(np.float32)
    w = (rng.standard_normal((d, k)) / np.sqrt(d)).astype(np.float32)
    p = rng.integers(0, 256, (b, d), dtype=np.uint8)
    split_eng.set_model(mu, w)
    f1 = split_eng.project(p)
    f0 = _project_opt(split_eng, p, 0)
    ref = orc.project(p, mu.astype(np.float64), w.astype(np.float64))
    bound = np.abs(p.astype(np.float64) - mu) @ np.abs(w.astype(np.float64))
    e1, e0 = np.abs(f1 - ref), np.abs(f0 - ref)
    print(f"split d={d} k={k} b={b}: max err split {e1.max():.3e} fp32 {e0.max():.3e} ratio "
          f"{e1.max() / e0.max():.3f}; rms ratio {np.sqrt((e1 ** 2).mean() / (e0 ** 2).mean()):.3f}; "
          f"max err / bound {np.max(e1 / (2e-6 * bound + 1e-6)):.3f}")
    assert np.all(e1 <= 2e-6 * bound + 1e-6)


# ---- 4. rows are independent, calls repeat ----------------------------------------------------
def test_rows_independent(split_eng):
    import torch
    rng = np.random.default_rng(4)
    d, k = 1024, 128
    mu = rng.uniform(60, 200, d).astype(np.float32)
    w = (rng.standard_normal((d, k)) / np.sqrt(d)).astype(np.float32)
    p = rng.integers(0, 256, (200, d), dtype=np.uint8)
    split_eng.set_model(mu, w)
    f200 = split_eng.project(p)
    _same_bits(split_eng.project(p[:1]), f200[:1])      # the same padded batch
    _same_bits(split_eng.project(p[:127]), split_eng.project(p[:129])[:127])
    _same_bits(split_eng.project(p), f200)
    pd = torch.from_numpy(p).cuda()
    assert pd.data_ptr() % 16 == 0
    _same_bits(split_eng.project(pd).cpu().numpy(), f200)


# ---- 5. what the form does not cover runs today's kernel ------------------------------------
def _model(rng, d, k, lo=60, hi=200):
    return rng.uniform(lo, hi, d).astype(np.float32), (rng.standard_normal((d, k)) / np.sqrt(d)).astype(np.float32)


def test_eligible_model_takes_the_split_form(split_eng):
    """The control of the fallback cases below: on a model the guard passes the two options do
    not give the same bits (another summation order, no input rounding)."""
    rng = np.random.default_rng(50)
    mu, w = _model(rng, 4096, 128)
    p = rng.integers(0, 256, (200, 4096), dtype=np.uint8)
    split_eng.set_model(mu, w)
    assert not np.array_equal(_bits(split_eng.project(p)), _bits(_project_opt(split_eng, p, 0)))


@pytest.mark.parametrize("case", ["f32_probes", "d333", "d10000", "mean_range", "w_tiny", "w_inf", "w_nan"])
def test_fallback_is_fp32_kernel(split_eng, case):
    rng = np.random.default_rng(51)
    d = {"d333": 333, "d10000": 10000}.get(case, 4096)
    k, b = 128, 200
    mu, w = _model(rng, d, k, *((-40, 300) if case == "mean_range" else (60, 200)))
    if case.startswith("w_"):
        w[1234, 77] = {"w_tiny": np.float32(1e-35), "w_inf": np.float32(np.inf), "w_nan": np.float32(np.nan)}[case]
    p = rng.integers(0, 256, (b, d), dtype=np.uint8)
    if case == "f32_probes":
        p = p.astype(np.float32)
    split_eng.set_model(mu, w)
    _same_bits(split_eng.project(p), _project_opt(split_eng, p, 0))


def test_fallback_unaligned_device_pointer(split_eng):
    import torch
    rng = np.random.default_rng(52)
    d, k, b = 4096, 128, 200
    mu, w = _model(rng, d, k)
    p = rng.integers(0, 256, (b, d), dtype=np.uint8)
    buf = torch.zeros(b * d + 16, dtype=torch.uint8, device="cuda")
    pd = buf[1:1 + b * d].view(b, d)
    pd.copy_(torch.from_numpy(p))
    assert pd.data_ptr() % 16 == 1 and pd.is_contiguous()
    split_eng.set_model(mu, w)
    f1 = split_eng.project(pd).cpu().numpy()
    split_eng.set_option(OPT, 0)
    f0 = split_eng.project(pd).cpu().numpy()
    _same_bits(f1, f0)
    _same_bits(f0, split_eng.project(p))  # option 0: the aligned host copy runs the same arithmetic


# ---- 6. the pieces follow the model; the option is read per call ----------------------------
def test_stale_pieces_and_toggle(split_eng):
    from eigenface import Engine
    rng = np.random.default_rng(6)
    d, k, b = 1024, 128, 130
    mu, w1 = _model(rng, d, k)
    w2 = (rng.standard_normal((d, k)) / np.sqrt(d)).astype(np.float32)
    p = rng.integers(0, 256, (b, d), dtype=np.uint8)
    with Engine(0) as fresh:
        fresh.set_model(mu, w2)
        want1 = fresh.project(p)
        fresh.set_option(OPT, 0)
        want0 = fresh.project(p)
    split_eng.set_model(mu, w1)
    f_w1 = split_eng.project(p)
    split_eng.set_model(mu, w2)
    _same_bits(split_eng.project(p), want1)
    assert not np.array_equal(_bits(f_w1), _bits(want1))
    split_eng.set_option(OPT, 0)
    _same_bits(split_eng.project(p), want0)
    split_eng.set_option(OPT, 1)
    _same_bits(split_eng.project(p), want1)
    assert not np.array_equal(_bits(want0), _bits(want1))


# ---- 7. the option ---------------------------------------------------------------------------
def test_option_default_and_range():
    from eigenface import Engine
    with Engine(0) as e:
        assert e.get_option(OPT) == 1
        for v in (0, 1):
            e.set_option(OPT, v)
            assert e.get_option(OPT) == v
        for v in (2, -1):
            with pytest.raises(Exception):
                e.set_option(OPT, v)
            assert e.get_option(OPT) == 1


# ---- 8. identities ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [64, 128])
def test_identities_do_not_move(split_eng, k):
    rng = np.random.default_rng(80 + k)
    d, n = 4096, 2000
    mu = rng.uniform(60, 200, d).astype(np.float32)
    w = (rng.standard_normal((d, k)) / 64).astype(np.float32)
    gal = rng.integers(0, 256, (n, d), dtype=np.uint8)
    rows = rng.choice(n, 300, replace=False)
    probes = np.clip(gal[rows].astype(np.int32) + rng.integers(-3, 4, (300, d)), 0, 255).astype(np.uint8)
    split_eng.set_model(mu, w)
    idx = {}
    for opt in (0, 1):
        split_eng.set_option(OPT, opt)
        split_eng.set_gallery(split_eng.project(gal))
        idx[opt], _, feats = split_eng.recognize(probes, "l2", return_features=True)
        _same_bits(feats, split_eng.project(probes))
    np.testing.assert_array_equal(idx[1], rows)
    np.testing.assert_array_equal(idx[0], idx[1])
