"""The single-bf16 prefix screen (EF_OPT_SEARCH_PREFIX_SCREEN) restated in NumPy /
torch: the constants of its bound, the scores its kernel forms and the proof of its reduce."""
import numpy as np
import torch

U = 2.0 ** -24
ES = 2.01 * 2.0 ** -8  # bf16 round-to-nearest of both operands: |2qg - 2q^g^| <= ES 2|q||g|


def cf(k1):
    """K1 + 6 roundings of the fp32 chain at 2u each, 1 % for the rounded operands' products."""
    return (k1 + 6) * 2.0 * U * 1.01


def cg(k1):
    """The row's share of the fp32 slack (chain and fp32 norm), safety factor 2."""
    return 2.0 * (2.01 * cf(k1) + k1 * U)


def cq(k1):
    """The probe's share of the fp32 slack, safety factor 2."""
    return 2.0 * 1.01 * cf(k1)


def underflow(k1, qn, gm):
    return (4 * k1 + 8) * 2.0 ** -126 * (1.0 + 2.02 * qn + gm)


def bound(k1, q1, g1):
    """|S~1 - S1| <= this for a (probe, row) pair: es (q1 + g1) + slack."""
    return (ES + cq(k1)) * q1 + (ES + cg(k1)) * g1


def bf16(x):
    """fp32 array rounded to bf16 (nearest even), back as fp32."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def norms1(g, k1):
    """fp32 ||g[:K1]||^2 as the gallery kernel sums it (fp32 FMA chain; order differs only)."""
    gp = g[:, :k1].astype(np.float32)
    return np.einsum("ij,ij->i", gp, gp, dtype=np.float32)


def start_values(gn1, k1):
    """The chains' start values: fp32 gn1 (1 - es - cg), rounded down by 1 - 2^-22."""
    fac = np.float32(1.0 - ES - cg(k1))
    return (gn1.astype(np.float32) * fac) * np.float32(1.0 - 2.0 ** -22)


def chain(start, q, g, k1):
    """fp32 chain of one bf16 product per element from the rows' start values: [b][n] fp32."""
    qh = torch.from_numpy(bf16(-2.0 * q[:, :k1].astype(np.float32)))
    gh = torch.from_numpy(bf16(g[:, :k1]))
    acc = torch.from_numpy(np.ascontiguousarray(start, dtype=np.float32))[None, :].repeat(len(q), 1)
    for i in range(k1):  # products of two bf16 values are exact in fp32; every add rounds once
        acc = acc + qh[:, i:i + 1] * gh[None, :, i]
    return acc.numpy()


def exact_s1(q, g, k1):
    q64, g64 = q[:, :k1].astype(np.float64), g[:, :k1].astype(np.float64)
    return (g64 ** 2).sum(1)[None, :] - 2.0 * q64 @ g64.T


def screen_proves(q, g, k1):
    """The screen's decision per probe as the reduce takes it: (proven, winner, margin) with the
    records of an exact top-2 over the lower bounds L."""
    L = chain(start_values(norms1(g, k1), k1), q, g, k1).astype(np.float64)
    w = L.argmin(1)
    rows = np.arange(len(q))
    L[rows, w] = np.inf
    r2 = L.min(1)
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    q1 = (q64[:, :k1] ** 2).sum(1)
    qq = (q64 ** 2).sum(1)
    gmax2 = (g64 ** 2).sum(1).max()
    dw = ((q64 - g64[w]) ** 2).sum(1)
    tol = 1e-12 * (dw + qq + gmax2)
    margin = q1 * (1.0 - ES - cq(k1)) + r2 - underflow(k1, np.sqrt(qq), np.sqrt(gmax2)) - dw - tol
    return margin > 0, w, margin
