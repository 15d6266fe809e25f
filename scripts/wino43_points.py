"""Interpolation points of the Winograd F(4x4,3x3) family (csrc/wino43.h), on the CPU with numpy.

    python scripts/wino43_points.py            # the matrices of the chosen points, then the error table
    python scripts/wino43_points.py --ci 256   # a shorter reduction (faster)

toom_cook(points, m, r) builds A^T [m][n], G [n][r] and B^T [n][n] (n = m + r - 1; the last point is infinity) for
Y = A^T [(G g) .* (B^T d)] by the Toom-Cook construction in exact rationals: with M(x) = prod (x - p_i) over the finite points,
  A^T[i][j] = p_j^i, G[j][k] = p_j^k / M'(p_j), B^T[j][:] = the coefficients of M(x) / (x - p_j)      (finite j)
and for infinity A^T[m-1][n-1] = 1, G[n-1][r-1] = 1, B^T[n-1][:] = the coefficients of M(x).  Row j of G and of B^T may be
rescaled by s and 1/s; the scale here (the 1/M'(p_j) factor on G) is the one csrc/wino43.h holds: it keeps B^T and A^T in small
dyadic numbers that float32 multiplies exactly.

The table: a 2-D layer with Ci input channels, N(0,1) inputs, N(0,0.02^2) weights, float32 transforms, float32 products
accumulated in float32 over chains of 32 (the MFMA K loop's depth per chunk) whose partial sums are added in float32, against
the float64 direct convolution.  worst = max|err| / max|y|, rms = rms(err) / rms(y).
"""
import argparse
from fractions import Fraction as Fr

import numpy as np

INF = None
CHOSEN = (0, 1, -1, Fr(1, 2), -2, INF)
POINT_SETS = [
    ("F(4x4,3x3), Lavin 0, +-1, +-2, inf", (0, 1, -1, 2, -2, INF)),
    ("F(4x4,3x3), 0, +-1, +-1/2, inf", (0, 1, -1, Fr(1, 2), Fr(-1, 2), INF)),
    ("F(4x4,3x3), 0, 1, -1, 1/2, -2, inf", CHOSEN),
    ("F(4x4,3x3), 0, 1, -1, 2, -1/2, inf", (0, 1, -1, 2, Fr(-1, 2), INF)),
]


def poly_mul(a, b):
    out = [Fr(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] += x * y
    return out


def toom_cook(points, m, r):
    """(A^T, G, B^T) as lists of lists of Fractions; points: n - 1 finite values and INF last."""
    n = m + r - 1
    assert len(points) == n and points[-1] is INF
    fin = [Fr(p) for p in points[:-1]]
    M = [Fr(1)]
    for p in fin:
        M = poly_mul(M, [-p, Fr(1)])                     # ascending coefficients of prod (x - p)
    AT = [[Fr(0)] * n for _ in range(m)]
    G = [[Fr(0)] * r for _ in range(n)]
    BT = [[Fr(0)] * n for _ in range(n)]
    for j, p in enumerate(fin):
        q = [Fr(1)]
        for k, o in enumerate(fin):
            if k != j:
                q = poly_mul(q, [-o, Fr(1)])             # M(x) / (x - p_j), degree n - 2
        dM = sum(c * p ** k for k, c in enumerate(q))    # M'(p_j)
        for i in range(m):
            AT[i][j] = p ** i
        for k in range(r):
            G[j][k] = p ** k / dM
        for k, c in enumerate(q):
            BT[j][k] = c
    AT[m - 1][n - 1] = Fr(1)
    G[n - 1][r - 1] = Fr(1)
    for k, c in enumerate(M):
        BT[n - 1][k] = c
    # sign convention of the printed family: a positive 1/M' scale on the x = 0 row
    if G[0][0] < 0:
        G[0] = [-v for v in G[0]]
        BT[0] = [-v for v in BT[0]]
    return AT, G, BT


def as_np(mat, dtype):
    return np.array([[float(v) for v in row] for row in mat], dtype=dtype)


def conv_direct(d, g):
    """d [Ci, H, W], g [Ci, 3, 3] -> valid correlation [H - 2, W - 2] in the arrays' dtype."""
    H, W = d.shape[1] - 2, d.shape[2] - 2
    out = np.zeros((H, W), dtype=d.dtype)
    for r in range(3):
        for s in range(3):
            out += (d[:, r:r + H, s:s + W] * g[:, r, s][:, None, None]).sum(0, dtype=d.dtype)
    return out


def chained_sum(p, chain=32):
    """Sum over axis 0 in float32: chains of `chain` sequential additions, then the partial sums in order."""
    acc = np.zeros(p.shape[1:], dtype=np.float32)
    for c0 in range(0, p.shape[0], chain):
        part = np.zeros(p.shape[1:], dtype=np.float32)
        for k in range(c0, min(c0 + chain, p.shape[0])):
            part = part + p[k]
        acc = acc + part
    return acc


def wino_tile(points, d, g, m=4, r=3):
    """One m x m output tile from d [Ci, n, n], g [Ci, r, r], float32 throughout."""
    AT, G, BT = (as_np(x, np.float32) for x in toom_cook(points, m, r))
    U = np.einsum("ir,crs,js->cij", G, g, G).astype(np.float32)
    V = np.einsum("ir,crs,js->cij", BT, d, BT).astype(np.float32)
    Mx = chained_sum((U * V).astype(np.float32))
    return np.einsum("ir,rs,js->ij", AT, Mx, AT).astype(np.float32)


def errors(tile_fn, ci, trials, seed=0):
    rng = np.random.default_rng(seed)
    err, ref = [], []
    for _ in range(trials):
        d = rng.standard_normal((ci, 6, 6)).astype(np.float32)
        g = (0.02 * rng.standard_normal((ci, 3, 3))).astype(np.float32)
        want = conv_direct(d.astype(np.float64), g.astype(np.float64))
        got = tile_fn(d, g)
        err.append(got.astype(np.float64) - want)
        ref.append(want)
    err, ref = np.array(err), np.array(ref)
    return np.abs(err).max() / np.abs(ref).max(), np.sqrt((err ** 2).mean()) / np.sqrt((ref ** 2).mean())


def f23_tiles(d, g):
    """The 4x4 outputs as four F(2x2,3x3) tiles, points (0, 1, -1, inf)."""
    pts = (0, 1, -1, INF)
    out = np.zeros((4, 4), dtype=np.float32)
    for ty in range(2):
        for tx in range(2):
            out[2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = wino_tile(pts, d[:, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4], g, m=2)
    return out


def direct32(d, g):
    p = np.stack([d[:, r:r + 4, s:s + 4] * g[:, r, s][:, None, None] for r in range(3) for s in range(3)], 0)
    return chained_sum(p.reshape(-1, 4, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ci", type=int, default=1024)
    ap.add_argument("--trials", type=int, default=64)
    a = ap.parse_args()
    AT, G, BT = toom_cook(CHOSEN, 4, 3)
    for name, mat in (("A^T", AT), ("G", G), ("B^T", BT)):
        print(name)
        for row in mat:
            print("   ", "  ".join("%6s" % v for v in row))
    # exactness in float64: Y = A^T [(G g G^T) .* (B^T d B)] A against the direct convolution
    rng = np.random.default_rng(1)
    d, g = rng.standard_normal((1, 6, 6)), rng.standard_normal((1, 3, 3))
    a64, g64, b64 = (as_np(x, np.float64) for x in (AT, G, BT))
    y = a64 @ ((g64 @ g[0] @ g64.T) * (b64 @ d[0] @ b64.T)) @ a64.T
    print("float64 check against the direct convolution: %.1e" % np.abs(y - conv_direct(d, g)).max())
    print("\nCi = %d, %d tiles of N(0,1) inputs and N(0,0.02^2) weights" % (a.ci, a.trials))
    print("| family / points | worst error | rms error |\n|---|---|---|")
    rows = [("F(2x2,3x3), points 0, +-1", f23_tiles), ("direct float32", direct32)]
    rows += [(name, (lambda d, g, p=pts: wino_tile(p, d, g))) for name, pts in POINT_SETS]
    for name, fn in rows:
        print("| %s | %.1e | %.1e |" % ((name,) + errors(fn, a.ci, a.trials)))


if __name__ == "__main__":
    main()
