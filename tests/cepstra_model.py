"""numpy model of the cepstral features of include/afg.h (afg_cep_dct, afg_cepstra_hip, afg_batch_decode_mfcc): the float64
statement -- the closed-form DCT-II with its lifter, the matrix product, the regression formula of the deltas -- and the
float32 restatement of the kernel's sums on the exact fmaf of tests/melspec_model.py: every sum a chain of fmaf from +0.0f in
ascending index order, the differences and the final product rounded on their own.

Error bounds of the float32 model against the float64 statement, u = 2^-24.
  statics.  c[q][t] is an fmaf chain over n_mels exact products: recursive summation of n_mels terms with one rounding each
    (the first rounds the product itself).  |c32 - c| <= n_mels u sum_m |D[q][m]| |x[m][t]| =: E[q][t]  (Jeannerod and Rump,
    "Improved error bounds for inner products in floating-point arithmetic", 2013: no second-order term is needed; a fused
    chain rounds less often than the product-then-add chain the result is stated for).
  deltas.  With a[t] the exact input sequence, a32 its float32 version and A >= |a32 - a| its bound, g = 1 / (2 sum n^2):
    the differences read a32, which moves the exact sum by at most sum_n n (A[t+n] + A[t-n]); each difference is rounded once,
    the chain over N exact products n * diff rounds N times (as above), g is rounded once and the final product once --
    N + 3 roundings of terms whose magnitudes sum to at most S = sum_n n (|a[t+n] - a[t-n]| + A[t+n] + A[t-n]), and one more
    u S covers every second-order term (all of them carry u^2 and N + 3 <= 11):
      |d32 - d| <= g (sum_n n (A[t+n] + A[t-n]) + (N + 4) u S)
    (indices clamped into [0, F)).  For d1, a = c and A = E; for d2, a = d1 and A is d1's bound."""
import numpy as np

import melspec_model as mm

DCT_NONE, DCT_ORTHO = 0, 1
TILE = 64
U = 2.0 ** -24

ROW_DTYPE = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("first_tile", np.uint64), ("frames", np.uint32),
                      ("reserved", np.uint32)])


def dct64(n_ceps, n_mels, norm=DCT_ORTHO, lifter=0.0, log_scale=1.0):
    """the table in float64, [n_ceps, n_mels]: log_scale * L[q] * s[q] * cos(pi * q * (2 m + 1) / (2 n_mels)), the product
    q * (2 m + 1) reduced mod 4 n_mels in integers"""
    q = np.arange(n_ceps, dtype=np.int64)
    m = np.arange(n_mels, dtype=np.int64)
    r = (q[:, None] * (2 * m[None, :] + 1)) % (4 * n_mels)
    L = 1.0 + (lifter / 2.0) * np.sin(np.pi * q.astype(np.float64) / lifter) if lifter > 0 else np.ones(n_ceps)
    s = np.where(q == 0, np.sqrt(1.0 / n_mels), np.sqrt(2.0 / n_mels)) if norm == DCT_ORTHO else np.full(n_ceps, 2.0)
    return (log_scale * L * s)[:, None] * np.cos(np.pi * r.astype(np.float64) / (2.0 * n_mels))


def layout(rows):
    """afg_cep_layout on a ROW_DTYPE array: fills first_tile, returns the tile count"""
    tiles = 0
    for r in rows:
        r["first_tile"] = tiles
        tiles += (int(r["frames"]) + TILE - 1) // TILE
    return tiles


def gain64(N):
    return 1.0 / (2.0 * sum(n * n for n in range(1, N + 1)))


def clamped(F, t):
    return np.clip(t, 0, F - 1)


def delta64(a, N):
    """the regression formula in float64 along the last axis, edges replicated"""
    a = np.asarray(a, np.float64)
    F = a.shape[-1]
    t = np.arange(F)
    acc = np.zeros(a.shape)
    for n in range(1, N + 1):
        acc = acc + n * (a[..., clamped(F, t + n)] - a[..., clamped(F, t - n)])
    return acc * gain64(N)


def delta_bound(a, A, N):
    """the bound of the module docstring: a the exact sequence (float64), A the bound of its float32 version's error"""
    F = a.shape[-1]
    t = np.arange(F)
    moved, S = np.zeros(a.shape), np.zeros(a.shape)
    for n in range(1, N + 1):
        hi, lo = clamped(F, t + n), clamped(F, t - n)
        moved = moved + n * (A[..., hi] + A[..., lo])
        S = S + n * (np.abs(a[..., hi] - a[..., lo]) + A[..., hi] + A[..., lo])
    return gain64(N) * (moved + (N + 4) * U * S)


def delta32(a, N, mutant=None):
    """the kernel's delta of a float32 sequence along the last axis.  mutant: one wrong place, for the tests that show the
    bound notices it -- "clamp" (indices wrap around instead of replicating the edge), "n0" (n runs 0 .. N - 1), "gain" (the
    product with g is missing)"""
    a = np.asarray(a, np.float32)
    F = a.shape[-1]
    t = np.arange(F)
    acc = np.zeros(a.shape, np.float32)
    with np.errstate(all="ignore"):
        for n in (range(0, N) if mutant == "n0" else range(1, N + 1)):
            hi, lo = ((t + n) % F, (t - n) % F) if mutant == "clamp" else (clamped(F, t + n), clamped(F, t - n))
            diff = (a[..., hi] - a[..., lo]).astype(np.float32)
            acc = mm.fmaf32(np.float32(n), diff, acc)
        return acc if mutant == "gain" else (acc * np.float32(gain64(N))).astype(np.float32)


def cepstra32(D, x, delta_order=0, N=2, mutant=None):
    """the kernel's output of one slab x [n_mels, F] with the float32 table D [n_ceps, n_mels]: [(1 + delta_order) * n_ceps, F].
    mutant: delta32's, or "d2c" (the delta-deltas taken of the statics), "swap" (the delta planes exchanged)"""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        planes = [mm.chain32(D, x)]
    inner = mutant if mutant in ("clamp", "n0", "gain") else None
    if delta_order >= 1:
        planes.append(delta32(planes[0], N, inner))
    if delta_order >= 2:
        planes.append(delta32(planes[0] if mutant == "d2c" else planes[1], N, inner))
    if mutant == "swap" and delta_order >= 2:
        planes[1], planes[2] = planes[2], planes[1]
    return np.concatenate(planes, axis=0)


def cepstra64(D, x, delta_order=0, N=2):
    """the float64 statement with the same table, and the bound of the float32 model's distance from it: (value, bound)"""
    D, x = np.asarray(D, np.float64), np.asarray(x, np.float64)
    planes = [D @ x]
    bounds = [D.shape[1] * U * (np.abs(D) @ np.abs(x))]
    for _ in range(delta_order):
        bounds.append(delta_bound(planes[-1], bounds[-1], N))
        planes.append(delta64(planes[-1], N))
    return np.concatenate(planes, axis=0), np.concatenate(bounds, axis=0)
