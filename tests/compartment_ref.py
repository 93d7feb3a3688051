"""c3d_compartments restated in numpy: the definitions of include/c3d.h, rounded as defined.

A map M is n x n and symmetric: IF, one model's distance map (sqrt(((ux ux) + uy uy) + uz uz), the distance of c3d_compare_replicas) or
the mean over a pick list of such maps, summed in list order and divided by the count (c3d_ensemble_map's `mean`).
  1. E[s] = mean over i of M(i, i+s); E[0] = 0.  The sum is taken in extended precision and rounded once, so that the device's sum of
     T terms, whatever its order, lies within T 2^-53 of it (relative).
  2. X(i,j) = M(i,j) / E[|i-j|] where |i-j| >= min_sep and E != 0, 1 elsewhere; every pair once, both halves from one value.
  3. m_i = mean_j X(i,j), q_i = sqrt(mean_j (X(i,j) - m_i)^2), D_i = 1/q_i or 0, live = #{q_i > 0}.
  4. C v = D (X w - m (1 . w)) / n with w = X (D v) - (m . D v) 1.
  5. rounds of modified Gram-Schmidt and Y = C V; lambda, share = lambda / live, residual.
  6. the two sign rules.   7. |Pearson r| and the same-side share against IF's vectors.
The sums of 3 - 7 are numpy's; the device's run in another order, which tests/test_gpu_compartments.py bounds."""
import numpy as np


def start(n, n_vec):
    """c3d_compartment_start: ((h + 0.5) / 2^32) - 0.5 of the 32-bit hash h of k = 4 i + a; exact in float64"""
    i = np.arange(n, dtype=np.uint64)
    out = np.empty((n_vec, n))
    M = np.uint64(0xFFFFFFFF)
    for a in range(n_vec):
        h = (np.uint64(4) * i + np.uint64(a) + np.uint64(0x9E3779B9)) & M
        h ^= h >> np.uint64(16)
        h = (h * np.uint64(0x85EBCA6B)) & M
        h ^= h >> np.uint64(13)
        h = (h * np.uint64(0xC2B2AE35)) & M
        h ^= h >> np.uint64(16)
        out[a] = (h.astype(np.float64) + 0.5) / 4294967296.0 - 0.5
    return out


def rows_of_distance_map(x, r0, r1):
    """rows r0..r1-1 of a model's distance map, the host's distance operation for operation"""
    x = np.asarray(x, dtype=np.float64)
    u = x[r0:r1, None, :] - x[None, :, :]
    return np.sqrt(((u[..., 0] * u[..., 0]) + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2])


def distance_map(x):
    return rows_of_distance_map(x, 0, len(x))


def consensus_map(models):
    """the mean distance map of the models, summed in list order from 0.0 and divided once"""
    s = np.zeros((len(models[0]), len(models[0])))
    for x in models:
        s = s + distance_map(x)
    return s / float(len(models))


class BlockedMap:
    """a model's O/E map formed and kept in row blocks, never as one n x n temporary with its n x n x 3 differences (the 16384-bead case)"""

    def __init__(self, x, min_sep=1, block=512):
        self.x, self.n, self.min_sep, self.block = np.asarray(x, dtype=np.float64), len(x), min_sep, block
        n, x = self.n, self.x
        acc = np.zeros(n, dtype=np.longdouble)
        self.rows = []
        for r0 in range(0, n, block):
            r1 = min(n, r0 + block)
            d = np.square(x[r0:r1, 0, None] - x[None, :, 0])
            d += np.square(x[r0:r1, 1, None] - x[None, :, 1])
            d += np.square(x[r0:r1, 2, None] - x[None, :, 2])
            np.sqrt(d, out=d)
            for k in range(r1 - r0):
                acc[:n - r0 - k] += d[k, r0 + k:]
            self.rows.append(d)
        self.E = expected_from_sums(acc, n)
        self.m, self.q = np.empty(n), np.empty(n)
        j = np.arange(n)
        for b, r0 in enumerate(range(0, n, block)):
            X = self.rows[b]
            sep = np.abs(np.arange(r0, r0 + len(X))[:, None] - j[None, :])
            e = self.E[sep]
            on = (sep >= min_sep) & (e != 0.0)
            np.divide(X, e, out=X, where=on)
            X[~on] = 1.0
            self.m[r0:r0 + len(X)] = X.mean(axis=1)
            self.q[r0:r0 + len(X)] = np.sqrt(np.square(X - self.m[r0:r0 + len(X), None]).mean(axis=1))

    def blocks(self):
        for b, r0 in enumerate(range(0, self.n, self.block)):
            yield r0, self.rows[b]

    def dot(self, U):
        """X U^T for U [k, n] -> [k, n]"""
        out = np.empty_like(U)
        for r0, X in self.blocks():
            out[:, r0:r0 + len(X)] = (X @ U.T).T
        return out


def expected_from_sums(acc, n):
    E = np.zeros(n)
    # sum and division in extended precision, one rounding to double: within 2^-53 of the exact mean, so that a double sum of T terms in
    # any order (at most T - 1 roundings) and its division (one more) stay within T 2^-53 of this value to first order
    E[1:] = (acc[1:] / np.arange(n - 1, 0, -1).astype(np.longdouble)).astype(np.float64)
    return E


def expected(M):
    """E[s], s = 0..n-1: the diagonal sums in extended precision, rounded once, divided by the count in double"""
    M = np.asarray(M, dtype=np.float64)
    n = len(M)
    acc = np.zeros(n, dtype=np.longdouble)
    for i in range(n):
        acc[:n - i] += M[i, i:]
    return expected_from_sums(acc, n)


def oe(M, min_sep=1, E=None):
    """the observed/expected map X"""
    M = np.asarray(M, dtype=np.float64)
    n = len(M)
    E = expected(M) if E is None else E
    i, j = np.triu_indices(n, 1)
    e = E[j - i]
    on = (j - i >= min_sep) & (e != 0.0)
    v = np.where(on, M[i, j] / np.where(on, e, 1.0), 1.0)
    X = np.ones((n, n))
    X[i, j] = v
    X[j, i] = v
    return X


def row_stats(X):
    m = X.mean(axis=1)
    q = np.sqrt(((X - m[:, None]) ** 2).mean(axis=1))
    return m, q


class Dependent(ValueError):
    """a vector projected to exactly 0: the call's C3D_ERR_INVALID "dependent start vectors\""""


def orthonormalise(V):
    V = V.copy()
    for a in range(len(V)):
        for b in range(a):
            V[a] -= (V[b] @ V[a]) * V[b]
        nn = V[a] @ V[a]
        if not nn > 0.0:
            raise Dependent("dependent start vectors")
        V[a] /= np.sqrt(nn)
    return V


def sign_largest(v):
    at = int(np.argmax(np.abs(v)))                  # the first of equal magnitudes
    return -v if v[at] < 0.0 else v


def pearson(x, y):
    xc, yc = x - x.sum() / len(x), y - y.sum() / len(y)
    return (xc @ yc) / np.sqrt((xc @ xc) * (yc @ yc))


def solve_operator(dot, m, q, n_vec=1, iters=200, start_vectors=None):
    """steps 4 and 5 for a map given by `dot` (U [k, n] -> X U^T [k, n]) and its row statistics: (V, lambda, share, residual), unsigned"""
    n = len(m)
    D = np.where(q > 0.0, 1.0 / np.where(q > 0.0, q, 1.0), 0.0)
    live = int((q > 0.0).sum())

    def C(V):
        U = D[None, :] * V
        W = dot(U) - (U @ m)[:, None]
        return D[None, :] * (dot(W) - m[None, :] * W.sum(axis=1)[:, None]) / float(n)

    V = np.array(start(n, n_vec) if start_vectors is None else start_vectors, dtype=np.float64)
    for _ in range(iters):
        V = C(orthonormalise(V))
    V = orthonormalise(V)
    Y = C(V)
    lam = np.einsum("aj,aj->a", V, Y)
    res = np.sqrt(((Y - lam[:, None] * V) ** 2).sum(axis=1))
    share = lam / live if live else np.zeros(n_vec)
    return V, lam, share, res


def solve_map(M, min_sep=1, n_vec=1, iters=200, start_vectors=None):
    """(E, V, share, residual) of one map, vectors unsigned"""
    E = expected(M)
    X = oe(M, min_sep, E)
    m, q = row_stats(X)
    V, _, share, res = solve_operator(lambda U: U @ X, m, q, n_vec, iters, start_vectors)
    return E, V, share, res


def compartments(maps, has_if, min_sep=1, n_vec=1, iters=200, start_vectors=None):
    """the call: maps = the Q matrices in order (IF first when has_if).  A dict as Solver.compartments returns it."""
    Q = len(maps)
    out = {"expected": [], "vectors": [], "share": [], "residual": [], "agreement": [], "same_side": []}
    F = None
    for q, M in enumerate(maps):
        E, V, share, res = solve_map(M, min_sep, n_vec, iters, start_vectors)
        if not has_if or q == 0:
            V = np.stack([sign_largest(v) for v in V])
            if has_if:
                F = V
        else:
            V = sign_against(V, F)
            out["agreement"].append(np.array([[abs(pearson(V[a], F[b])) for b in range(n_vec)] for a in range(n_vec)]))
            out["same_side"].append(np.array([float(((V[a] * F[a]) > 0.0).sum()) / len(E) for a in range(n_vec)]))
        for k, v in (("expected", E), ("vectors", V), ("share", share), ("residual", res)):
            out[k].append(v)
    return {k: np.array(v) for k, v in out.items() if len(v) or k not in ("agreement", "same_side")} | {"Q": Q}


def sign_against(V, F):
    out = []
    for a in range(len(V)):
        d = V[a] @ F[a]
        out.append(-V[a] if d < 0.0 else (V[a] if d > 0.0 else sign_largest(V[a])))
    return np.stack(out)


def eigh_vectors(M, min_sep=1, k=3):
    """(eigenvalues descending, eigenvectors as rows) of numpy.corrcoef of the O/E map's live rows, dead rows 0: what the iteration
    converges to.  The eigenvalues are those of C / ... times live / n: corrcoef has trace `live`, C has trace live too (its diagonal is 1
    on live rows), so they compare directly."""
    X = oe(M, min_sep)
    m, q = row_stats(X)
    live = q > 0.0
    Cm = np.corrcoef(X[live])
    w, U = np.linalg.eigh(Cm)
    order = np.argsort(w)[::-1]
    vec = np.zeros((len(order), len(M)))
    vec[:, live] = U[:, order].T
    return w[order], vec[:k] if k else vec


def planted_chain(n, seed=0, block=None):
    """a two-compartment chain: labels in alternating blocks, coordinates a random coil pulled towards one of two centres by label.
    Returns (xyz [n, 3] float64, labels [n] in {-1, +1})."""
    rng = np.random.default_rng(1000 + n + seed)
    block = block or max(2, n // 4)
    labels = np.where((np.arange(n) // block) % 2 == 0, 1, -1)
    centre = np.array([12.0, 0.0, 0.0])
    x = labels[:, None] * centre[None, :] + rng.normal(scale=2.0, size=(n, 3))
    return x, labels


def planted_model(n, seed=0, box=(60.0, 30.0, 15.0), noise=2.0):
    """a model with three planted axes of unequal weight: bead i sits at the corner of `box` its block's three bits name, plus noise — the
    leading eigenvalues of its map are well apart (the GPU tests assert that from eigh).  float32, as a replica holds it."""
    rng = np.random.default_rng(5000 + 17 * n + seed)
    i = np.arange(n)
    b = max(1, n // 16)
    bits = np.stack([(i // b) % 2, (i // (2 * b)) % 2, (i // (4 * b)) % 2], axis=1)
    return (bits * np.array(box)[None, :] + rng.normal(scale=noise, size=(n, 3))).astype(np.float32)


def gap_ratio(M, min_sep, n_vec):
    """g = the largest lambda_{a+1} / lambda_a among the first n_vec eigenvalues of the map's correlation, from eigh"""
    w, _ = eigh_vectors(M, min_sep, 0)
    w = np.concatenate([np.maximum(w, 0.0), np.zeros(n_vec + 1)])
    return max(w[a + 1] / w[a] if w[a] > 0.0 else np.inf for a in range(n_vec))
