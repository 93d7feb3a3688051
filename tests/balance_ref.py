"""The numpy restatement of c3d_balance_matrix (include/c3d.h, steps 1-6): the mask with its closure, the rounds of ICE / VC / sqrt-VC, the
scale and the balanced matrix, in float64 or, by `dtype`, in np.longdouble.  Plain numpy in index order: the sums' orders are numpy's, not
the device's.  tests/test_balance_ref.py holds it to things it does not compute itself; tests/test_gpu_balance.py holds the device to it."""
import numpy as np

ICE, VC, SQRT_VC = 0, 1, 2
METHODS = {"ice": ICE, "vc": VC, "sqrt-vc": SQRT_VC}
MAX_ITERS = 10000


class Refused(ValueError):
    """what the entry answers with C3D_ERR_INVALID"""


class Diverged(ArithmeticError):
    """what the entry answers with C3D_ERR_DIVERGED"""


def seen_by_marginals(M, ignore_diags):
    """step 1: A'(i, j) = M(i, j) where |i - j| >= ignore_diags, else 0 (M itself, not a copy, where ignore_diags is 0)"""
    n = M.shape[0]
    if ignore_diags == 0:
        return M
    A = M.copy()
    for k in range(min(int(ignore_diags), n)):
        i = np.arange(n - k)
        A[i, i + k] = 0.0
        A[i + k, i] = 0.0
    return A


def mask_codes(A, min_nnz=10, mask=None):
    """step 2: 0 kept, 1 listed in mask, 2 fewer than max(min_nnz, 1) non-zeros, 3 removed by the closure"""
    n = A.shape[0]
    pos = A > 0
    code = np.zeros(n, dtype=np.int32)
    if mask is not None:
        code[np.asarray(mask).reshape(-1) != 0] = 1
    code[(code == 0) & (pos.sum(axis=1) < max(int(min_nnz), 1))] = 2
    while True:
        U = code == 0
        out = U & (pos[:, U].sum(axis=1) == 0)
        if not out.any():
            return code
        code[out] = 3


def balance(M, method="ice", ignore_diags=2, min_nnz=10, mask=None, w0=None, tol=1e-5, max_iters=200, target=1.0, rounds=None, dtype=np.float64, want_matrix=True):
    """Steps 1-6.  rounds=R runs exactly R updates (R + 1 passes) whatever tol says; `converged` is then var_R < tol.  A dict with the
    entry's outputs — weights, masked, balanced, history (T + 1 entries), rounds, converged, var, kept, masked_counts, mean_marginal —
    and r_max, the largest r_i of every pass (the tests' bounds need it), all arithmetic in `dtype`; want_matrix=False leaves `balanced` None."""
    M = np.asarray(M, dtype=np.float64)
    method = METHODS.get(method, method)
    n = M.shape[0]
    if M.ndim != 2 or M.shape[1] != n or n < 2:
        raise Refused("n < 2 or not square")
    if not np.isfinite(M).all() or (M < 0).any() or not (M == M.T).all():
        raise Refused("the matrix is not finite, not >= 0 or not symmetric")
    if method not in (ICE, VC, SQRT_VC) or ignore_diags < 0 or not (np.isfinite(target) and target > 0):
        raise Refused("method, ignore_diags or target")
    if method == ICE:
        if not tol >= 0 or not 0 <= max_iters <= MAX_ITERS:
            raise Refused("tol or max_iters")
    else:
        if w0 is not None:
            raise Refused("w0 with VC")
        tol, max_iters = 0.0, 1
    A = seen_by_marginals(M, ignore_diags)
    code = mask_codes(A, min_nnz, mask)
    U = code == 0
    k = int(U.sum())
    if k < 2:
        raise Refused("|U| < 2")
    w = np.zeros(n, dtype=dtype)
    if w0 is not None:
        w0 = np.asarray(w0)
        if not (np.isfinite(w0[U]).all() and (w0[U] > 0).all()):
            raise Refused("w0 on U")
        w[U] = w0[U]
    else:
        w[U] = 1
    Ad = np.asarray(A, dtype=dtype)
    kd = dtype(k)
    history, r_max = [], []
    t, converged = 0, False
    while True:
        s = w * (Ad @ w)
        mbar = s[U].sum() / kd
        r = s[U] / mbar
        var = ((r - 1) ** 2).sum() / kd
        history.append(var)
        r_max.append(r.max())
        if rounds is None:
            if var < tol:
                converged = True
                break
            if t == max_iters:
                break
        elif t == rounds:
            converged = bool(var < tol)
            break
        w[U] = w[U] / (np.sqrt(r) if method == SQRT_VC else r)
        if not (np.isfinite(w[U]).all() and (w[U] > 0).all()):
            raise Diverged("a weight stopped being finite and positive")
        t += 1
    w = w * np.sqrt(dtype(target) / mbar)
    return {"weights": w, "masked": code, "balanced": (w[:, None] * w[None, :]) * np.asarray(M, dtype=dtype) if want_matrix else None, "history": np.array(history, dtype=dtype), "rounds": t,
            "converged": converged, "var": var, "kept": k, "masked_counts": [int((code == c).sum()) for c in (1, 2, 3)], "mean_marginal": mbar,
            "r_max": np.array(r_max, dtype=dtype)}


def worked_example(S, seed=1):
    """the issue's example: a normalised map S turned into biased counts rint(50 S b b^T), b = exp(N(0, 0.5)), with row and column n // 3
    zeroed (an unmappable bin).  Returns (counts, b)."""
    n = S.shape[0]
    b = np.exp(np.random.default_rng(seed).normal(0.0, 0.5, n))
    M = np.rint(50.0 * S * (b[:, None] * b[None, :]))      # (symmetric bit for bit where S is: b_i b_j is one product)
    M[n // 3, :] = 0.0
    M[:, n // 3] = 0.0
    return M, b
