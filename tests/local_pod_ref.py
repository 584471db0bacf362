"""NumPy restatement of the local POD basis extension (include/lrbms_hip.h: lrbms_local_pod) with a dense local
product, the SVD in the product it is pinned against, a NumPy restatement of the eigen kernel's Jacobi iteration, and the inputs
the GPU tests share (tests/test_local_pod_host.py checks their margins on the CPU)."""
import numpy as np
import scipy.linalg as sla

L_VALUES = (1, 3, 16, 17, 64, 65, 128)
EPS = np.finfo(np.float64).eps


# The Gram route finds lam_j = sigma_j^2 with an absolute error of order eps sigma_1^2, so sigma_j with eps sigma_1^2 / sigma_j:
# within SIGMA_TOL sigma_1 for every sigma_j >= RESOLVED sigma_1 (2.2e-7: about where rtol >= 1e-7 keeps the threshold), and
# within NOISE sigma_1 = 4 sqrt(eps) sigma_1 for the ones below, which no admissible threshold retains.
SIGMA_TOL = 1e-9
RESOLVED = EPS / SIGMA_TOL
NOISE = 4.0 * np.sqrt(EPS)


def sigma_error(sv, sig):
    """(largest error over the resolved values, largest error over the rest), both relative to sigma_1 = sig[0]."""
    m = min(len(sv), len(sig))
    err = np.abs(sv[:m] - sig[:m]) / sig[0]
    res = sig[:m] >= RESOLVED * sig[0]
    return float(err[res].max()), float(err[~res].max()) if (~res).any() else 0.0


def sym(A):
    return 0.5 * (A + A.T)


def local_pod_one(U, V, nloc, P, modes, rtol=1e-6, atol=0.0):
    """Steps 1-9 for ONE subdomain: U [n, L], V [n, Nw] (nloc orthonormal columns, zeros behind), dense P [n, n].
    Returns (V_new, sv [L], added)."""
    Nw = V.shape[1]
    norm0 = np.sqrt(max(np.einsum('ij,ij->j', U, P @ U).max(), 0.0))                # 1
    R = U.copy()
    for _ in range(2):                                                               # 2
        R = R - V @ (V.T @ (P @ R))
    lam, Z = np.linalg.eigh(sym(R.T @ (P @ R)))                                      # 3, 4
    order = np.argsort(-lam, kind='stable')
    lam, Z = lam[order], Z[:, order]
    sv = np.sqrt(np.maximum(lam, 0.0))
    k = int(min(np.count_nonzero(sv > max(atol, rtol * norm0)), modes, Nw - nloc))   # 5
    Vn = V.copy()
    if k > 0:
        W = R @ (Z[:, :k] / sv[:k])                                                  # 6
        W = W - V @ (V.T @ (P @ W))                                                  # 7
        l2, Z2 = np.linalg.eigh(sym(W.T @ (P @ W)))                                  # 8 (Loewdin)
        W = W @ ((Z2 / np.sqrt(l2)) @ Z2.T)
        Vn[:, nloc:nloc + k] = W                                                     # 9
    return Vn, sv, k


def local_pod_ref(U, V, nloc, P, modes, rtol=1e-6, atol=0.0):
    """The batched call: U [S, n, L], V [S (or more: halo rows are left alone), n, Nw], nloc [S], P [S, n, n].
    Returns (V_new, nloc_new, sv [S, L], added [S])."""
    S, _, L = U.shape
    Vn, sv, added = V.copy(), np.zeros((S, L)), np.zeros(S, dtype=np.int64)
    for s in range(S):
        Vn[s], sv[s], added[s] = local_pod_one(U[s], V[s], int(nloc[s]), P[s], modes, rtol, atol)
    return Vn, np.asarray(nloc[:S]) + added, sv, added


def product_svd(R, P):
    """SVD of R in the product P = C C^T: (sigma, W) with W P-orthonormal left singular vectors (the modes)."""
    C = np.linalg.cholesky(P)
    Q, sig, _ = np.linalg.svd(C.T @ R, full_matrices=False)
    return sig, sla.solve_triangular(C.T, Q, lower=False)


def deflate(U, V, P):
    R = U.copy()
    for _ in range(2):
        R = R - V @ (V.T @ (P @ R))
    return R


def orthonormality(V, nloc, P):
    """max |V^T P V - I| over the real columns."""
    worst = 0.0
    for s in range(len(nloc)):
        Vs = V[s][:, :int(nloc[s])]
        if Vs.shape[1]:
            worst = max(worst, float(np.abs(Vs.T @ (P[s] @ Vs) - np.eye(Vs.shape[1])).max()))
    return worst


def span_defect(W_ref, W, P):
    """Largest P-norm of what the columns of W_ref (P-orthonormal) leave outside span(W) (P-orthonormal): 0 = contained."""
    if W_ref.shape[1] == 0:
        return 0.0
    D = W_ref - W @ (W.T @ (P @ W_ref))
    return float(np.sqrt(np.maximum(np.einsum('ij,ij->j', D, P @ D), 0.0)).max())


def projection_error2(U, W, P):
    """sum_j |u_j - Pi u_j|_P^2 with Pi the P-orthogonal projection onto span(W), W P-orthonormal."""
    D = U - W @ (W.T @ (P @ U))
    return float(np.einsum('ij,ij->', D, P @ D))


# ---------------------------------------------------------------------------------------------------------------------------
def jacobi_eigh(G, max_sweeps=40):
    """The iteration of k_pod_eigh in NumPy: two-sided cyclic Jacobi in the round-robin ordering on sym(G) padded to an even
    order, a rotation zeroes its entry exactly and updates the two diagonal entries by the t-formulas, entries of at most
    eps |G|_F / Lp are left alone, convergence when off(G) <= eps |G|_F, tested once per sweep.
    Returns (lam descending, Z with the eigenvector of lam[j] in ROW j, sweeps, converged)."""
    L = G.shape[0]
    Lp = L + (L & 1)
    A = np.zeros((Lp, Lp))
    A[:L, :L] = 0.5 * (G + G.T)
    Zt = np.eye(Lp)
    tol2 = EPS * EPS * float((A * A).sum())
    small = np.sqrt(tol2) / Lp                     # entries below it are not rotated (all below it: converged)
    m, half = Lp - 1, Lp // 2
    converged, sweeps = False, 0
    for sweep in range(max_sweeps + 1):
        off2 = float(((A - np.diag(np.diag(A))) ** 2).sum())
        if off2 <= tol2:
            converged = True
            break
        if sweep == max_sweeps:
            break
        sweeps += 1
        for rnd in range(Lp - 1):
            k = np.arange(half)
            a = np.where(k == 0, m, (rnd + k) % m)
            c = np.where(k == 0, rnd, (rnd - k + m) % m)
            p, q = np.minimum(a, c), np.maximum(a, c)
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            nz = np.abs(apq) > small
            tau = np.where(nz, (aqq - app) / np.where(nz, 2.0 * apq, 1.0), 0.0)
            t = np.where(nz, np.where(tau >= 0.0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau)), 0.0)
            cs = 1.0 / np.sqrt(1.0 + t * t)
            sn = t * cs
            gp, gq = A[:, p].copy(), A[:, q].copy()
            A[:, p], A[:, q] = cs * gp - sn * gq, sn * gp + cs * gq
            zp, zq = Zt[p].copy(), Zt[q].copy()
            Zt[p], Zt[q] = cs[:, None] * zp - sn[:, None] * zq, sn[:, None] * zp + cs[:, None] * zq
            gp, gq = A[p].copy(), A[q].copy()
            A[p], A[q] = cs[:, None] * gp - sn[:, None] * gq, sn[:, None] * gp + cs[:, None] * gq
            A[p, p], A[q, q] = app - t * apq, aqq + t * apq
            A[p, q] = A[q, p] = 0.0
    lam = np.diag(A)[:L]
    order = np.argsort(-lam, kind='stable')
    return lam[order], Zt[order][:, :L], sweeps, converged


def eigen_matrices(L, seed=0):
    """Symmetric test matrices of order L: clustered, repeated and zero eigenvalues (name -> (matrix, eigenvalues descending))."""
    rng = np.random.default_rng(1000 * L + seed)
    Q = np.linalg.qr(rng.standard_normal((L, L)))[0]
    j = np.arange(L)
    spectra = {
        'geometric': 10.0 ** (-0.25 * j),
        'clustered': 1.0 + 1e-9 * j,
        'repeated': np.where(j < (L + 1) // 2, 2.0, 0.5),
        'zeros': np.where(j < (L + 1) // 2, 10.0 ** (-0.5 * j), 0.0),
        'near_identity': 1.0 + 1e-4 * np.cos(j),
    }
    out = {}
    for name, lam in spectra.items():
        lam = np.sort(lam)[::-1]
        out[name] = (sym((Q * lam) @ Q.T), lam)
    Z0 = np.zeros((L, L))                      # a zero row / column (a zero snapshot): an exact zero eigenvalue
    if L > 1:
        B = rng.standard_normal((L - 1, L - 1))
        Z0[1:, 1:] = sym(B @ B.T)
    out['zero_column'] = (Z0, None)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
def p_orthonormal(X, P):
    """P-orthonormal basis of span(X) (Cholesky QR, twice)."""
    for _ in range(2):
        X = X @ np.linalg.inv(np.linalg.cholesky(sym(X.T @ (P @ X))).T)
    return X


def ragged_nloc(S, Nw):
    """0, 1, an odd count, a full slab, then more of the same."""
    base = [0, 1, min(3, Nw), Nw, min(2, Nw), min(5, Nw)]
    return np.array([base[s % len(base)] for s in range(S)], dtype=np.int64)


def make_case(P, L, Nw, seed=0, nloc=None):
    """Inputs of one call for the dense products P [S, n, n]: V [S, n, Nw] with ragged nloc, snapshots U [S, n, L] that decay
    geometrically (sigma_j = 10^(-0.4 j), j < 10, the rest below 1e-9: nothing within a factor 10 of the threshold
    1e-6 norm0, 1 <= norm0 < 5) and carry an O(1) component in the span of V.  Snapshot 0 is the first mode alone.
    Returns (U, V, nloc, sigma_true [S][...])."""
    S, n = P.shape[0], P.shape[1]
    rng = np.random.default_rng(seed + 17 * L + 1000 * Nw)
    nloc = ragged_nloc(S, Nw) if nloc is None else np.asarray(nloc, dtype=np.int64)
    U, V, sig_all = np.zeros((S, n, L)), np.zeros((S, n, Nw)), []
    for s in range(S):
        r = min(L, n - int(nloc[s]))
        B = p_orthonormal(rng.standard_normal((n, int(nloc[s]) + r)), P[s])
        V[s][:, :nloc[s]] = B[:, :nloc[s]]
        j = np.arange(r)
        sig = np.where(j < 10, 10.0 ** (-0.4 * j), 1e-9 * 0.9 ** (j - 10))
        O = np.zeros((r, L))                                                     # r orthonormal rows, O[:, 0] = e_0
        if r:
            O[0, 0] = 1.0
            O[1:, 1:] = np.linalg.qr(rng.standard_normal((L - 1, r - 1)))[0].T
        U[s] = B[:, nloc[s]:] @ (sig[:, None] * O)
        if nloc[s]:
            U[s] += B[:, :nloc[s]] @ rng.uniform(0.5, 1.5, (int(nloc[s]), L))
        sig_all.append(sig)
    return U, V, nloc, sig_all


def threshold_margin(U, V, nloc, P, rtol=1e-6, atol=0.0):
    """Smallest factor between a singular value (product SVD of the deflated snapshots) and the threshold, over the subdomains."""
    worst = np.inf
    for s in range(U.shape[0]):
        norm0 = np.sqrt(np.einsum('ij,ij->j', U[s], P[s] @ U[s]).max())
        thr = max(atol, rtol * norm0)
        sig, _ = product_svd(deflate(U[s], V[s], P[s]), P[s])
        ratio = np.maximum(sig / thr, thr / np.maximum(sig, 1e-300))
        worst = min(worst, float(ratio.min()))
    return worst


def spd_products(S, n, seed=0):
    """Dense SPD stand-ins for the local product (host tests): a 1D stiffness-like matrix plus a random SPD perturbation."""
    rng = np.random.default_rng(seed)
    P = np.zeros((S, n, n))
    for s in range(S):
        T = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
        B = rng.standard_normal((n, n)) / np.sqrt(n)
        P[s] = T + 0.1 * np.eye(n) + 0.05 * sym(B @ B.T)
    return P
