"""A plain NumPy / SciPy PCG and the preconditioners of the product's solvers, restated from the kernels.

The k-th PCG iterate from x_0 = 0 is the A-norm minimiser over the Krylov space K_k(M^-1 A, M^-1 b): it does not depend on
how a PCG variant arranges its recurrences, but it does depend on M.  Every solver export honours ``max_iter`` exactly and
leaves the k-th iterate in its output with info = (k, |r_k| / |r_0|) (pylrbms_amd/csrc/online.hip ``red_cg_run`` and
``reduced_solve_batch_drive``, fom.hip ``fom_cg_run``), so ``pcg_iterate`` with the same A and the same M, stopped at k, is an
exact reference for the whole iteration: matvec, update, the inverse diagonal blocks, the coarse inverse and the coarse apply.

The operators are built from arrays the product computed (B_sys of the fused pass, A_diag / A_cpl of the assembly); those
are pinned to the oracle elsewhere, so the tests on top of this file test the solvers alone."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

COARSE_S_MIN, COARSE_S_MAX = 4, 4096      # online.hip coarse_begin: no coarse level outside 4 <= S <= 4096


def pcg_iterate(apply_A, apply_Minv, b, k):
    """Textbook PCG from x_0 = 0, stopped after k iterations.  ``b`` [n] or [n, m] (independent columns; a zero column stays
    zero).  -> (x_k of the shape of b, |r_k| / |r_0| per column: a float for a 1-D b, [m] otherwise)."""
    b = np.asarray(b, dtype=np.float64)
    one = b.ndim == 1
    B = b[:, None] if one else b
    x = np.zeros_like(B)
    r = B.copy()
    z = apply_Minv(r)
    p = z.copy()
    rz = np.einsum('ij,ij->j', r, z)
    for _ in range(k):
        Ap = apply_A(p)
        pAp = np.einsum('ij,ij->j', p, Ap)
        alpha = np.divide(rz, pAp, out=np.zeros_like(rz), where=pAp != 0.0)
        x += alpha * p
        r -= alpha * Ap
        z = apply_Minv(r)
        rz_new = np.einsum('ij,ij->j', r, z)
        beta = np.divide(rz_new, rz, out=np.zeros_like(rz), where=rz != 0.0)
        p = z + beta * p
        rz = rz_new
    n0 = np.linalg.norm(B, axis=0)
    rel = np.divide(np.linalg.norm(r, axis=0), n0, out=np.zeros_like(n0), where=n0 > 0.0)
    return (x[:, 0], float(rel[0])) if one else (x, rel)


def _as2d(fn):
    """Wrap a preconditioner written for [n, m] so that it also takes [n]."""
    def apply(r):
        return fn(r[:, None])[:, 0] if r.ndim == 1 else fn(r)
    return apply


def _coarse_factor(A0):
    """Cholesky factor of the coarse matrix (sparse or dense), or None if it is not positive definite -- the product then
    runs without a coarse level (online.hip coarse_finish: the pivot flag of k_bt_factor / the info of rocsolver_dpotrf)."""
    A0 = A0.toarray() if sp.issparse(A0) else np.asarray(A0)
    try:
        return sla.cho_factor(A0, lower=True)
    except np.linalg.LinAlgError:
        return None


# --------------------------------------------------------------------------------------------------------- 2D reduced
def combine_reduced(B_sys, theta):
    """A(theta) in the fixed-slot layout: Amu [S, 5, N, N] = sum_q theta_q B_sys[q] (online.hip k_assemble_mu)."""
    return np.einsum('q,qsaij->saij', np.asarray(theta, dtype=np.float64), np.asarray(B_sys, dtype=np.float64))


def reduced_operator(Amu, nbr):
    """Sparse [S N, S N] operator of the reduced solvers: block row s holds Amu[s, slot] in block column nbr[s, slot]
    (online.hip k_cg2_matvec: y_s = sum_slot Amu[s][slot] p_nbr(s, slot))."""
    S, _, N, _ = Amu.shape
    nbr = np.asarray(nbr)
    s_idx, slot = np.nonzero(nbr >= 0)
    t_idx = nbr[s_idx, slot]
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
    rows = (s_idx[:, None, None] * N + ii[None]).ravel()
    cols = (t_idx[:, None, None] * N + jj[None]).ravel()
    vals = Amu[s_idx, slot].ravel()
    return sp.csr_matrix((vals, (rows, cols)), shape=(S * N, S * N))


def reduced_block_jacobi(Amu_diag):
    """D^-1 [S, N, N]: the inverse of every diagonal block, where an exactly zero diagonal entry (a zero-padded basis column)
    becomes 1 first (online.hip k_block_inverse, :218-225), so that the padded unknown decouples and stays 0."""
    D = np.array(Amu_diag, dtype=np.float64, copy=True)
    S, N, _ = D.shape
    d = D[:, np.arange(N), np.arange(N)]
    d[d == 0.0] = 1.0
    D[:, np.arange(N), np.arange(N)] = d
    return np.linalg.inv(D)


def reduced_coarse_matrix(Amu, nbr):
    """A0 [S, S] (sparse): A0[s, t] = entry (0, 0) of block [s][slot] with t = nbr[s, slot] (online.hip k_coarse_entries)."""
    S = Amu.shape[0]
    nbr = np.asarray(nbr)
    s_idx, slot = np.nonzero(nbr >= 0)
    return sp.csr_matrix((Amu[s_idx, slot, 0, 0], (s_idx, nbr[s_idx, slot])), shape=(S, S))


class ReducedPrecond:
    """M^-1 r = D^-1 r + R0^T A0^-1 R0 r with (R0 r)_s = r[s][0] (online.hip k_cg2_update + k_coarse_apply(1)).
    The coarse level exists if ``coarse`` != 0, 4 <= S <= 4096 and A0 is positive definite."""

    def __init__(self, Amu, nbr, coarse=1):
        self.S, self.N = Amu.shape[0], Amu.shape[2]
        self.Dinv = reduced_block_jacobi(Amu[:, 2])
        self.A0 = None
        self.cho = None
        if coarse != 0 and COARSE_S_MIN <= self.S <= COARSE_S_MAX:
            self.A0 = reduced_coarse_matrix(Amu, nbr)
            self.cho = _coarse_factor(self.A0)
        self.apply = _as2d(self._apply)

    @property
    def has_coarse(self):
        return self.cho is not None

    def _apply(self, r):
        S, N, m = self.S, self.N, r.shape[1]
        z = np.einsum('sij,sjm->sim', self.Dinv, r.reshape(S, N, m))
        if self.cho is not None:
            z[:, 0, :] += sla.cho_solve(self.cho, r.reshape(S, N, m)[:, 0, :])
        return z.reshape(S * N, m)


# ------------------------------------------------------------------------------------------------------ 2D full order
def blockell_operator(vals, template):
    """Block-diagonal sparse [S n, S n] matrix of per-subdomain block-ELL values vals [S, n_T, 4, 9] (block 0: the element's
    own 3 x 3 block, 1 + f: its face neighbour nb_elem[e, f] inside the subdomain; the layout of ``blockell_to_dense``,
    pylrbms_amd/engine.py), built sparse for all subdomains at once."""
    t = template
    V = np.asarray(vals, dtype=np.float64).reshape(-1, t.n_T, 4, 3, 3)
    S, n = V.shape[0], t.n
    ii, jj = np.meshgrid(np.arange(3), np.arange(3), indexing='ij')
    e = np.arange(t.n_T)
    rows, cols, data = [], [], []
    for b in range(4):
        nb = e if b == 0 else np.asarray(t.nb_elem)[:, b - 1]
        ok = nb >= 0
        base = np.arange(S)[:, None] * n
        rows.append(((base + 3 * e[ok][None, :])[:, :, None, None] + ii).ravel())
        cols.append(((base + 3 * nb[ok][None, :])[:, :, None, None] + jj).ravel())
        data.append(V[:, ok, b].ravel())
    return sp.csr_matrix((np.concatenate(data), (np.concatenate(rows), np.concatenate(cols))), shape=(S * n, S * n))


def fom_operator(A_diag, A_cpl, theta, template, nbr):
    """Sparse [S n, S n] full-order operator sum_q theta_q A_q: A_diag [Q, S, n_T, 4, 9] as in ``blockell_operator``,
    A_cpl [Q, S, 4, ncf, 9] (rows: side_elem[side, p] of s, columns: side_elem_out[side, p] of the neighbour on that side,
    the layout of ``coupling_to_dense``)."""
    t = template
    th = np.asarray(theta, dtype=np.float64)
    A = blockell_operator(np.einsum('q,qsebk->sebk', th, np.asarray(A_diag)), t)
    Ac = np.einsum('q,qsfpk->sfpk', th, np.asarray(A_cpl)).reshape(-1, 4, t.ncf, 3, 3)
    S, n = Ac.shape[0], t.n
    ii, jj = np.meshgrid(np.arange(3), np.arange(3), indexing='ij')
    rows, cols, data = [], [], []
    for side, slot in enumerate((0, 1, 3, 4)):
        cnt = int(t.side_count[side])
        ei = np.asarray(t.side_elem)[side, :cnt]
        eo = np.asarray(t.side_elem_out)[side, :cnt]
        for s in range(S):
            s2 = int(nbr[s][slot])
            if s2 < 0 or cnt == 0:
                continue
            rows.append((s * n + 3 * ei[:, None, None] + ii).ravel())
            cols.append((s2 * n + 3 * eo[:, None, None] + jj).ravel())
            data.append(Ac[s, side, :cnt].ravel())
    if rows:
        A = A + sp.csr_matrix((np.concatenate(data), (np.concatenate(rows), np.concatenate(cols))), shape=(S * n, S * n))
    return A.tocsr()


class FomPrecond:
    """Preconditioner of lrbms_fom_solve (fom.hip): Minv = the inverse of every diagonal 3 x 3 element block of A(mu)
    (k_fom_combine), plus the coarse level on the subdomain indicator functions: A0 = R0 A R0^T, i.e. A0[s, t] = 1^T A_st 1
    (k_fom_coarse_entries), R0 sums a subdomain's DoFs (k_fom_restrict / the wave sums of k_fom_cg_update + k_fom_coarse1),
    and z += R0^T A0^-1 R0 r.  Built from any sparse global A with ``S`` subdomains of ``n`` DoFs each."""

    def __init__(self, A, S, n, coarse=1):
        A = sp.csr_matrix(A)
        self.S, self.n = S, n
        e3 = 3 * np.arange(S * n // 3)
        blocks = np.empty((e3.size, 3, 3))
        for i in range(3):
            for j in range(3):
                blocks[:, i, j] = np.asarray(A[e3 + i, e3 + j]).ravel()
        self.Minv = np.linalg.inv(blocks)
        self.cho = None
        if coarse != 0 and COARSE_S_MIN <= S <= COARSE_S_MAX:
            R0 = sp.kron(sp.identity(S, format='csr'), np.ones((1, n)), format='csr')
            self.A0 = (R0 @ A @ R0.T).toarray()
            self.cho = _coarse_factor(self.A0)
        self.apply = _as2d(self._apply)

    @property
    def has_coarse(self):
        return self.cho is not None

    def _apply(self, r):
        m = r.shape[1]
        z = np.einsum('eij,ejm->eim', self.Minv, r.reshape(-1, 3, m)).reshape(-1, m)
        if self.cho is not None:
            c = sla.cho_solve(self.cho, r.reshape(self.S, self.n, m).sum(axis=1))
            z = (z.reshape(self.S, self.n, m) + c[:, None, :]).reshape(-1, m)
        return z


def precond_matrix(apply_Minv, n):
    """Dense M^-1 [n, n] of a preconditioner (host tests on small problems)."""
    return apply_Minv(np.eye(n))


def spd_check(M):
    """Smallest eigenvalue of the symmetric part and the asymmetry of a dense matrix."""
    M = np.asarray(M)
    sym = 0.5 * (M + M.T)
    return float(np.linalg.eigvalsh(sym).min()), float(np.abs(M - M.T).max() / np.abs(M).max())

