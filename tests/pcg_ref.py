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



# ------------------------------------------------------------------------------------------- neighbourhood correctors
SIDE_TO_SLOT_2D = (0, 1, 3, 4)            # csrc/lrbms_dev.h side_to_slot


def diagonal_blocks(A, bs):
    """The bs x bs diagonal blocks [n / bs, bs, bs] of a sparse matrix."""
    A = sp.csr_matrix(A)
    first = bs * np.arange(A.shape[0] // bs)
    blocks = np.empty((first.size, bs, bs))
    for i in range(bs):
        for j in range(bs):
            blocks[:, i, j] = np.asarray(A[first + i, first + j]).ravel()
    return blocks


def block_jacobi(Minv):
    """z = M^-1 r for the inverse diagonal blocks Minv [nb, bs, bs]; takes r [n] or [n, m]."""
    bs = Minv.shape[1]
    return _as2d(lambda r: np.einsum('eij,ejm->eim', Minv, r.reshape(-1, bs, r.shape[1])).reshape(-1, r.shape[1]))


def hood_operator_2d(A_diag, A_cpl, D_corr, theta, template, nbr, ii):
    """The operator of the corrector problem of subdomain ii (enrich.hip ``hood_block``, restated block by block) from the
    assembled arrays A_diag [Q, S, n_T, 4, 9], A_cpl / D_corr [Q, S, 4, ncf, 9] -> (A csr on the present members of N(ii) in slot
    order, dofs: the index of every row in the [S, n] numbering -- ``dofs // n == ii`` picks the own part).

    Member in slot s (subdomain kk = nbr[ii, s]), element e: block 0 is the diagonal block, block 1 + f the one of the element
    across face f inside kk.  Across a side face: the centre (s == 2) couples through A_cpl with every member it has (a physical
    side has none: its boundary term is in A_diag already), another member couples with the centre only (side slot == 4 - s).
    Every other side face of a non-centre member that has a subdomain behind it (nbr[kk, side slot] >= 0) lies on the outer
    boundary of N(ii): D_corr is added to the element's diagonal block; nothing is added on physical sides."""
    t = template
    nT, n = t.n_T, t.n
    th = np.asarray(theta, dtype=np.float64)
    nbr = np.asarray(nbr)
    Ad = np.einsum('q,qsebk->sebk', th, np.asarray(A_diag, dtype=np.float64)).reshape(-1, nT, 4, 3, 3)
    Ac = np.einsum('q,qsfpk->sfpk', th, np.asarray(A_cpl, dtype=np.float64)).reshape(-1, 4, t.ncf, 3, 3)
    Dc = np.einsum('q,qsfpk->sfpk', th, np.asarray(D_corr, dtype=np.float64)).reshape(-1, 4, t.ncf, 3, 3)
    slots = [s for s in range(5) if nbr[ii, s] >= 0]
    where = {s: k for k, s in enumerate(slots)}
    nb_elem, pos, out = np.asarray(t.nb_elem), np.asarray(t.elem_side_pos), np.asarray(t.nb_elem_out)
    ii3, jj3 = np.meshgrid(np.arange(3), np.arange(3), indexing='ij')
    e = np.arange(nT)
    rows, cols, data = [], [], []

    def put(member, er, col_member, ec, blocks):
        rows.append((where[member] * n + 3 * er[:, None, None] + ii3).ravel())
        cols.append((where[col_member] * n + 3 * ec[:, None, None] + jj3).ravel())
        data.append(blocks.ravel())

    for s in slots:
        kk = int(nbr[ii, s])
        put(s, e, s, e, Ad[kk, :, 0])
        for f in range(3):
            inner = nb_elem[:, f] >= 0
            put(s, e[inner], s, nb_elem[inner, f], Ad[kk, inner, 1 + f])
            for side in range(4):
                on = nb_elem[:, f] == -(1 + side)
                if not on.any():
                    continue
                s2 = SIDE_TO_SLOT_2D[side]
                if s == 2 and nbr[ii, s2] >= 0:
                    put(s, e[on], s2, out[on, f], Ac[kk, side, pos[on, f]])
                elif s != 2 and s2 == 4 - s:
                    put(s, e[on], 2, out[on, f], Ac[kk, side, pos[on, f]])
                elif s != 2 and nbr[kk, s2] >= 0:
                    put(s, e[on], s, e[on], Dc[kk, side, pos[on, f]])
    m = len(slots) * n
    A = sp.csr_matrix((np.concatenate(data), (np.concatenate(rows), np.concatenate(cols))), shape=(m, m))
    dofs = np.concatenate([int(nbr[ii, s]) * n + np.arange(n) for s in slots])
    return A, dofs


def hood_block_jacobi_2d(A_hood):
    """Minv [5 n_T', 3, 3] of k_hood_pcg: the inverse (``inv3``) of every 3 x 3 diagonal block of the corrected neighbourhood
    operator -- D_corr on the non-centre members included."""
    return np.linalg.inv(diagonal_blocks(A_hood, 3))


def hood_block_jacobi_3d(A_sys, dofs):
    """Minv [n_el, 10, 10] of lrbms3_local_correction_solve: the inverse of every 10 x 10 element diagonal block of the
    UNCORRECTED system matrix (k3f_block_inverse on the combined A_diag; one inverse per element for all problems) on the rows
    ``dofs`` of a neighbourhood (whole elements)."""
    first = np.asarray(dofs).reshape(-1, 10)[:, 0]
    A = sp.csr_matrix(A_sys)
    blocks = np.empty((first.size, 10, 10))
    for i in range(10):
        for j in range(10):
            blocks[:, i, j] = np.asarray(A[first + i, first + j]).ravel()
    return np.linalg.inv(blocks)


def pcg_history(apply_A, apply_Minv, b, kmax):
    """The iterates x_1 .. x_kmax of ``pcg_iterate`` for one right-hand side b [n] in one sweep -> (X [kmax, n], ratios
    [kmax]); row k - 1 is x_k, by the recurrences of ``pcg_iterate``."""
    b = np.asarray(b, dtype=np.float64)
    x, r = np.zeros_like(b), b.copy()
    z = apply_Minv(r)
    p, rz, n0 = z.copy(), float(r @ z), float(np.linalg.norm(b))
    X, ratios = np.empty((kmax, b.size)), np.empty(kmax)
    for k in range(kmax):
        Ap = apply_A(p)
        pAp = float(p @ Ap)
        alpha = rz / pAp if pAp != 0.0 else 0.0
        x = x + alpha * p
        r = r - alpha * Ap
        z = apply_Minv(r)
        rz_new = float(r @ z)
        beta = rz_new / rz if rz != 0.0 else 0.0
        p = z + beta * p
        rz = rz_new
        X[k], ratios[k] = x, (np.linalg.norm(r) / n0 if n0 > 0.0 else 0.0)
    return X, ratios


class CorrectorRef:
    """One corrector problem for the iterate tests: operator A (sparse) and load b on the neighbourhood, ``own`` (the rows of
    the marked subdomain: what the solver exports return) and the inverse diagonal blocks Minv of its preconditioner."""

    def __init__(self, A, b, own, Minv):
        self.A, self.b, self.own, self.Minv = sp.csr_matrix(A), np.asarray(b, dtype=np.float64), own, Minv
        self._hist = {}

    def history(self, kmax, Minv=None):
        """(x_k restricted to ``own`` [kmax, n], ratios [kmax]) with the cell's preconditioner, or with another one (Minv: inverse
        diagonal blocks, or None inside a 1-tuple for the identity)."""
        if Minv is None:
            if self._hist.get('kmax', 0) < kmax:
                X, ratios = pcg_history(lambda v: self.A @ v, block_jacobi(self.Minv), self.b, kmax)
                self._hist = {'kmax': kmax, 'X': X[:, self.own], 'ratios': ratios}
            return self._hist['X'][:kmax], self._hist['ratios'][:kmax]
        apply = (lambda r: r) if Minv[0] is None else block_jacobi(Minv)
        X, ratios = pcg_history(lambda v: self.A @ v, apply, self.b, kmax)
        return X[:, self.own], ratios

    def iterate(self, k):
        """The ``reference(k)`` of ``check_iterates``: (x_k on ``own`` [n, 1], ratio [1])."""
        X, ratios = self.history(k)
        return X[k - 1][:, None], ratios[k - 1:k]

    def stop(self, rtol, cap=2000):
        """(j, ratios [j]): the first iteration j with |r_j| / |b| <= rtol, as every solver export stops."""
        kmax = 16
        while True:
            _, ratios = self.history(kmax)
            hit = np.nonzero(ratios <= rtol)[0]
            if hit.size:
                return int(hit[0]) + 1, ratios[:hit[0] + 1]
            assert kmax < cap, 'no iterate below rtol within {} iterations'.format(cap)
            kmax *= 2

    def solve(self):
        from scipy.sparse.linalg import spsolve
        return spsolve(self.A.tocsc(), self.b)[self.own]
