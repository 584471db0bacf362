"""NumPy restatement of lrbms_fom_solve_batch (pylrbms_amd/csrc/fom.hip) on top of tests/pcg_ref.py.

Column m of a call solves A(theta_m) x_m = sum_j phi[m][j] b_K[j] from x = 0 by PCG with

    M_m^-1 = blockdiag_3x3(A(theta_m))^-1 + R0^T (R0 A(theta_bar) R0^T)^-1 R0,

theta_bar[q] = (1 / nmu) sum_m theta[m][q]: the inverse element blocks are the column's own, the coarse level on the
subdomain indicator functions is built once per call at the mean theta.  Without a coarse level (``coarse`` 0, S outside
4..4096, A0 not positive definite) the element blocks run alone."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import pcg_ref


class BatchFomPrecond:
    """The preconditioner of one column: ``Minv`` from A_col = A(theta_m), the Cholesky factor of R0 A_bar R0^T with
    A_bar = A(theta_bar).  For A_bar = A_col it is ``pcg_ref.FomPrecond``."""

    def __init__(self, A_col, A_bar, S, n, coarse=1):
        self.S, self.n = S, n
        self.Minv = np.linalg.inv(pcg_ref.diagonal_blocks(A_col, 3))
        self.A0 = None
        self.cho = None
        if coarse != 0 and pcg_ref.COARSE_S_MIN <= S <= pcg_ref.COARSE_S_MAX:
            R0 = sp.kron(sp.identity(S, format='csr'), np.ones((1, n)), format='csr')
            self.A0 = (R0 @ sp.csr_matrix(A_bar) @ R0.T).toarray()
            self.cho = pcg_ref._coarse_factor(self.A0)
        self.apply = pcg_ref._as2d(self._apply)

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


def mean_theta(thetas):
    """theta_bar of a call: summed in column order, then divided by nmu."""
    thetas = np.asarray(thetas, dtype=np.float64)
    acc = np.zeros(thetas.shape[1])
    for row in thetas:
        acc = acc + row
    return acc / thetas.shape[0]


class BatchFomRef:
    """Operators, right-hand sides and preconditioners of one call: thetas [nmu, Q], phi [nmu, K], b_K [K, S, n].
    ``coarse_theta``: where the coarse level is built (default: the call mean, as the product does)."""

    def __init__(self, A_diag, A_cpl, template, nbr, thetas, phi, b_K, coarse=1, coarse_theta=None):
        self.thetas = np.asarray(thetas, dtype=np.float64)
        self.nmu = self.thetas.shape[0]
        S, n = np.asarray(A_diag).shape[1], template.n
        self.S, self.n = S, n
        Q = self.thetas.shape[1]
        Aq = [pcg_ref.fom_operator(A_diag, A_cpl, np.eye(Q)[q], template, nbr) for q in range(Q)]      # the components, once

        def combine(th):
            A = float(th[0]) * Aq[0]
            for q in range(1, Q):
                A = A + float(th[q]) * Aq[q]
            return A.tocsr()
        self.As = [combine(th) for th in self.thetas]
        tb = mean_theta(self.thetas) if coarse_theta is None else np.asarray(coarse_theta, dtype=np.float64)
        self.A_bar = combine(tb)
        self.Ms = [BatchFomPrecond(A, self.A_bar, S, n, coarse) for A in self.As]
        K = np.asarray(b_K).shape[0]
        self.cols = np.einsum('mk,kn->nm', np.asarray(phi, dtype=np.float64), np.asarray(b_K, dtype=np.float64).reshape(K, -1))

    @property
    def has_coarse(self):
        return self.Ms[0].has_coarse

    def iterate(self, k):
        """The ``reference(k)`` of ``check_iterates``: (X_k [S n, nmu], ratios [nmu])."""
        out = [pcg_ref.pcg_iterate(lambda p, A=A: A @ p, M.apply, self.cols[:, j], k)
               for j, (A, M) in enumerate(zip(self.As, self.Ms))]
        return np.stack([x for x, _ in out], axis=1), np.array([r for _, r in out])

    def solve(self, j):
        from scipy.sparse.linalg import spsolve
        return spsolve(self.As[j].tocsc(), self.cols[:, j])
