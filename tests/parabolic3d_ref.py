"""CPU reference of the parabolic 3D / P2 path: a restatement of oracle/parabolic.py (OracleParabolic, OracleParabolicReduced;
reference estimators.py:141-168 and pyMOR's implicit Euler) on top of the 3D oracle ``oracle.lrbms3d.Discretization3D``
(``system_matrix(mu)``, ``M``, ``b``, ``local_terms``) and ``Reductor3D``.  Test infrastructure only."""
import numpy as np
import scipy.sparse.linalg as spla

from oracle.lrbms3d import Reductor3D


def combine(o, mu, dt, nc, r, df, tr2, tdnc2):
    """estimators.py:99-102, :146-166 from squared local terms nc / r / df [S, L], time residuals [L - 1], nc of dU [S, L - 1]."""
    a_bar, g_bar, a_hat = o.alpha(mu, o.mu_bar), o.gamma(mu, o.mu_bar), o.alpha(mu, o.mu_hat)
    eta = (np.sqrt(g_bar) * np.linalg.norm(nc, axis=0) + (1.0 / np.sqrt(a_hat)) * np.linalg.norm(r + df, axis=0)) / np.sqrt(a_bar)
    time_residual = np.sqrt(np.asarray(tr2) * dt / 3)
    s = 2 * np.sqrt(dt / 3)
    eta, nc, r, df = eta * s, nc * s, r * s, df * s
    time_deriv_nc = np.sqrt(np.maximum(tdnc2, 0.0) / dt)
    est = np.linalg.norm(eta) + np.linalg.norm(time_residual) + np.linalg.norm(time_deriv_nc)
    return est, (nc, r, df, time_residual, time_deriv_nc)


class Parabolic3D:
    """Full order: (M + dt A(mu)) U_{k+1} = M U_k + dt b; U [nt + 1, S, n]."""

    def __init__(self, o, T, nt):
        self.o, self.T, self.nt = o, float(T), int(nt)
        self.dt = self.T / self.nt

    def solve(self, mu, U0=None):
        o = self.o
        lu = spla.splu((o.M + self.dt * o.system_matrix(mu)).tocsc())
        U = np.zeros((self.nt + 1, o.ndof))
        if U0 is not None:
            U[0] = np.asarray(U0).reshape(-1)
        for k in range(self.nt):
            U[k + 1] = lu.solve(o.M @ U[k] + self.dt * o.b)
        return U.reshape(self.nt + 1, o.S, o.n)

    def time_residual2(self, dU, mu):
        """y^T M^-1 y with y = A(mu) dU_k, summed over the subdomains: [len(dU)]."""
        o = self.o
        A = o.system_matrix(mu)
        lu = spla.splu(o.M.tocsc())
        out = []
        for v in np.asarray(dU).reshape(len(dU), -1):
            y = A @ v
            out.append(lu.solve(y) @ y)
        return np.array(out)

    def estimate(self, U, mu):
        o = self.o
        U = np.asarray(U).reshape(len(U), -1)
        terms = np.array([o.local_terms(U[k], mu) for k in range(len(U))])        # [L, 3, S]
        dU = U[1:] - U[:-1]
        tdnc2 = np.array([o.local_terms(v, mu)[0] for v in dU]).T
        return combine(o, mu, self.dt, terms[:, 0].T, terms[:, 1].T, terms[:, 2].T, self.time_residual2(dU, mu), tdnc2)


class ParabolicReduced3D:
    """Reduced model on local bases (list of [n, N_s]): the Galerkin projections of A, M, b; u [nt + 1, sum N_s]."""

    def __init__(self, o, bases, T, nt):
        self.o, self.T, self.nt = o, float(T), int(nt)
        self.dt = self.T / self.nt
        self.bases = [np.asarray(b) for b in bases]
        self.rd = Reductor3D(o, self.bases).reduce()
        self.off = np.concatenate([[0], np.cumsum([b.shape[1] for b in self.bases])])
        Mt = o.M.tocsr()
        self.M_blocks = [b.T @ (Mt[o.dofs_of(ii)][:, o.dofs_of(ii)] @ b) for ii, b in enumerate(self.bases)]

    def matrices(self, mu):
        o, off = self.o, self.off
        th = o.theta(mu)
        A, M = np.zeros((off[-1], off[-1])), np.zeros((off[-1], off[-1]))
        for ii in range(o.S):
            M[off[ii]:off[ii + 1], off[ii]:off[ii + 1]] = self.M_blocks[ii]
            for jj, blocks in self.rd.op[ii].items():
                A[off[ii]:off[ii + 1], off[jj]:off[jj + 1]] = sum(t * B for t, B in zip(th, blocks))
        return A, M, np.concatenate(self.rd.rhs)

    def solve(self, mu):
        A, M, b = self.matrices(mu)
        u = np.zeros((self.nt + 1, self.off[-1]))
        for k in range(self.nt):
            u[k + 1] = np.linalg.solve(M + self.dt * A, M @ u[k] + self.dt * b)
        return u

    def split(self, v):
        return [v[self.off[ii]:self.off[ii + 1]] for ii in range(self.o.S)]

    def estimate(self, u, mu):
        A, M, _ = self.matrices(mu)
        terms = np.array([self.rd.local_terms(self.split(uk), mu) for uk in u])      # [L, 3, S]
        du = u[1:] - u[:-1]
        tdnc2 = np.array([self.rd.local_terms(self.split(v), mu)[0] for v in du]).T
        tr2 = np.array([np.linalg.solve(M, A @ v) @ (A @ v) for v in du])
        return combine(self.o, mu, self.dt, terms[:, 0].T, terms[:, 1].T, terms[:, 2].T, tr2, tdnc2)
