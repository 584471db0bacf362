"""NumPy / SciPy restatement of lrbms3_fom_implicit_euler_batch (pylrbms_amd/csrc/lrbms3d.hip) on top of
tests/fom_batch3d_ref.py, tests/pcg3d_ref.py and tests/pcg_ref.py.

Column m of a call runs the implicit Euler

    (M + dt A(theta_m)) u_{k+1} = M u_k + dt sum_j phi[m][k+1][j] b_K[j],     k = 0 .. nt-1,

with M the P2 DG mass (element-block-diagonal: the table TM of the element's type; ``mass_from_tables``, or the oracle's through
``pcg3d_ref.oracle_mass``) and A from ``fom_batch3d_ref.component_operators``.  Every step is a PCG from the warm start x = u_k
with ONE preconditioner per call,

    P^-1 = blockdiag_10(M + dt A(theta_bar))^-1 + R0^T (R0 (M + dt A(theta_bar)) R0^T)^-1 R0,

``fom_batch3d_ref.BatchFomPrecond3D`` with both levels on the step operator at the call mean theta_bar (summed in column order).
The ratio of an iterate is relative to the step's full right-hand side |M u_k + dt sum_j phi b_j|: ``pcg_iterate`` on the start
residual r_0, rescaled by |r_0| / |f| as ``pcg3d_ref.fom_euler_step`` does.  The dense reference solves every step directly."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu

import fom_batch3d_ref as ref3
import pcg_ref


def mass_from_tables(TM, elem_type, S):
    """Sparse [S n, S n] mass in the product's layout: per subdomain the blocks TM[elem_type[e]] [10, 10] on the diagonal."""
    TM = np.asarray(TM, dtype=np.float64).reshape(-1, 10, 10)
    one = sp.block_diag([TM[int(ty)] for ty in np.asarray(elem_type)], format='csr')
    return sp.kron(sp.identity(S, format='csr'), one, format='csr')


class BatchFomEuler3DRef:
    """One call: components ``Aq`` (sparse), mass ``M`` (sparse), thetas [nmu, Q], phis [nmu, nt + 1, K], b_K [K, S, n],
    U0 [S n] or [S n, nmu] (default 0), ``Phi`` [n, nc] the coarse functions (None: element blocks alone).  Switches for the mutant
    references: ``coarse`` 0 (no coarse level), ``coarse_theta`` (where the coarse level is built; default the call mean),
    ``mass_in_blocks`` False (inverse element blocks of dt A(theta_bar) alone)."""

    def __init__(self, Aq, M, S, n, thetas, dt, nt, phis, b_K, U0=None, Phi=None, coarse=1, coarse_theta=None, mass_in_blocks=True):
        self.thetas = np.asarray(thetas, dtype=np.float64)
        self.nmu, self.S, self.n, self.dt, self.nt = self.thetas.shape[0], S, n, float(dt), int(nt)
        self.M = sp.csr_matrix(M)
        self.As = [(self.M + self.dt * ref3.combine(Aq, th)).tocsr() for th in self.thetas]              # the step operators
        tb = ref3.mean_theta(self.thetas)
        dtA_bar = (self.dt * ref3.combine(Aq, tb)).tocsr()
        self.A_bar = (self.M + dtA_bar).tocsr()
        A_crs = self.A_bar if coarse_theta is None else (self.M + self.dt * ref3.combine(Aq, coarse_theta)).tocsr()
        self.P = ref3.BatchFomPrecond3D(self.A_bar if mass_in_blocks else dtA_bar, A_crs, S, n, Phi, coarse)
        self.Ms = [self.P] * self.nmu
        self.phis = np.asarray(phis, dtype=np.float64)
        K = np.asarray(b_K).shape[0]
        assert self.phis.shape == (self.nmu, self.nt + 1, K), self.phis.shape
        self.b_K = np.asarray(b_K, dtype=np.float64).reshape(K, S * n)
        U0 = np.zeros((S * n, self.nmu)) if U0 is None else np.asarray(U0, dtype=np.float64).reshape(S * n, -1)
        self.U0 = np.ascontiguousarray(np.broadcast_to(U0, (S * n, self.nmu)))
        self._traj = None

    @property
    def has_coarse(self):
        return self.P.has_coarse

    def rhs(self, m, k, uk):
        """The full right-hand side of step k (0-based) of column m: M u_k + dt sum_j phi[m][k + 1][j] b_K[j]."""
        return self.M @ uk + self.dt * (self.phis[m, k + 1] @ self.b_K)

    def trajectories(self):
        """Dense reference [nt + 1, S n, nmu]: one direct solve per step and column."""
        if self._traj is None:
            U = np.zeros((self.nt + 1, self.S * self.n, self.nmu))
            U[0] = self.U0
            for m, A in enumerate(self.As):
                lu = splu(A.tocsc())
                for k in range(self.nt):
                    U[k + 1, :, m] = lu.solve(self.rhs(m, k, U[k, :, m]))
            self._traj = U
        return self._traj

    def iterate(self, k, step=0, Uk=None):
        """The ``reference(k)`` of ``check_iterates`` for one step (default the first, from U0; ``Uk`` [S n, nmu]: the start values of
        step ``step``): (x_k - u [S n, nmu], |r_k| / |M u + dt sum phi b| [nmu]) of the PCG from the warm start -- ``pcg_iterate`` on
        the start residual, the ratio rescaled to the full right-hand side.  A column with a zero right-hand side: zeros, ratio 0."""
        Uk = self.U0 if Uk is None else np.asarray(Uk, dtype=np.float64).reshape(self.S * self.n, self.nmu)
        X, ratios = np.zeros((self.S * self.n, self.nmu)), np.zeros(self.nmu)
        for m, A in enumerate(self.As):
            f = self.rhs(m, step, Uk[:, m])
            r0 = f - A @ Uk[:, m]
            nf = np.linalg.norm(f)
            if nf == 0.0 or not r0.any():
                continue                                                    # no say (u_{k+1} = u_k), or nothing to do
            X[:, m], rel = pcg_ref.pcg_iterate(lambda p, A=A: A @ p, self.P.apply, r0, k)
            ratios[m] = rel * np.linalg.norm(r0) / nf
        return X, ratios

    def column_errors(self, U):
        """max |U - U_ref| / max |U_ref| per (step >= 1, column) of U [nt + 1, S n, nmu] against the dense reference -> [nt, nmu]."""
        U, U_ref = np.asarray(U).reshape(self.nt + 1, -1, self.nmu), self.trajectories()
        num = np.abs(U[1:] - U_ref[1:]).max(axis=1)
        den = np.abs(U_ref[1:]).max(axis=1)
        return num / np.where(den > 0.0, den, 1.0)

    def true_residuals(self, U):
        """|(M + dt A_m) u_{k+1} - f| / |f|, f = M u_k + dt sum_j phi b_j, for every step and column of U [nt + 1, S n, nmu] -> [nt, nmu]
        (the plain norm where f is zero)."""
        U = np.asarray(U).reshape(self.nt + 1, -1, self.nmu)
        out = np.zeros((self.nt, self.nmu))
        for m, A in enumerate(self.As):
            for k in range(self.nt):
                f = self.rhs(m, k, U[k, :, m])
                nf = np.linalg.norm(f)
                out[k, m] = np.linalg.norm(A @ U[k + 1, :, m] - f) / nf if nf > 0.0 else np.linalg.norm(A @ U[k + 1, :, m])
        return out


# ------------------------------------------------------------------------------------------------ the cells of the tests
DT = 0.05                                 # the step of tests/test_pcg_iterates3d_gpu.py
SWEEP = 'q3_2x1x2'
CELL_PROBLEMS = (SWEEP, 'q1_strip', 'interior_3x3x3', 'kc_3x1x2', 'aniso_2x2x1')
NMU = 17
U0_SEED = 11
U0_RATIO = 1.65                           # max |u_0| / max |x_1| of a column stays below this (worst cell: 1.602): U[1] - U[0] loses less
                                          # than one binary digit, 2e-16 |x_1| against TOL_X = 1e-10


def cell_mus(nmu):
    return np.linspace(0.1, 1.0, nmu) if nmu > 1 else np.array([0.1])


def start_values(Aq, thetas, b, seed=U0_SEED):
    """U0 [S n, nmu]: per column standard normal numbers times max |A(theta_m)^-1 b|, the size of that column's stationary solution."""
    from scipy.sparse.linalg import spsolve
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    scale = np.array([np.abs(spsolve(ref3.combine(Aq, th).tocsc(), b)).max() for th in np.asarray(thetas)])
    return np.random.default_rng(seed).standard_normal((b.size, len(scale))) * scale[None, :]
