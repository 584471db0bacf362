"""CPU restatement of the parabolic path with a time-dependent affine source f(t, mu) = sum_j phi_j(t, mu) f_j, built on
``oracle.lrbms`` / ``oracle.parabolic`` the way tests/parabolic3d_ref.py is built on the 3D oracle.  Test infrastructure only.

* phi [nt + 1][K]: row 0 at t = 0, row k at the time of step k with t accumulated as pyMOR's implicit Euler does (t += dt).
* Implicit Euler: (M + dt A(mu)) U_{k+1} = M U_k + dt sum_j phi[k+1][j] b_j, one sparse LU, b_j from oracle discretizations
  of the single components.
* The elliptic part of the estimate of U_k is the STATIONARY oracle estimator with f frozen at f(t_k): an oracle
  discretization whose f is sum_j phi[k][j] f_j (its load vector and ||f||^2 re-assembled).  The time residual and the
  time-derivative nonconformity do not involve f and are those of oracle.parabolic.OracleParabolic."""
import copy

import numpy as np
import scipy.sparse.linalg as spla

from common import oracle_from_problem
from oracle.parabolic import OracleParabolic


def phi_table(coefficients, mu, T, nt):
    """[nt + 1, K]: the coefficients at t_0 = 0 and at the times of the nt steps (t += T / nt)."""
    from pylrbms_amd.parameters import Parameter
    dt = T / nt
    out = np.zeros((nt + 1, len(coefficients)))
    t = 0.0
    for k in range(nt + 1):
        if k:
            t = t + dt
        m = Parameter(dict(mu, _t=np.array(t)))
        out[k] = [c.evaluate(m) if hasattr(c, 'evaluate') else float(c) for c in coefficients]
    return out


class ParabolicSource(OracleParabolic):
    """``OracleParabolic`` for a problem dict whose ``f`` is ``{'functions': [...], 'coefficients': [...]}``."""

    def __init__(self, p, T, nt):
        from pylrbms_amd.functions import SumFunction
        self.p = p
        self.funcs, self.coeffs = list(p['f']['functions']), list(p['f']['coefficients'])
        self.K = len(self.funcs)
        # the same quadrature orders as the product, which builds its elliptic discretization on sum_j f_j
        base = oracle_from_problem(dict(p, f=SumFunction(self.funcs, [1.0] * self.K)))
        super().__init__(base, T, nt)
        self.b_K = np.stack([self.frozen(np.eye(self.K)[j]).b for j in range(self.K)])      # [K, ndof]

    def frozen(self, weights):
        """An oracle discretization with f := sum_j weights[j] f_j (everything else shared with the base)."""
        from pylrbms_amd.functions import SumFunction
        o = copy.copy(self.d)
        o._smp_cache = {}
        o.f = SumFunction(self.funcs, [float(w) for w in weights], name='f_frozen')
        o._assemble_rhs()
        return o

    def parse(self, mu):
        from pylrbms_amd.parameters import parse_parameter
        return parse_parameter(mu, self.p['parameter_type'])

    def phi(self, mu):
        return phi_table(self.coeffs, self.parse(mu), self.T, self.nt)

    def gram(self):
        """F2 [S, K, K] = (f_j, f_l)_{L2(Omega_s)} with the oracle's f2 rule."""
        o = self.d
        w = o._tri(o.quad.f2)['w']
        smp = [o._vol(fn, o.quad.f2) for fn in self.funcs]
        F2 = np.zeros((o.S, self.K, self.K))
        for j in range(self.K):
            for l in range(self.K):
                per_e = (smp[j] * smp[l] * w[None, :]).sum(axis=1) * o.mesh.area
                F2[:, j, l] = per_e.reshape(o.S, o.nT).sum(axis=1)
        return F2

    def solve(self, mu):
        """[nt + 1, S, n]; zero initial data."""
        d = self.d
        phi = self.phi(mu)
        M = d.l2_product.tocsc()
        lu = spla.splu((M + self.dt * d.assemble_global(self.parse(mu))).tocsc())
        U = np.zeros((self.nt + 1, d.ndof))
        for k in range(self.nt):
            U[k + 1] = lu.solve(M @ U[k] + self.dt * (phi[k + 1] @ self.b_K))
        return U.reshape(self.nt + 1, d.S, d.n)

    def _elliptic_local(self, U, mu, elliptic_reconstruction):
        assert not elliptic_reconstruction
        phi = self.phi(mu)
        assert U.shape[0] == self.nt + 1
        L = U.shape[0]
        nc, r, df = np.zeros((self.d.S, L)), np.zeros((self.d.S, L)), np.zeros((self.d.S, L))
        for k in range(L):
            _, (nc[:, k], r[:, k], df[:, k]), _ = self.frozen(phi[k]).estimate(U[k], self.parse(mu), decompose=True)
        return nc, r, df

    def estimate(self, U, mu, elliptic_reconstruction=False):
        return super().estimate(np.asarray(U).reshape(self.nt + 1, self.d.S, self.d.n), self.parse(mu), elliptic_reconstruction)


def reduced_matrices(B_sys, M_red, nbr, theta):
    """Dense (sum_q theta_q B_q) and block-diagonal M_red of the product's block-sparse reduced system (numpy arrays)."""
    Q, S, _, N, _ = B_sys.shape
    A = np.zeros((S * N, S * N))
    M = np.zeros((S * N, S * N))
    for s in range(S):
        M[s * N:(s + 1) * N, s * N:(s + 1) * N] = M_red[s]
        for slot in range(5):
            t = int(nbr[s, slot])
            if t >= 0:
                A[s * N:(s + 1) * N, t * N:(t + 1) * N] += sum(theta[q] * B_sys[q, s, slot] for q in range(Q))
    return A, M


def reduced_stepping(A, M, rhs_K, phi, dt, nt):
    """Reduced implicit Euler on dense arrays: rhs_K [K, S * N]; -> u [nt + 1, S * N]."""
    u = np.zeros((nt + 1, A.shape[0]))
    for k in range(nt):
        u[k + 1] = np.linalg.solve(M + dt * A, M @ u[k] + dt * (phi[k + 1] @ rhs_K))
    return u
