"""CPU restatement of the 3D / P2 path with an affine source f = sum_j c_j f_j, stationary (c_j(mu)) and parabolic (c_j(mu, t)),
built on ``oracle.lrbms3d.Discretization3D`` / ``Reductor3D`` and tests/parabolic3d_ref.py the way tests/affine_source_ref.py and
tests/parabolic_source_ref.py are in 2D.  Test infrastructure only.

* Every quantity at mu (or at (t_k, mu)) is that of the oracle discretization with f frozen at sum_j c_j f_j: the three arrays
  of the oracle that read f (``b``, ``f2``, ``bdiv``; oracle/lrbms3d.py ``_assemble_rhs_and_products``,
  ``_assemble_estimator_operators``) are re-evaluated with the frozen function by the oracle's own formulas and quadrature.
* Parabolic stepping uses M U_k + dt b(t_{k+1}, mu); the elliptic part of U_k in the estimate uses f(t_k, mu).
* Components: f_0 = common3d._f and a second smooth function.  Stationary coefficients [1, max(0, 2 mu - 1)] (the second
  component vanishes for mu <= 0.5); parabolic coefficients [sin(4 pi t) > 0, -1] (the switching pattern of the artificial-channels
  demo)."""
import copy

import numpy as np
import scipy.sparse.linalg as spla

import common3d as c3
from oracle.lrbms3d import Reductor3D, _feval
from parabolic3d_ref import combine


def f_second(x):
    return np.sin(2.0 * x[..., 0] + x[..., 1]) + 0.5 * x[..., 2] * x[..., 1]


FUNCS = [c3._f, f_second]
STATIONARY = [1, lambda mu: max(0.0, 2 * mu - 1)]
PARABOLIC = [lambda mu, t: float(np.sin(4 * np.pi * t) > 0), -1.0]


def problem_dict(p, funcs=None, coeffs=None):
    """The product's 3D problem dict for the common3d problem ``p``, with the affine source (default: FUNCS / STATIONARY)."""
    f = {'functions': list(FUNCS if funcs is None else funcs), 'coefficients': list(STATIONARY if coeffs is None else coeffs)}
    return {'grid': p['grid'], 'lambda': {'functions': p['lambdas'], 'coefficients': p['thetas']}, 'lambda_bar': p['lambda_bar'],
            'lambda_hat': p['lambda_hat'], 'f': f, 'mu_bar': p['mu_bar'], 'mu_hat': p['mu_hat']}


def evaluate(coeffs, mu, t=None):
    """[K]: plain numbers are constants, lambdas of one argument read mu, of two (mu, t)."""
    import inspect
    out = []
    for c in coeffs:
        if not callable(c):
            out.append(float(c))
        elif len(inspect.signature(c).parameters) == 2:
            out.append(float(c(mu, t)))
        else:
            out.append(float(c(mu)))
    return np.array(out)


def projected_self_blocks(o, V):
    """(rhs [S, N], r_fd [S, QN]) of the oracle ``o`` on the bases V [S, n, N]: V_s^T b_s and the [self] block of the projected r_fd
    (columns q-major), the lines of ``Reductor3D.reduce`` for the images of a subdomain's own basis on itself."""
    m, S, N = o.mesh, o.S, V.shape[2]
    rhs = np.stack([V[ii].T @ o.b[o.dofs_of(ii)] for ii in range(S)])
    r_fd = []
    for ii in range(S):
        emb = np.zeros((o.ndof, N))
        emb[o.dofs_of(ii)] = V[ii]
        R = np.hstack([o.F_q[q] @ emb for q in range(o.Q)])
        el = m.elements_of(ii)
        r_fd.append(o.bdiv[el] @ np.einsum('ef,efc->ec', o.div[el], R[m.elem_face[el]]))
    return rhs, np.stack(r_fd)


class AffineSource3D:
    """The oracle discretization of a common3d problem whose source is sum_j c_j f_j."""

    def __init__(self, p, funcs=None, coeffs=None):
        self.p = p
        self.funcs = list(FUNCS if funcs is None else funcs)
        self.coeffs = list(STATIONARY if coeffs is None else coeffs)
        self.K = len(self.funcs)
        self.d = c3.oracle_of(dict(p, f=lambda x: sum(_feval(fn, x) for fn in self.funcs)))      # built on sum_j f_j, as the product

    def frozen(self, weights):
        """An oracle discretization with f := sum_j weights[j] f_j; everything that does not read f is shared with the base."""
        w = [float(v) for v in weights]
        funcs = self.funcs

        def f(x):
            out = w[0] * _feval(funcs[0], x)
            for wj, fn in zip(w[1:], funcs[1:]):
                out = out + wj * _feval(fn, x)
            return out
        o = copy.copy(self.d)
        o.f = f
        m = o.mesh
        x, wq, phi, _ = o._vol_points(o.deg + 4)                      # oracle/lrbms3d.py: b and f2
        fv = _feval(f, x)
        o.b = np.einsum('k,e,ek,ki->ei', wq, m.volume, fv, phi).ravel()
        o.f2 = np.array([np.einsum('k,e,ek->', wq, m.volume[m.elements_of(ii)], fv[m.elements_of(ii)] ** 2) for ii in range(o.S)])
        x, wq, _, _ = o._vol_points(3 * o.deg + 4)                    # oracle/lrbms3d.py: bdiv
        o.bdiv = np.einsum('k,e,ek->e', wq, m.volume, _feval(f, x))
        return o

    def component(self, j):
        return self.frozen(np.eye(self.K)[j])

    def gram(self):
        """F2 [S, K, K] = (f_j, f_l)_{L2(Omega_s)} by the oracle's rule for f2."""
        o, m = self.d, self.d.mesh
        x, wq, _, _ = o._vol_points(o.deg + 4)
        fv = np.stack([_feval(fn, x) for fn in self.funcs])
        return np.array([np.einsum('k,e,jek,lek->jl', wq, m.volume[m.elements_of(ii)], fv[:, m.elements_of(ii)], fv[:, m.elements_of(ii)])
                         for ii in range(o.S)])

    def coefficients(self, mu, t=None):
        return evaluate(self.coeffs, mu, t)

    def at(self, mu, t=None):
        return self.frozen(self.coefficients(mu, t))

    # ---- stationary
    def solve(self, mu):
        return self.at(mu).solve(mu).reshape(self.d.S, self.d.n)

    def estimate(self, U, mu):
        return self.at(mu).estimate(np.asarray(U).ravel(), mu, decompose=True)

    def reduced_rhs_only(self, rd0, V, mu):
        """``rd0`` (a reduced model of the base) with the right-hand side of f frozen at mu: enough for ``solve``."""
        o = self.at(mu)
        rd = copy.copy(rd0)
        rd.d, rd.rhs = o, [V[ii].T @ o.b[o.dofs_of(ii)] for ii in range(o.S)]
        return rd

    def reduced(self, V, mu, t=None):
        """The oracle reduced model on the bases V [S, n, N] with f frozen at (mu, t)."""
        o = self.at(mu, t)
        return Reductor3D(o, [V[ii] for ii in range(o.S)]).reduce()


class ParabolicSource3D:
    """Full order: (M + dt A(mu)) U_{k+1} = M U_k + dt b(t_{k+1}, mu); the elliptic terms of U_k with f(t_k, mu)."""

    def __init__(self, src, T, nt):
        self.src, self.o, self.T, self.nt = src, src.d, float(T), int(nt)
        self.dt = self.T / self.nt

    def table(self, mu):
        return np.stack([self.src.coefficients(mu, k * self.dt) for k in range(self.nt + 1)])

    def solve(self, mu):
        o = self.o
        lu = spla.splu((o.M + self.dt * o.system_matrix(mu)).tocsc())
        U = np.zeros((self.nt + 1, o.ndof))
        for k in range(self.nt):
            U[k + 1] = lu.solve(o.M @ U[k] + self.dt * self.src.at(mu, (k + 1) * self.dt).b)
        return U.reshape(self.nt + 1, o.S, o.n)

    def estimate(self, U, mu):
        o = self.o
        U = np.asarray(U).reshape(len(U), -1)
        terms = np.array([self.src.at(mu, k * self.dt).local_terms(U[k], mu) for k in range(len(U))])      # [L, 3, S]
        dU = U[1:] - U[:-1]
        tdnc2 = np.array([o.local_terms(v, mu)[0] for v in dU]).T
        A = o.system_matrix(mu)
        lu = spla.splu(o.M.tocsc())
        tr2 = np.array([lu.solve(A @ v) @ (A @ v) for v in dU])
        return combine(o, mu, self.dt, terms[:, 0].T, terms[:, 1].T, terms[:, 2].T, tr2, tdnc2)


class ParabolicSourceReduced3D:
    """The reduced model on local bases V [S, n, N]: Galerkin projections of A, M and of b(t, mu)."""

    def __init__(self, src, V, T, nt):
        self.src, self.o, self.T, self.nt = src, src.d, float(T), int(nt)
        self.dt = self.T / self.nt
        o = self.o
        self.V = np.asarray(V)
        self.N = self.V.shape[2]
        self.rd = Reductor3D(o, [self.V[ii] for ii in range(o.S)]).reduce()
        Mt = o.M.tocsr()
        self.M_blocks = [self.V[ii].T @ (Mt[o.dofs_of(ii)][:, o.dofs_of(ii)] @ self.V[ii]) for ii in range(o.S)]

    def matrices(self, mu):
        o, N = self.o, self.N
        th = o.theta(mu)
        A, M = np.zeros((o.S * N, o.S * N)), np.zeros((o.S * N, o.S * N))
        for ii in range(o.S):
            M[ii * N:(ii + 1) * N, ii * N:(ii + 1) * N] = self.M_blocks[ii]
            for jj, blocks in self.rd.op[ii].items():
                A[ii * N:(ii + 1) * N, jj * N:(jj + 1) * N] = sum(t * B for t, B in zip(th, blocks))
        return A, M

    def rhs(self, mu, t):
        b = self.src.at(mu, t).b.reshape(self.o.S, self.o.n)
        return np.concatenate([self.V[ii].T @ b[ii] for ii in range(self.o.S)])

    def solve(self, mu):
        A, M = self.matrices(mu)
        u = np.zeros((self.nt + 1, self.o.S * self.N))
        for k in range(self.nt):
            u[k + 1] = np.linalg.solve(M + self.dt * A, M @ u[k] + self.dt * self.rhs(mu, (k + 1) * self.dt))
        return u

    def estimate(self, u, mu):
        o, N = self.o, self.N
        A, M = self.matrices(mu)
        split = lambda v: [v[ii * N:(ii + 1) * N] for ii in range(o.S)]                                # noqa: E731
        terms, cache = [], {}
        for k, uk in enumerate(u):
            w = tuple(self.src.coefficients(mu, k * self.dt))
            if w not in cache:                           # the reduced model with f frozen at t_k: r_fd and d.f2 read f
                ok = self.src.frozen(w)
                rd = copy.copy(self.rd)
                rd.d, rd.r_fd = ok, Reductor3D(ok, [self.V[ii] for ii in range(o.S)]).reduce().r_fd
                cache[w] = rd
            terms.append(cache[w].local_terms(split(uk), mu))
        terms = np.array(terms)
        du = u[1:] - u[:-1]
        tdnc2 = np.array([self.rd.local_terms(split(v), mu)[0] for v in du]).T
        tr2 = np.array([np.linalg.solve(M, A @ v) @ (A @ v) for v in du])
        return combine(o, mu, self.dt, terms[:, 0].T, terms[:, 1].T, terms[:, 2].T, tr2, tdnc2)
