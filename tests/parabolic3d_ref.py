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


# ------------------------------------------------------------------------ the side kernels of the parabolic path, one by one
# Plain restatements of lrbms3_project_mass, lrbms3_mass_inverse_norm2, lrbms3_reduced_time_residual and the reduced stepper for
# tests/test_parabolic3d_dispatch_gpu.py.  Each takes one switch per property of the kernel it restates: with a switch thrown it
# is a deliberately wrong ("mutant") reference, which tests/test_parabolic3d_dispatch_host.py shows to be more than 1e-6 away
# from the right one at the cells of the GPU test -- so a kernel with that fault could not pass there.
SELF = 3                                   # the self slot of the 7-slot layout
WAVES = 8                                  # k3p_project_mass: waves per workgroup, one element per wave at a time
CHUNK = 256                                # k3p_mass_inv_norm2: vectors per trip of its l0 loop = threads per workgroup


def element_mass_blocks(o, s):
    """The 10 x 10 element blocks [n_T, 10, 10] of the oracle's mass matrix on subdomain s (it is element-block-diagonal)."""
    dofs = o.dofs_of(s)
    Ms = o.M.tocsr()[dofs][:, dofs].toarray()
    nT = o.n // 10
    blk = Ms.reshape(nT, 10, nT, 10)
    own = blk[np.arange(nT), :, np.arange(nT), :]
    assert np.count_nonzero(Ms) == np.count_nonzero(own), 'the mass matrix couples elements'
    return own


def project_mass(o, V, elem_type=None, swap_types=None, drop_tail=False, drop_cross=False):
    """lrbms3_project_mass: M_red [S, N, N] = sum_e V_e^T M_e V_e from the oracle's ``o.M``, accumulated in np.longdouble.
    Mutants: ``swap_types`` = (a, b) with ``elem_type`` [n_T]: the elements of type a take the block of the first element of type
    b; ``drop_tail``: the elements e >= 8 (n_T // 8) are left out (the partial last round of the 8 waves); ``drop_cross``: the
    16 x 16 tiles off the diagonal (rt != ct) stay zero."""
    V = np.asarray(V, dtype=np.float64)
    S, n, N = V.shape
    nT = n // 10
    out = np.zeros((S, N, N), dtype=np.longdouble)
    for s in range(S):
        TM = element_mass_blocks(o, s).astype(np.longdouble)
        if swap_types is not None:
            a, b = swap_types
            et = np.asarray(elem_type)
            TM[et == a] = TM[np.flatnonzero(et == b)[0]]
        Ve = V[s].reshape(nT, 10, N).astype(np.longdouble)
        last = WAVES * (nT // WAVES) if drop_tail else nT
        Z = np.einsum('eij,ejl->eil', TM[:last], Ve[:last])
        out[s] = np.einsum('eik,eil->kl', Ve[:last], Z)
    if drop_cross:
        tile = np.arange(N) // 16
        out[:, tile[:, None] != tile[None, :]] = 0.0
    return out


def chunk_of(L, l):
    """(Lc, G) of column l in a call of k3p_mass_inv_norm2 with L vectors: its trip of the l0 loop holds Lc <= 256 vectors,
    G = 256 // Lc threads share one vector, thread g takes the elements g, g + G, ..."""
    l0 = CHUNK * (l // CHUNK)
    Lc = min(L - l0, CHUNK)
    return Lc, CHUNK // Lc


def mass_inverse_norm2(o, Y, first_trip_only=False, drop_group_tail=False):
    """lrbms3_mass_inverse_norm2: out [S, L] = y_s^T M_s^-1 y_s for the columns of Y [S, n, L], by a sparse LU of ``o.M``.
    Mutants: ``first_trip_only``: the columns >= 256 stay zero (the l0 loop ends after one trip); ``drop_group_tail``: the
    elements e >= G (n_T // G) of a column are left out (the partial last round of the column's G threads)."""
    Y = np.asarray(Y, dtype=np.float64)
    S, n, L = Y.shape
    nT = n // 10
    flat = Y.reshape(S * n, L)
    X = spla.splu(o.M.tocsc()).solve(flat)
    per_elem = (flat * X).reshape(S, nT, 10, L).sum(axis=2)              # [S, n_T, L]: M is element-block-diagonal
    if drop_group_tail:
        for l in range(L):
            G = chunk_of(L, l)[1]
            per_elem[:, G * (nT // G):, l] = 0.0
    out = per_elem.sum(axis=1)
    if first_trip_only:
        out[:, CHUNK:] = 0.0
    return out


def reduced_operator_rows(B, nbr, theta, dU, drop_slot=None):
    """y [L, S, N]: y_s = sum_slot sum_q theta_q B_q[s, slot] dU[nbr[s, slot]] over the present slots (mutant: without ``drop_slot``)."""
    B, dU = np.asarray(B, dtype=np.float64), np.asarray(dU, dtype=np.float64)
    nbr = np.asarray(nbr).reshape(-1, 7)
    y = np.zeros_like(dU)
    for s in range(dU.shape[1]):
        for slot in range(7):
            t = int(nbr[s, slot])
            if t < 0 or slot == drop_slot:
                continue
            y[:, s] += dU[:, t] @ np.einsum('q,qij->ij', np.asarray(theta, dtype=np.float64), B[:, s, slot]).T
    return y


def reduced_time_residual(B, M_red, nbr, theta, dU, keep=None, drop_slot=None, diagonal_inverse=False):
    """lrbms3_reduced_time_residual: out [L, S] = y_s^T M_red[s]^-1 y_s on the kept indices (``keep`` [S, N] bool: False on the
    zero-padded unknowns of a ragged basis), dense NumPy per subdomain.  Mutants: ``drop_slot`` (one neighbour slot left out of
    y), ``diagonal_inverse`` (the inverse of the diagonal of M_red in place of M_red^-1)."""
    M_red = np.asarray(M_red, dtype=np.float64)
    y = reduced_operator_rows(B, nbr, theta, dU, drop_slot)
    L, S, N = y.shape
    keep = np.ones((S, N), dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    out = np.zeros((L, S))
    for s in range(S):
        ks = keep[s]
        Ms = M_red[s][np.ix_(ks, ks)]
        ys = y[:, s][:, ks]
        out[:, s] = np.einsum('li,li->l', ys, ys / np.diag(Ms) if diagonal_inverse else np.linalg.solve(Ms, ys.T).T)
    return out


def reduced_stepping(A, M_red, rhs, dt, nt, keep=None, mass_in_rhs=True):
    """lrbms3_reduced_implicit_euler from zero: (M + dt A) u_{k+1} = M u_k + dt rhs on the kept unknowns, dense; A [S N, S N] the
    reduced operator at the parameter, M_red [S, N, N] -> u [nt + 1, S N] (zero on the unknowns not kept).
    Mutant: ``mass_in_rhs`` False (every step starts from zero: the right-hand side without M u_k)."""
    M_red = np.asarray(M_red, dtype=np.float64)
    S, N = M_red.shape[:2]
    M = np.zeros((S * N, S * N))
    for s in range(S):
        M[s * N:(s + 1) * N, s * N:(s + 1) * N] = M_red[s]
    keep = np.ones(S * N, dtype=bool) if keep is None else np.asarray(keep, dtype=bool).reshape(S * N)
    Ak, Mk, bk = np.asarray(A)[np.ix_(keep, keep)], M[np.ix_(keep, keep)], np.asarray(rhs).reshape(S * N)[keep]
    u = np.zeros((nt + 1, S * N))
    for k in range(nt):
        u[k + 1, keep] = np.linalg.solve(Mk + dt * Ak, (Mk @ u[k, keep] if mass_in_rhs else 0.0) + dt * bk)
    return u
