"""NumPy / SciPy reference of the batched reduced implicit Euler of the 3D / P2 path (lrbms3_reduced_implicit_euler_batch(_src)).

Per parameter: the sparse step operator ``block_diag(M_red) + dt * pcg_ref.reduced_operator(pcg_ref.combine_reduced(B, theta))``
on the 7-slot layout (both helpers are slot-count agnostic; the self slot is 3) and one direct solve per step,
(M + dt A) u_{k+1} = M u_k + dt b_k.  ``StepPrecond3D`` restates the two-level preconditioner of the call: the step operator at
the mean theta, inverse diagonal blocks with the zero-diagonal -> 1 rule, the coarse matrix from the (0, 0) entries, Cholesky or
none.  tests/test_parabolic_batch3d_host.py pins the stepping to ``ParabolicReduced3D.solve`` of tests/parabolic3d_ref.py."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
from scipy.sparse.linalg import splu

import pcg_ref

SELF = 3          # the self slot of the 7-slot layout


def mass_operator(M_red):
    """Block-diagonal sparse [S N, S N] matrix of M_red [S, N, N]."""
    return sp.block_diag([np.asarray(Ms) for Ms in M_red], format='csr')


def step_blocks(B, M_red, theta, dt):
    """The step operator in the fixed-slot layout [S, 7, N, N]: dt sum_q theta_q B_q with M_red on the self slot."""
    Amu = dt * pcg_ref.combine_reduced(B, theta)
    Amu[:, SELF] += np.asarray(M_red)
    return Amu


def step_operator(B, M_red, nbr, theta, dt):
    """Sparse [S N, S N] step operator M + dt A(theta)."""
    return (mass_operator(M_red) + dt * pcg_ref.reduced_operator(pcg_ref.combine_reduced(B, theta), nbr)).tocsr()


def step_rhs(S, N, step, rhs=None, rhs_K=None, phi=None):
    """b of step ``step`` (row step + 1 of the coefficient table phi [nt + 1, K]) as a flat [S N] vector."""
    if rhs_K is None:
        return np.asarray(rhs, dtype=np.float64).reshape(S * N)
    return np.einsum('j,jn->n', np.asarray(phi)[step + 1], np.asarray(rhs_K).reshape(-1, S * N))


def dense_euler(B, M_red, nbr, theta, dt, nt, rhs=None, rhs_K=None, phi=None, U0=None, keep=None):
    """One trajectory [nt + 1, S, N] at ``theta``.  ``keep`` [S, N] (0 / 1): zero-padded basis columns get 1 on the diagonal of
    the step operator (they have a zero row and column in B and M_red), so that they stay 0 and the solve is regular."""
    S, N = np.asarray(M_red).shape[:2]
    M = mass_operator(M_red)
    lhs = step_operator(B, M_red, nbr, theta, dt)
    if keep is not None:
        lhs = lhs + sp.diags(1.0 - np.asarray(keep, dtype=np.float64).ravel())
    lu = splu(lhs.tocsc())
    U = np.zeros((nt + 1, S * N))
    if U0 is not None:
        U[0] = np.asarray(U0, dtype=np.float64).reshape(S * N)
    for k in range(nt):
        U[k + 1] = lu.solve(M @ U[k] + dt * step_rhs(S, N, k, rhs, rhs_K, phi))
    return U.reshape(nt + 1, S, N)


def dense_euler_batch(B, M_red, nbr, thetas, dt, nt, rhs=None, rhs_K=None, phis=None, U0=None, keep=None):
    """[nt + 1, S, N, nmu]: column m at thetas[m] (and phis[m] [nt + 1, K]); U0 [S, N] or [S, N, nmu]."""
    cols = []
    for m, th in enumerate(thetas):
        u0 = None if U0 is None else (U0 if np.ndim(U0) == 2 else np.asarray(U0)[:, :, m])
        cols.append(dense_euler(B, M_red, nbr, th, dt, nt, rhs=rhs, rhs_K=rhs_K, phi=None if phis is None else phis[m], U0=u0,
                                keep=keep))
    return np.stack(cols, axis=-1)


def column_errors(U, U_ref):
    """max |U - U_ref| / max |U_ref| per (step >= 1, column) of two [nt + 1, S, N, nmu] arrays -> [nt, nmu]."""
    U, U_ref = np.asarray(U), np.asarray(U_ref)
    assert U.shape == U_ref.shape, (U.shape, U_ref.shape)
    num = np.abs(U[1:] - U_ref[1:]).max(axis=(1, 2))
    den = np.abs(U_ref[1:]).max(axis=(1, 2))
    return num / np.where(den > 0.0, den, 1.0)


def true_residuals(U, B, M_red, nbr, thetas, dt, rhs=None, rhs_K=None, phis=None):
    """|(M + dt A_m) u_{k+1} - f_m| / |f_m|, f_m = M u_k + dt b_m, for every step and column of U [nt + 1, S, N, nmu] -> [nt, nmu]."""
    U = np.asarray(U)
    nt, S, N, nmu = U.shape[0] - 1, U.shape[1], U.shape[2], U.shape[3]
    M = mass_operator(M_red)
    out = np.zeros((nt, nmu))
    for m, th in enumerate(thetas):
        lhs = step_operator(B, M_red, nbr, th, dt)
        for k in range(nt):
            f = M @ U[k, :, :, m].ravel() + dt * step_rhs(S, N, k, rhs, rhs_K, None if phis is None else phis[m])
            out[k, m] = np.linalg.norm(lhs @ U[k + 1, :, :, m].ravel() - f) / np.linalg.norm(f)
    return out


def coarse_matrix(Amu, nbr):
    """A0 [S, S] dense: A0[s, t] = entry (0, 0) of block [s][slot] with t = nbr[s, slot] (k3r_coarse_fill; nbr[s, 3] == s)."""
    S = Amu.shape[0]
    A0 = np.zeros((S, S))
    for s in range(S):
        for slot in range(7):
            t = s if slot == SELF else int(nbr[s][slot])
            if t >= 0:
                A0[s, t] = Amu[s, slot, 0, 0]
    return A0


class StepPrecond3D:
    """M^-1 r = D^-1 r + R0^T A0^-1 R0 r with (R0 r)_s = r[s][0] for the step operator at ``theta`` (the call mean):
    D^-1 = ``pcg_ref.reduced_block_jacobi`` of the self-slot blocks; the coarse level exists if ``coarse`` and A0 is positive
    definite (no limits on S: the 3D call builds it for every S)."""

    def __init__(self, B, M_red, nbr, theta, dt, coarse=True):
        Amu = step_blocks(B, M_red, theta, dt)
        self.S, self.N = Amu.shape[0], Amu.shape[2]
        self.Dinv = pcg_ref.reduced_block_jacobi(Amu[:, SELF])
        self.A0 = coarse_matrix(Amu, nbr)
        self.cho = None
        if coarse:
            try:
                self.cho = sla.cho_factor(self.A0, lower=True)
            except np.linalg.LinAlgError:
                self.cho = None

    @property
    def has_coarse(self):
        return self.cho is not None

    def matrix(self):
        """Dense M^-1 [S N, S N]."""
        return self.apply(np.eye(self.S * self.N))

    def apply(self, r):
        one = r.ndim == 1
        R = r[:, None] if one else r
        S, N, m = self.S, self.N, R.shape[1]
        z = np.einsum('sij,sjm->sim', self.Dinv, R.reshape(S, N, m))
        if self.cho is not None:
            z[:, 0, :] += sla.cho_solve(self.cho, R.reshape(S, N, m)[:, 0, :])
        z = z.reshape(S * N, m)
        return z[:, 0] if one else z


def pcg_dense(A, Minv, b, k, dtype=np.float64):
    """The recurrences of ``pcg_ref.pcg_iterate`` for ONE right-hand side with dense A and M^-1 in ``dtype`` (float64 or
    longdouble: the tolerance of the iterate tests is their difference) -> (x_k, |r_k| / |b|)."""
    A, Minv, b = np.asarray(A, dtype=dtype), np.asarray(Minv, dtype=dtype), np.asarray(b, dtype=dtype)
    x, r = np.zeros_like(b), b.copy()
    z = Minv @ r
    p, rz = z.copy(), r @ z
    for _ in range(k):
        Ap = A @ p
        pAp = p @ Ap
        alpha = rz / pAp if pAp != 0 else dtype(0)
        x = x + alpha * p
        r = r - alpha * Ap
        z = Minv @ r
        rz_new = r @ z
        beta = rz_new / rz if rz != 0 else dtype(0)
        p = z + beta * p
        rz = rz_new
    n0 = np.sqrt(b @ b)
    return x, (np.sqrt(r @ r) / n0 if n0 > 0 else dtype(0))
