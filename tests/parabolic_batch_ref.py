"""NumPy / SciPy reference of the batched reduced implicit Euler (lrbms_reduced_implicit_euler_batch(_src)).

Per parameter: the sparse step operator ``block_diag(M_red) + dt * pcg_ref.reduced_operator(pcg_ref.combine_reduced(B, theta))``
and one direct solve per step,  (M + dt A) u_{k+1} = M u_k + dt b_k.  tests/test_parabolic_batch_host.py pins it to
``oracle.parabolic.OracleParabolicReduced.solve`` on the CPU; the GPU tests compare the exports against it."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

import pcg_ref


def mass_operator(M_red):
    """Block-diagonal sparse [S N, S N] matrix of M_red [S, N, N]."""
    return sp.block_diag([np.asarray(Ms) for Ms in M_red], format='csr')


def step_blocks(B, M_red, theta, dt):
    """The step operator in the fixed-slot layout [S, 5, N, N]: dt sum_q theta_q B_q with M_red on the self slot (slot 2)."""
    Amu = dt * pcg_ref.combine_reduced(B, theta)
    Amu[:, 2] += np.asarray(M_red)
    return Amu


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
    lhs = M + dt * pcg_ref.reduced_operator(pcg_ref.combine_reduced(B, theta), nbr)
    if keep is not None:
        lhs = lhs + sp.diags(1.0 - np.asarray(keep, dtype=np.float64).ravel())
    lhs = lhs.tocsc()
    U = np.zeros((nt + 1, S * N))
    if U0 is not None:
        U[0] = np.asarray(U0, dtype=np.float64).reshape(S * N)
    for k in range(nt):
        U[k + 1] = spsolve(lhs, M @ U[k] + dt * step_rhs(S, N, k, rhs, rhs_K, phi))
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
    """|(M + dt A_m) u_{k+1} - M u_k - dt b| / |M u_k + dt b| for every step and column of U [nt + 1, S, N, nmu] -> [nt, nmu]."""
    U = np.asarray(U)
    nt, S, N, nmu = U.shape[0] - 1, U.shape[1], U.shape[2], U.shape[3]
    M = mass_operator(M_red)
    out = np.zeros((nt, nmu))
    for m, th in enumerate(thetas):
        lhs = M + dt * pcg_ref.reduced_operator(pcg_ref.combine_reduced(B, th), nbr)
        for k in range(nt):
            b = M @ U[k, :, :, m].ravel() + dt * step_rhs(S, N, k, rhs, rhs_K, None if phis is None else phis[m])
            out[k, m] = np.linalg.norm(lhs @ U[k + 1, :, :, m].ravel() - b) / np.linalg.norm(b)
    return out
