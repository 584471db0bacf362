"""NumPy restatement of the pieces lrbms_reduced_parabolic_estimate_batch adds to the existing estimate exports:

* ``time_residual_panel``: y = A(theta_m) (U[k+1] - U[k]) and y^T M_red^-1 y per subdomain, step and column, on the sparse
  operators of tests/parabolic_batch_ref.py (``step_blocks`` with a zero mass gives the fixed-slot blocks of A(theta));
* ``nc_of_differences``: the nonconformity form of U[k+1] - U[k], the difference taken on the coefficients FIRST;
* ``combine``: the host half of ``ParabolicEstimator.estimate`` (pylrbms_amd/estimators.py:124-157 with
  ``_estimate_elliptic``:65-72), incl. ``sqrt_local``.

tests/test_parabolic_estimate_batch_host.py pins them to ``oracle.parabolic.OracleParabolicReduced.estimate`` on the CPU; the GPU
tests compare the export against them."""
import numpy as np

import pcg_ref
from parabolic_batch_ref import mass_operator, step_blocks


def time_residual_panel(U, B, M_red, nbr, thetas):
    """U [nt + 1, S, N, nmu] -> y^T M_red[s]^-1 y [nt, S, nmu] with y = (sum_q theta_mq B_q (U[k+1] - U[k]))_s.  A zero diagonal
    entry of M_red (zero-padded basis column: zero row and column) counts as 1, the rule of the block inverse."""
    U = np.asarray(U, dtype=np.float64)
    nt, S, N, nmu = U.shape[0] - 1, U.shape[1], U.shape[2], U.shape[3]
    M = np.array(M_red, dtype=np.float64)
    for s in range(S):
        for j in range(N):
            if M[s, j, j] == 0.0:
                M[s, j, j] = 1.0
    Minv = np.stack([np.linalg.inv(Ms) for Ms in M])
    assert mass_operator(M).shape == (S * N, S * N)
    out = np.zeros((nt, S, nmu))
    for m, th in enumerate(thetas):
        A = pcg_ref.reduced_operator(step_blocks(B, np.zeros_like(M), th, 1.0), nbr)
        for k in range(nt):
            dU = (U[k + 1, :, :, m] - U[k, :, :, m]).reshape(S * N)
            y = (A @ dU).reshape(S, N)
            out[k, :, m] = np.einsum('si,sij,sj->s', y, Minv, y)
    return out


def nc_form(G_nc, nbr, u):
    """u [S, N, L] -> uo^T G_nc[s] uo [S, L] with uo the coefficients of the five fixed slots (absent neighbour: zeros);
    G_nc [S, 5 N, 5 N] (the dense layout)."""
    S, N, L = u.shape
    out = np.zeros((S, L))
    for s in range(S):
        uo = np.zeros((5 * N, L))
        for slot in range(5):
            s2 = int(nbr[s, slot])
            if s2 >= 0:
                uo[slot * N:(slot + 1) * N] = u[s2]
        out[s] = np.einsum('il,ij,jl->l', uo, G_nc[s], uo)
    return out


def nc_of_differences(G_nc, nbr, U):
    """U [nt + 1, S, N, nmu] -> nc_s(U[k+1] - U[k]) [nt, S, nmu]: difference first, then the form (never
    nc(U[k+1]) - 2 cross + nc(U[k]), which cancels)."""
    U = np.asarray(U, dtype=np.float64)
    return np.stack([nc_form(G_nc, nbr, U[k + 1] - U[k]) for k in range(U.shape[0] - 1)])


def combine(eta_raw, tr2, nc_diff, alpha_bar, gamma_bar, alpha_hat, dt, sqrt_local=False):
    """eta_raw [3, nt + 1, S, nmu] (nc, r, df as ``_local_estimates`` returns them), tr2 [nt, S, nmu], nc_diff [nt, S, nmu],
    alpha_bar / gamma_bar / alpha_hat [nmu] -> dict with eta_loc [3, nt + 1, S, nmu], time_deriv_nc [nt, S, nmu],
    time_residual [nt, nmu], eta [nt + 1, nmu], est [nmu]."""
    nc, r, df = (np.asarray(x, dtype=np.float64) for x in eta_raw)
    a_bar, g_bar, a_hat = (np.asarray(x, dtype=np.float64) for x in (alpha_bar, gamma_bar, alpha_hat))
    if sqrt_local:                                                          # estimators.py:65-66
        nc, r, df = (np.sqrt(np.abs(x)) for x in (nc, r, df))
    n0 = np.sqrt((nc ** 2).sum(axis=1))                                     # :70 (global_norms), per step and column
    n1 = np.sqrt(((r + df) ** 2).sum(axis=1))
    eta = (np.sqrt(g_bar) * n0 + (1.0 / np.sqrt(a_hat)) * n1) * (1.0 / np.sqrt(a_bar))      # :71-72
    time_residual = np.sqrt(np.asarray(tr2).sum(axis=1) * (dt / 3))         # :131-133
    s = 2 * np.sqrt(dt / 3)                                                 # :136-139
    eta = eta * s
    time_deriv_nc = np.sqrt(np.maximum(np.asarray(nc_diff) * (1 / dt), 0.0))        # :142-144
    est = (np.sqrt((eta ** 2).sum(axis=0)) + np.sqrt((time_residual ** 2).sum(axis=0))
           + np.sqrt((time_deriv_nc ** 2).sum(axis=(0, 1))))                # :146, :156
    return {'eta_loc': np.stack([nc * s, r * s, df * s]), 'time_deriv_nc': time_deriv_nc, 'time_residual': time_residual,
            'eta': eta, 'est': est}
