"""NumPy / SciPy reference of the parabolic exports with a diffusion-coefficient row per step (lrbms_fom_implicit_euler_batch_tv,
lrbms_reduced_implicit_euler_batch_tv, lrbms_reduced_parabolic_estimate_batch_tv), on top of
tests/parabolic_batch_ref.py, tests/fom_euler_batch_ref.py and tests/parabolic_estimate_batch_ref.py.

theta_t [nt + 1, Q] is the table of one column (row k: the coefficients at the time of step k).  The step k -> k + 1 solves with
row k + 1 -- the operator pyMOR's implicit Euler assembles after ``t += dt`` --, the elliptic indicators of U_k use row k and the
time residual of U_{k+1} - U_k row k + 1.  ``rows`` lets a test step with OTHER rows (the wrong variants of
tests/test_parabolic_tv_host.py).  tests/test_parabolic_tv_host.py pins the constant-table case to the oracle."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu

import pcg_ref
from fom_euler_batch_ref import combine as combine_fom
from parabolic_batch_ref import mass_operator, step_blocks, step_rhs
from parabolic_estimate_batch_ref import time_residual_panel


def step_rows(theta_t):
    """The nt operator rows of the steps 0 .. nt - 1: rows 1 .. nt of the table (the right limit)."""
    return np.asarray(theta_t, dtype=np.float64)[1:]


def step_mean(thetas_t, first=1, last=None):
    """Where the drivers build the preconditioner (reduced) and the coarse level (full order) of a call: the mean of
    thetas_t [nmu, nt + 1, Q] over the columns and the rows 1 .. nt -> [Q].  ``first`` / ``last`` (inclusive) select OTHER rows:
    the wrong variants (row 1 only: last = 1; the rows 0 .. nt: first = 0) that the iterate tests must tell from the right one."""
    thetas_t = np.asarray(thetas_t, dtype=np.float64)
    last = thetas_t.shape[1] - 1 if last is None else last
    return thetas_t[:, first:last + 1].mean(axis=(0, 1))


def row_step_blocks(B, M_red, theta_row, dt):
    """The step operator of one table row in the fixed-slot layout [S, 5, N, N]: M_red on the self slot + dt sum_q theta_row[q] B_q
    (``parabolic_batch_ref.step_blocks`` at that row; the step k -> k + 1 of column m takes thetas_t[m, k + 1])."""
    return step_blocks(B, M_red, np.asarray(theta_row, dtype=np.float64), dt)


def dense_euler_tv(B, M_red, nbr, theta_t, dt, nt, rhs=None, rhs_K=None, phi=None, U0=None, keep=None, rows=None):
    """One reduced trajectory [nt + 1, S, N]: ``parabolic_batch_ref.dense_euler`` with the step operator rebuilt per step."""
    S, N = np.asarray(M_red).shape[:2]
    M = mass_operator(M_red)
    rows = step_rows(theta_t) if rows is None else np.asarray(rows, dtype=np.float64)
    assert rows.shape[0] == nt
    pad = sp.diags(1.0 - np.asarray(keep, dtype=np.float64).ravel()) if keep is not None else None
    U = np.zeros((nt + 1, S * N))
    if U0 is not None:
        U[0] = np.asarray(U0, dtype=np.float64).reshape(S * N)
    for k in range(nt):
        lhs = M + dt * pcg_ref.reduced_operator(pcg_ref.combine_reduced(B, rows[k]), nbr)
        if pad is not None:
            lhs = lhs + pad
        U[k + 1] = splu(lhs.tocsc()).solve(M @ U[k] + dt * step_rhs(S, N, k, rhs, rhs_K, phi))
    return U.reshape(nt + 1, S, N)


def dense_euler_batch_tv(B, M_red, nbr, thetas_t, dt, nt, rhs=None, rhs_K=None, phis=None, U0=None, keep=None):
    """[nt + 1, S, N, nmu]: column m with the table thetas_t[m] [nt + 1, Q] (and phis[m] [nt + 1, K])."""
    cols = []
    for m, th in enumerate(thetas_t):
        u0 = None if U0 is None else (U0 if np.ndim(U0) == 2 else np.asarray(U0)[:, :, m])
        cols.append(dense_euler_tv(B, M_red, nbr, th, dt, nt, rhs=rhs, rhs_K=rhs_K, phi=None if phis is None else phis[m], U0=u0,
                                   keep=keep))
    return np.stack(cols, axis=-1)


def fom_euler_tv(Aq, M, theta_t, dt, nt, phi, b_K, U0=None, rows=None):
    """One full-order trajectory [nt + 1, ndof]: (M + dt sum_q rows[k][q] Aq[q]) u_{k+1} = M u_k + dt sum_j phi[k + 1][j] b_K[j]
    with the sparse components ``Aq`` (``fom_euler_batch_ref.component_operators``) and mass ``M``."""
    rows = step_rows(theta_t) if rows is None else np.asarray(rows, dtype=np.float64)
    assert rows.shape[0] == nt
    M = sp.csr_matrix(M)
    b_K = np.asarray(b_K, dtype=np.float64).reshape(len(b_K), -1)
    U = np.zeros((nt + 1, M.shape[0]))
    if U0 is not None:
        U[0] = np.asarray(U0, dtype=np.float64).ravel()
    for k in range(nt):
        lhs = (M + dt * combine_fom(Aq, rows[k])).tocsc()
        U[k + 1] = splu(lhs).solve(M @ U[k] + dt * (np.asarray(phi)[k + 1] @ b_K))
    return U


def fom_euler_batch_tv(Aq, M, thetas_t, dt, nt, phis, b_K, U0=None):
    """[nt + 1, ndof, nmu]; U0 [ndof] or [ndof, nmu]."""
    cols = []
    for m, th in enumerate(thetas_t):
        u0 = None if U0 is None else (U0 if np.ndim(U0) == 1 else np.asarray(U0)[:, m])
        cols.append(fom_euler_tv(Aq, M, th, dt, nt, phis[m], b_K, U0=u0))
    return np.stack(cols, axis=-1)


def time_residual_panel_tv(U, B, M_red, nbr, thetas_t):
    """U [nt + 1, S, N, nmu], thetas_t [nmu, nt + 1, Q] -> y^T M_red[s]^-1 y [nt, S, nmu] with
    y = sum_q thetas_t[m][k + 1][q] B_q (U[k+1] - U[k]): the operator that produced U[k+1]."""
    U, thetas_t = np.asarray(U, dtype=np.float64), np.asarray(thetas_t, dtype=np.float64)
    return np.concatenate([time_residual_panel(U[k:k + 2], B, M_red, nbr, thetas_t[:, k + 1]) for k in range(U.shape[0] - 1)])


def combine_tv(eta_raw, tr2, nc_diff, coef, dt, sqrt_local=False):
    """``parabolic_estimate_batch_ref.combine`` with the two factors of the elliptic eta per (column, step): coef [nmu, nt + 1, 2] =
    sqrt(gamma_bar / alpha_bar), 1 / sqrt(alpha_hat alpha_bar) at row k.  eta_raw [3, nt + 1, S, nmu] (row k of the table),
    tr2 / nc_diff [nt, S, nmu]."""
    nc, r, df = (np.asarray(x, dtype=np.float64) for x in eta_raw)
    coef = np.asarray(coef, dtype=np.float64)
    if sqrt_local:
        nc, r, df = (np.sqrt(np.abs(x)) for x in (nc, r, df))
    s = 2 * np.sqrt(dt / 3)
    n0 = np.sqrt((nc ** 2).sum(axis=1))                                     # [nt + 1, nmu]
    n1 = np.sqrt(((r + df) ** 2).sum(axis=1))
    eta = (coef[:, :, 0].T * n0 + coef[:, :, 1].T * n1) * s
    time_residual = np.sqrt(np.asarray(tr2).sum(axis=1) * (dt / 3))
    time_deriv_nc = np.sqrt(np.maximum(np.asarray(nc_diff) * (1 / dt), 0.0))
    est = (np.sqrt((eta ** 2).sum(axis=0)) + np.sqrt((time_residual ** 2).sum(axis=0))
           + np.sqrt((time_deriv_nc ** 2).sum(axis=(0, 1))))
    return {'eta_loc': np.stack([nc * s, r * s, df * s]), 'time_deriv_nc': time_deriv_nc, 'time_residual': time_residual,
            'eta': eta, 'est': est}


def switch_table(nmu, nt, Q, T, t_star=None, seed=0):
    """thetas_t [nmu, nt + 1, Q] inside (0.1, 1], the parameter range of the test problems: per column a level in [0.5, 1] times a
    smooth factor of the time (0.85 + 0.15 sin(2 pi t / T + column phase)), and a two-level switch on the last component (x 0.3
    after ``t_star``; default: between the first two step times, never on a step time).  Component 0 stays 1 for Q = 2 (the
    problems' theta = (1, mu)).  Row k sits at t_k accumulated like the implicit Euler (t += dt)."""
    dt = T / nt
    t_star = 0.4 * dt if t_star is None else t_star
    rng = np.random.default_rng(seed)
    levels = rng.uniform(0.5, 1.0, (nmu, Q))
    out = np.empty((nmu, nt + 1, Q))
    t = 0.0
    for k in range(nt + 1):
        if k > 0:
            t += dt
        for m in range(nmu):
            out[m, k] = levels[m] * (0.85 + 0.15 * np.sin(2 * np.pi * t / T + 0.7 * m))
            out[m, k, Q - 1] *= 1.0 if t <= t_star else 0.3
    if Q == 2:
        out[:, :, 0] = 1.0
    assert out.min() > 0.1 and out.max() <= 1.0
    return np.ascontiguousarray(out)
