"""NumPy restatement of the three ``lrbms3_*_tv`` exports (diffusion coefficients of the time, theta_t
[nmu, nt + 1, Q]) on top of the references of their twins: tests/parabolic_batch3d_ref.py (reduced stepping, ``StepPrecond3D``),
tests/fom_euler_batch3d_ref.py (full-order stepping, ``BatchFomEuler3DRef``), tests/parabolic_estimate_batch3d_ref.py (the rows of the
estimate) and tests/pcg_ref.py.  Test infrastructure only.

The conventions restated: the step k -> k + 1 solves with row k + 1; ONE preconditioner per call at the mean over the columns of the
time means over the rows 1 .. nt; in the estimate the elliptic rows of U[k], its source terms and coef use row k, the time residual
of U[k + 1] - U[k] row k + 1.

``fault`` (one of FAULTS, or None) throws one fault into a restatement; tests/test_parabolic_tv3d_host.py shows each to be more
than 1e-6 away from the right one on the inputs of the GPU cells, so an export with that fault could not pass there."""
import numpy as np
from scipy.sparse.linalg import splu

import fom_batch3d_ref as ref3
import parabolic_batch3d_ref as rb
import parabolic_estimate_batch3d_ref as pe
import pcg_ref
from fom_euler_batch3d_ref import BatchFomEuler3DRef

DT = 0.05
STEP_FAULTS = ('step_row_k', 'time_mean', 'column0')                  # stepping with row k; the time mean in every step; column 0's table
ESTIMATE_FAULTS = ('column0', 'elliptic_row_k1', 'residual_row_k', 'coef_row0')
PRECOND_FAULTS = ('precond_row1', 'precond_rows0')                    # the preconditioner at row 1 only; at the rows 0 .. nt
FAULTS = STEP_FAULTS + ESTIMATE_FAULTS[1:] + PRECOND_FAULTS

# ---- the cells of tests/test_parabolic_tv3d_gpu.py, shared with the host test (problem of common3d.PROBLEMS, ...)
RED_CELLS = (('interior_3x3x3', 5, 1, 2), ('interior_3x3x3', 5, 17, 2), ('interior_3x3x3', 5, 1, 3), ('interior_3x3x3', 5, 17, 3),
             ('wide_basis', 30, 64, 3), ('q3_2x1x2', 6, 33, 3))                                    # (name, N, nmu, nt)
RED_SOURCE_CELL = ('aniso_2x2x1', 4, 16, 3, 3)                                                     # (name, N, nmu, nt, K)
RED_START_CELL = ('interior_3x3x3', 5, 17, 2)                                                      # from a non-zero U[0]
RED_PAD_CELL = ('interior_3x3x3', 6, 17, 2)                                                        # subdomain 1 zero-padded by 2
FOM_CELLS = (('q3_2x1x2', 17, 3, 1, False), ('interior_3x3x3', 33, 2, 2, True))                    # (name, nmu, nt, K, start value)
EST_N = {'interior_3x3x3': 5, 'aniso_2x2x1': 4, 'q3_2x1x2': 6}
# nmu in {1, 16, 17, 33} x nt in {1, 3} on every case; coef [33][4][2] = 264 doubles needs two put chunks, the added cell
# coef [64][2][2] = 256 doubles fills its one chunk exactly
EST_CELLS = tuple((name, EST_N[name], nmu, nt) for name in EST_N for nmu in (1, 16, 17, 33) for nt in (1, 3)) + (('aniso_2x2x1', 4, 64, 1),)
ITERATE_CELL = ('interior_3x3x3', 17, 17)                                                          # (name, N, nmu), nt = 2
FOM_ITERATE_CELL = ('q3_2x1x2', 17)                                                                # (name, nmu), nt = 2, a start value per column
K_ITER = (1, 2, 5)


def switch_table(nmu, nt, Q, base=None, factor=10.0, at=2, q_switch=-1):
    """theta_t [nmu, nt + 1, Q], positive: ``base`` [nmu, Q] (default mu_m^q, mu_m in [0.15, 1.2]) times a smooth factor of (k, q)
    in [0.75, 1.25] that differs from row to row, and coefficient ``q_switch`` divided by ``factor`` from row ``at`` on: a 10 x
    switch between the steps 1 and 2 (row 1 belongs to the step 0 -> 1, row 2 to the step 1 -> 2)."""
    if base is None:
        mus = np.linspace(0.15, 1.2, nmu) if nmu > 1 else np.array([0.6])
        base = np.stack([mus ** q for q in range(Q)], axis=1)
    base = np.asarray(base, dtype=np.float64)
    assert base.shape == (nmu, Q) and (base > 0.0).all()
    k, q = np.arange(nt + 1)[:, None], np.arange(Q)[None, :]
    tab = base[:, None, :] * (1.0 + 0.25 * np.sin(0.9 * k + 1.7 * q + 0.4))[None]
    tab[:, at:, q_switch] /= factor
    return np.ascontiguousarray(tab)


def coef_table(nmu, nt, seed=3):
    """coef [nmu, nt + 1, 2]: positive, distinct per column, row and entry."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([0.6 + rng.random((nmu, nt + 1)), 1.7 + rng.random((nmu, nt + 1))], axis=2))


def constant_table(thetas, nt):
    """[nmu, Q] -> [nmu, nt + 1, Q], every row the same."""
    thetas = np.asarray(thetas, dtype=np.float64)
    return np.ascontiguousarray(np.repeat(thetas[:, None, :], nt + 1, axis=1))


def time_means(theta_t, which='mean'):
    """theta_bar [nmu, Q] per column: the mean over the rows 1 .. nt summed in ascending k (nt = 1: row 1 itself).  Faults:
    'precond_row1' (row 1 alone), 'precond_rows0' (the rows 0 .. nt)."""
    theta_t = np.asarray(theta_t, dtype=np.float64)
    if which == 'precond_row1':
        return theta_t[:, 1].copy()
    first = 0 if which == 'precond_rows0' else 1
    acc = np.zeros_like(theta_t[:, 0])
    for k in range(first, theta_t.shape[1]):
        acc = acc + theta_t[:, k]
    return acc / (theta_t.shape[1] - first)


def _faulted_table(theta_t, fault):
    """The table the stepping of a faulty export would read: row k + 1 of the result is what the step k -> k + 1 solves with."""
    theta_t = np.asarray(theta_t, dtype=np.float64)
    if fault == 'column0':
        return np.repeat(theta_t[:1], theta_t.shape[0], axis=0)
    if fault == 'step_row_k':
        return np.concatenate([theta_t[:, :1], theta_t[:, :-1]], axis=1)
    if fault == 'time_mean':
        return np.repeat(time_means(theta_t)[:, None, :], theta_t.shape[1], axis=1)
    assert fault is None or fault in PRECOND_FAULTS, fault
    return theta_t


# ------------------------------------------------------------------------------------------------------- reduced trajectories
def dense_euler_tv(B, M_red, nbr, theta_rows, dt, nt, rhs=None, rhs_K=None, phi=None, U0=None, keep=None):
    """One trajectory [nt + 1, S, N] with theta_rows [nt + 1, Q]: row by row, (M + dt A(row k + 1)) u_{k+1} = M u_k + dt b_k, a
    direct solve per step (``parabolic_batch3d_ref.dense_euler`` with the operator rebuilt per step)."""
    import scipy.sparse as sp
    S, N = np.asarray(M_red).shape[:2]
    M = rb.mass_operator(M_red)
    U = np.zeros((nt + 1, S * N))
    if U0 is not None:
        U[0] = np.asarray(U0, dtype=np.float64).reshape(S * N)
    for k in range(nt):
        lhs = rb.step_operator(B, M_red, nbr, theta_rows[k + 1], dt)
        if keep is not None:
            lhs = lhs + sp.diags(1.0 - np.asarray(keep, dtype=np.float64).ravel())
        U[k + 1] = splu(lhs.tocsc()).solve(M @ U[k] + dt * rb.step_rhs(S, N, k, rhs, rhs_K, phi))
    return U.reshape(nt + 1, S, N)


def dense_euler_batch_tv(B, M_red, nbr, theta_t, dt, nt, rhs=None, rhs_K=None, phis=None, U0=None, keep=None, fault=None):
    """[nt + 1, S, N, nmu]: column m with theta_t[m] [nt + 1, Q] (and phis[m]); U0 [S, N] or [S, N, nmu]."""
    tab = _faulted_table(theta_t, fault)
    cols = []
    for m in range(tab.shape[0]):
        u0 = None if U0 is None else (U0 if np.ndim(U0) == 2 else np.asarray(U0)[:, :, m])
        cols.append(dense_euler_tv(B, M_red, nbr, tab[m], dt, nt, rhs=rhs, rhs_K=rhs_K, phi=None if phis is None else phis[m], U0=u0,
                                   keep=keep))
    return np.stack(cols, axis=-1)


def reduced_precond(B, M_red, nbr, theta_t, dt, fault=None, coarse=True):
    """The two-level preconditioner of a reduced ``_tv`` call: ``StepPrecond3D`` at the mean over the columns of the time means."""
    return rb.StepPrecond3D(B, M_red, nbr, time_means(theta_t, fault or 'mean').mean(axis=0), dt, coarse=coarse)


def reduced_first_step_iterates(B, M_red, nbr, theta_t, dt, rhs, k, fault=None):
    """(x_k [S N, nmu], ratios [nmu]) of the first step from zero: the k-th PCG iterate on the row-1 operator of every column for
    the right-hand side dt rhs, with the preconditioner of the call."""
    P = reduced_precond(B, M_red, nbr, theta_t, dt, fault)
    b = dt * np.asarray(rhs, dtype=np.float64).ravel()
    out = [pcg_ref.pcg_iterate(lambda p, A=rb.step_operator(B, M_red, nbr, row[1], dt): A @ p, P.apply, b, k) for row in theta_t]
    return np.stack([x for x, _ in out], axis=1), np.array([r for _, r in out])


# ---------------------------------------------------------------------------------------------------- full-order trajectories
class BatchFomEulerTv3DRef(BatchFomEuler3DRef):
    """``BatchFomEuler3DRef`` with a step operator per (step, column): theta_t [nmu, nt + 1, Q].  The parent is built on the time
    means of the columns, so its preconditioner -- both levels on M + dt A at their mean, summed in column order -- is the one of
    the ``_tv`` call; ``fault``: one of STEP_FAULTS or PRECOND_FAULTS."""

    def __init__(self, Aq, M, S, n, theta_t, dt, nt, phis, b_K, U0=None, Phi=None, fault=None, **kw):
        theta_t = np.asarray(theta_t, dtype=np.float64)
        assert theta_t.shape[1] == nt + 1
        super().__init__(Aq, M, S, n, time_means(theta_t, fault if fault in PRECOND_FAULTS else 'mean'), dt, nt, phis, b_K, U0=U0, Phi=Phi,
                         **kw)
        tab = _faulted_table(theta_t, fault)
        self.theta_t = tab
        self.As_t = [[(self.M + self.dt * ref3.combine(Aq, tab[m, k + 1])).tocsr() for m in range(self.nmu)] for k in range(nt)]
        self.As = self.As_t[0]                                               # the first step: what ``iterate`` of the parent reads

    def trajectories(self):
        if self._traj is None:
            U = np.zeros((self.nt + 1, self.S * self.n, self.nmu))
            U[0] = self.U0
            for k in range(self.nt):
                for m in range(self.nmu):
                    U[k + 1, :, m] = splu(self.As_t[k][m].tocsc()).solve(self.rhs(m, k, U[k, :, m]))
            self._traj = U
        return self._traj


# ------------------------------------------------------------------------------------------------------------------ estimates
def estimate_outputs_tv(model, theta_t, coef_t, dt, U, keep=None, phi=None, source=None, fault=None):
    """The five outputs of lrbms3_reduced_parabolic_estimate_batch_tv as ``parabolic_estimate_batch3d_ref.estimate_outputs`` returns
    them: U [nt + 1, S, N, nmu], theta_t [nmu, nt + 1, Q], coef_t [nmu, nt + 1, 2], phi [nmu, nt + 1, K] with ``source``."""
    theta_t, coef_t, U = (np.asarray(x, dtype=np.float64) for x in (theta_t, coef_t, U))
    L, S, N, nmu = U.shape
    nt = L - 1
    assert theta_t.shape[:2] == (nmu, L) and coef_t.shape == (nmu, L, 2)
    if fault == 'column0':
        theta_t = np.repeat(theta_t[:1], nmu, axis=0)
    rows_e = np.minimum(np.arange(L) + 1, nt) if fault == 'elliptic_row_k1' else np.arange(L)
    X = np.ascontiguousarray(U.transpose(1, 2, 0, 3)).reshape(S, N, L * nmu)                  # column (k, m)
    th = theta_t[:, rows_e].transpose(1, 0, 2).reshape(L * nmu, -1)
    ph = None if source is None else np.asarray(phi, dtype=np.float64).transpose(1, 0, 2).reshape(L * nmu, -1)
    nc, r, df = (x.reshape(S, L, nmu).transpose(1, 0, 2) for x in pe.elliptic_rows(model, th, X, ph, source))
    dU = U[1:] - U[:-1]
    Xd = np.ascontiguousarray(dU.transpose(1, 2, 0, 3)).reshape(S, N, nt * nmu)
    nc_dU = pe.elliptic_rows(model, np.tile(theta_t[:, 0], (nt, 1)), Xd)[0].reshape(S, nt, nmu).transpose(1, 0, 2)      # reads no theta
    tr2 = np.concatenate([pe.time_residual2(model, theta_t[:, k if fault == 'residual_row_k' else k + 1], dU[k:k + 1], keep)
                          for k in range(nt)])
    cf = np.repeat(coef_t[:, :1], L, axis=1) if fault == 'coef_row0' else coef_t
    sc = 2.0 * np.sqrt(dt / 3.0)
    eta = sc * (cf[:, :, 0].T * np.linalg.norm(nc, axis=1) + cf[:, :, 1].T * np.linalg.norm(r + df, axis=1))
    time_residual = np.sqrt(dt / 3.0 * tr2.sum(axis=1))
    time_deriv_nc = np.sqrt(np.maximum(nc_dU, 0.0) / dt)
    est = np.linalg.norm(eta, axis=0) + np.linalg.norm(time_residual, axis=0) + np.sqrt((time_deriv_nc ** 2).sum(axis=(0, 1)))
    return dict(eta_loc=np.stack([nc, r, df]) * sc, time_deriv_nc=time_deriv_nc, time_residual=time_residual, eta=eta, est=est,
                nc_dU=nc_dU, tr2=tr2)


def source_data(S, QN, nT, K, nmu, nt, seed=5):
    """Synthetic source data of K components (the recipe of tests/test_parabolic_estimate_batch3d_gpu.py): F2 [S, K, K] SPD,
    r_fd_K [K, S, QN], bdiv_K [K, S, n_T], phi [nmu, nt + 1, K] whose first component switches between 0 and 1 from row to row."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((S, K, K))
    F2 = np.einsum('sij,skj->sik', G, G) + K * np.eye(K)[None]
    phi = rng.uniform(0.5, 1.5, size=(nmu, nt + 1, K))
    phi[:, :, 0] = (np.arange(nt + 1)[None, :] + np.arange(nmu)[:, None]) % 2
    return np.ascontiguousarray(F2), rng.standard_normal((K, S, QN)), rng.standard_normal((K, S, nT)), np.ascontiguousarray(phi)


def switching_phis(nmu, nt, K):
    """phi [nmu, nt + 1, K] of the reduced source cell: the first coefficient switches sign every step, shifted per column."""
    phis = np.empty((nmu, nt + 1, K))
    for m in range(nmu):
        phis[m, :, 0] = [1.0 if (k + m) % 2 else -1.0 for k in range(nt + 1)]
        for j in range(1, K):
            phis[m, :, j] = -1.0 + 0.02 * m + 0.3 * j
    return phis


def source_rhs(rhs, K, seed=4):
    """rhs_red_K [K, S, N] of the reduced source cell: the plain right-hand side and K - 1 random vectors of its size."""
    rng = np.random.default_rng(seed)
    rhs = np.asarray(rhs, dtype=np.float64)
    return np.ascontiguousarray(np.stack([rhs] + [rng.standard_normal(rhs.shape) * np.abs(rhs).max() for _ in range(K - 1)]))


def start_panel(S, N, nmu, scale, seed=11):
    """U[0] [S, N, nmu] of the cell that starts from a non-zero value: standard normal numbers of the size of a solution."""
    return np.ascontiguousarray(np.random.default_rng(seed).standard_normal((S, N, nmu)) * scale)


def fom_source(b, K, nmu, nt, seed=0):
    """(b_K [K, S, n], phis [nmu, nt + 1, K]) of a full-order cell -- K = 1: the plain source; K > 1: the draws of ``Call`` in
    tests/test_fom_euler_batch3d_gpu.py, in its order."""
    b = np.asarray(b, dtype=np.float64)
    if K == 1:
        return b[None], np.ones((nmu, nt + 1, 1))
    rng = np.random.default_rng(seed)
    b_K = rng.standard_normal((K,) + b.shape) * np.abs(b).max()
    return b_K, rng.uniform(0.2, 1.0, (nmu, nt + 1, K))
