"""CPU reference of the parabolic corrector trajectories (``lrbms_local_correction_euler``), built on
``oracle.lrbms``: test infrastructure only.

On the neighbourhood N(ii) of a marked subdomain (``OracleDiscretization.local_correction_system``: the SWIPDG operator with the
all-Dirichlet outer boundary, assembled from scratch) implicit Euler with zero initial value,

    (M_N + dt A_N(mu)) x_{k+1} = M_N x_k + dt sum_j phi[k+1][j] b_j|_N,   k = 0 .. nt-1,

with M_N the rows / columns of the oracle's global ``l2_product`` and ONE sparse LU for all steps; x_k restricted to ii is kept.
"""
import numpy as np
import scipy.sparse.linalg as spla

CORR_TOL = 1e-8        # the tolerance of tests/test_enrichment_gpu.py for the stationary correctors (iterative vs direct solve)
# One implicit Euler step of dt = 1e6 T (T = 0.05) against the stationary corrector, both solved directly on the CPU: the gap is
# 7.1e-7 on the 3 x 3 grid of the tests (7.1e-3 at 1e2 T, 7.1e-5 at 1e4 T: first order in 1 / dt;
# tests/test_parabolic_enrichment_host.py asserts it stays below LIMIT_GAP).  The GPU limit test compares the kernel's one huge step
# with the native stationary correctors at CORR_TOL * LIMIT_FACTOR = the solver tolerance plus this gap of the two PROBLEMS.
LIMIT_GAP = 1e-6
LIMIT_FACTOR = 1.0 + LIMIT_GAP / CORR_TOL


def corrector_trajectory(o, ii, mu, dt, nt, phi=None, b_K=None):
    """[nt, n]: row k - 1 = x_k on subdomain ``ii``.  ``phi`` [nt + 1, K] (row k = time of step k; default: ones, K = 1),
    ``b_K`` [K, ndof] global load vectors (default: the oracle's own ``b``)."""
    A, b, hood, dofs = o.local_correction_system(ii, mu)
    M = o.l2_product.tocsr()[dofs, :][:, dofs]
    bK = b[None, :] if b_K is None else np.asarray(b_K)[:, dofs]
    phi = np.ones((nt + 1, bK.shape[0])) if phi is None else np.asarray(phi, dtype=np.float64)
    assert phi.shape == (nt + 1, bK.shape[0])
    lu = spla.splu((M + dt * A).tocsc())
    k0 = hood.index(ii)
    x = np.zeros(len(dofs))
    out = np.zeros((nt, o.n))
    for k in range(nt):
        x = lu.solve(M @ x + dt * (phi[k + 1] @ bK))
        out[k] = x[k0 * o.n:(k0 + 1) * o.n]
    return out


def corrector_trajectories(o, marked, mu, dt, nt, phi=None, b_K=None):
    """[len(marked), n, nt], the layout of the native call (step fastest)."""
    return np.stack([corrector_trajectory(o, ii, mu, dt, nt, phi, b_K).T for ii in marked])


def stationary_limit_gap(o, marked, mu, dt):
    """max over ``marked`` of |x_1(dt) - x_stationary|_max / |x_stationary|_max: how far ONE implicit Euler step of size ``dt``
    is from the stationary corrector ``oracle.solve_for_local_correction`` (x_1 = (A + M / dt)^-1 b, so the gap is
    O(|A^-1 M| / dt)), both solved directly on the CPU."""
    gap = 0.0
    for ii in marked:
        stat = o.solve_for_local_correction(ii, mu)
        one = corrector_trajectory(o, ii, mu, dt, 1)[0]
        gap = max(gap, float(np.abs(one - stat).max() / np.abs(stat).max()))
    return gap


def max_rel(got, ref):
    """max_k |got_k - ref_k|_max / max_k |ref_k|_max for trajectories [n, nt]: relative to the largest step."""
    return float(np.abs(got - ref).max() / np.abs(ref).max())
