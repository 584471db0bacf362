"""The NumPy restatement of lrbms_fom_solve_batch's preconditioner (tests/fom_batch_ref.py), pinned on the CPU.

- For one column (theta_bar == theta) it is ``pcg_ref.FomPrecond``, exactly.
- With the coarse level built at another theta than the column's it is still symmetric positive definite.
- ``pcg_ref.pcg_iterate`` with it converges to a direct solve on the (4, 3) grid, for every column of a small call.
- ``mean_theta`` sums in column order."""
import numpy as np
from scipy.sparse.linalg import spsolve

import fom_batch_ref
import pcg_ref

_ORACLE = {}
MUS = (0.1, 0.37, 1.0)


def _oracle(shape=(4, 3)):
    if shape not in _ORACLE:
        from pylrbms_amd import multiscale_problem
        from common import oracle_from_problem
        p = multiscale_problem.init_grid_and_problem({'num_subdomains': list(shape), 'coarse_per_subdomain': 2})
        d = oracle_from_problem(p)
        As = [d.assemble_global(mu).tocsr() for mu in MUS]
        A_bar = (As[0] + As[1] + As[2]) / 3.0          # the operator is affine in theta = [1, mu]: A(theta_bar) = mean of A(theta_m)
        _ORACLE[shape] = (d, As, A_bar.tocsr())
    return _ORACLE[shape]


def test_one_column_is_the_single_solver_preconditioner_exactly():
    d, As, _ = _oracle()
    rng = np.random.default_rng(0)
    R = rng.standard_normal((d.S * d.n, 3))
    for coarse in (0, 1):
        F = pcg_ref.FomPrecond(As[1], d.S, d.n, coarse)
        B = fom_batch_ref.BatchFomPrecond(As[1], As[1], d.S, d.n, coarse)
        assert B.has_coarse == F.has_coarse == (coarse == 1)
        assert np.array_equal(B.Minv, F.Minv)
        if coarse:
            assert np.array_equal(B.A0, F.A0)
        assert np.array_equal(B.apply(R), F.apply(R))
        assert np.array_equal(B.apply(R[:, 0]), F.apply(R[:, 0]))


def test_no_coarse_level_below_four_subdomains():
    d, As, A_bar = _oracle((3, 1))
    assert not fom_batch_ref.BatchFomPrecond(As[0], A_bar, d.S, d.n, 1).has_coarse


def test_preconditioner_with_the_mean_theta_coarse_level_is_spd():
    d, As, A_bar = _oracle()
    for A in (As[0], As[2]):
        for coarse in (0, 1):
            M = fom_batch_ref.BatchFomPrecond(A, A_bar, d.S, d.n, coarse)
            lo, asym = pcg_ref.spd_check(pcg_ref.precond_matrix(M.apply, d.S * d.n))
            assert lo > 0.0 and asym < 1e-12, (coarse, lo, asym)


def test_pcg_with_it_converges_to_the_direct_solve():
    d, As, A_bar = _oracle()
    b = np.asarray(d.b, dtype=np.float64).ravel()
    for A in As:
        M = fom_batch_ref.BatchFomPrecond(A, A_bar, d.S, d.n, 1)
        x, rel = pcg_ref.pcg_iterate(lambda p: A @ p, M.apply, b, 400)
        ref = spsolve(A.tocsc(), b)
        assert rel < 1e-10, rel
        assert np.abs(x - ref).max() < 1e-8 * np.abs(ref).max()
    # the coarse level matters for the iterates: without it x_2 differs visibly
    M0 = fom_batch_ref.BatchFomPrecond(As[0], A_bar, d.S, d.n, 0)
    M1 = fom_batch_ref.BatchFomPrecond(As[0], A_bar, d.S, d.n, 1)
    x0, _ = pcg_ref.pcg_iterate(lambda p: As[0] @ p, M0.apply, b, 2)
    x1, _ = pcg_ref.pcg_iterate(lambda p: As[0] @ p, M1.apply, b, 2)
    assert np.linalg.norm(x0 - x1) > 1e-6 * np.linalg.norm(x1)
    # ... and so does the theta it is built at
    Mc = fom_batch_ref.BatchFomPrecond(As[0], As[0], d.S, d.n, 1)
    xc, _ = pcg_ref.pcg_iterate(lambda p: As[0] @ p, Mc.apply, b, 2)
    assert np.linalg.norm(xc - x1) > 1e-6 * np.linalg.norm(x1)


def test_mean_theta_sums_in_column_order():
    th = np.array([[1.0, 0.1], [1.0, 1e-17], [1.0, 0.7]])
    want = np.array([(1.0 + 1.0 + 1.0) / 3, ((0.1 + 1e-17) + 0.7) / 3])
    assert np.array_equal(fom_batch_ref.mean_theta(th), want)
