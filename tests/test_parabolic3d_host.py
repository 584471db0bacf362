"""The CPU reference of the parabolic 3D path (tests/parabolic3d_ref.py, a restatement of oracle/parabolic.py on the 3D oracle)
checked on its own, without a GPU: the properties the GPU tests then rely on."""
import numpy as np
import scipy.sparse.linalg as spla

import common3d as c3
from parabolic3d_ref import Parabolic3D, ParabolicReduced3D


def _setup(name='aniso_2x2x1'):
    p = c3.make_problem(name)
    return p, c3.oracle_of(p)


def test_implicit_euler_with_a_long_horizon_tends_to_the_stationary_solution():
    p, o = _setup()
    mu = p['mu']
    U = Parabolic3D(o, 400.0, 16).solve(mu)
    assert np.abs(U[0]).max() == 0.0
    assert c3.rel(U[-1].reshape(-1), o.solve(mu)) < 1e-8


def test_time_residual_is_the_dense_mass_inverse_norm():
    p, o = _setup()
    mu = p['mu']
    ref = Parabolic3D(o, 1.0, 3)
    dU = np.random.default_rng(4).standard_normal((2, o.S, o.n))
    got = ref.time_residual2(dU, mu)
    A, M = o.system_matrix(mu).toarray(), o.M.toarray()
    for k in range(2):
        y = A @ dU[k].reshape(-1)
        assert abs(got[k] - y @ np.linalg.solve(M, y)) < 1e-10 * abs(got[k])
    # the mass matrix is element-block-diagonal: the block inverse gives the same norm
    lu = spla.splu(o.M.tocsc())
    y = A @ dU[0].reshape(-1)
    assert abs(lu.solve(y) @ y - got[0]) < 1e-10 * abs(got[0])


def test_time_derivative_nc_of_a_constant_trajectory_vanishes():
    p, o = _setup()
    mu = p['mu']
    u = np.random.default_rng(2).standard_normal(o.ndof)
    U = np.stack([u, u, u])
    est, (nc, r, df, tres, tdnc) = Parabolic3D(o, 1.0, 2).estimate(U, mu)
    assert np.abs(tdnc).max() == 0.0 and np.abs(tres).max() == 0.0
    assert nc.shape == (o.S, 3) and tdnc.shape == (o.S, 2) and tres.shape == (2,)
    assert np.all(nc > 0.0) and np.isfinite(est)


def test_reduced_model_on_snapshot_spans_reproduces_the_trajectory():
    """With the whole trajectory in every local basis the reduced implicit Euler is the full-order one, and so are the parts of
    the estimate that do not involve M_red^-1 (the reduced time residual measures A dU in the dual norm of the reduced space)."""
    p, o = _setup()
    mu = p['mu']
    T, nt = 0.5, 3
    full = Parabolic3D(o, T, nt)
    U = full.solve(mu)
    bases = [np.linalg.qr(np.stack([np.ones(o.n)] + [U[k, ii] for k in range(1, nt + 1)], axis=1))[0] for ii in range(o.S)]
    red = ParabolicReduced3D(o, bases, T, nt)
    u = red.solve(mu)
    UU = np.stack([np.stack([bases[ii] @ c for ii, c in enumerate(red.split(uk))]) for uk in u])
    assert c3.rel(UU, U) < 1e-9
    est, parts = full.estimate(U, mu)
    est_r, parts_r = red.estimate(u, mu)
    for i in (0, 1, 2, 4):
        assert c3.rel(parts_r[i], parts[i]) < 1e-7
    assert np.all(parts_r[3] <= parts[3] * (1 + 1e-12))
