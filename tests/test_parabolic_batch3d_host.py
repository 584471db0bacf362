"""Batched reduced trajectories of the 3D / P2 path (lrbms3_reduced_implicit_euler_batch) on the host, without a GPU: the public
surface is declared everywhere it has to be, and the NumPy reference of the GPU tests (tests/parabolic_batch3d_ref.py)
reproduces the reduced implicit Euler of tests/parabolic3d_ref.py, ragged bases included."""
import os
import re

import numpy as np

import common3d as c3
from parabolic3d_ref import ParabolicReduced3D
from parabolic_batch3d_ref import StepPrecond3D, dense_euler, dense_euler_batch, pcg_dense, step_operator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ('lrbms3_reduced_implicit_euler_batch_work_size', 'lrbms3_reduced_implicit_euler_batch',
           'lrbms3_reduced_implicit_euler_batch_src')


def test_exports_are_declared_and_bound():
    from pylrbms_amd._native3d import SIGNATURES3, Native3DContext
    with open(os.path.join(ROOT, 'include', 'lrbms3d_hip.h')) as fh:
        header = fh.read()
    for name in EXPORTS:
        assert re.search(r'\b{}\s*\('.format(name), header), name
        assert name in SIGNATURES3, name
    # argument counts: ctx + 2 / 15 / 17 (the header is the contract; test_capi_symbols.py checks the types one by one)
    assert len(SIGNATURES3['lrbms3_reduced_implicit_euler_batch_work_size'][1]) == 3
    assert len(SIGNATURES3['lrbms3_reduced_implicit_euler_batch'][1]) == 16
    assert len(SIGNATURES3['lrbms3_reduced_implicit_euler_batch_src'][1]) == 18
    assert callable(Native3DContext.reduced_implicit_euler_batch) and callable(Native3DContext.reduced_implicit_euler_batch_src)


def test_solve_batch_of_the_parabolic_reduced_model_is_its_own_method():
    """The inherited method returns STATIONARY solutions [len(mus), S, N] without an error."""
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import ReducedDiscretization3D
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import InstationaryReducedDiscretization3D
    assert 'solve_batch' in vars(InstationaryReducedDiscretization3D)
    assert InstationaryReducedDiscretization3D.solve_batch is not ReducedDiscretization3D.solve_batch


def padded_model(p, red, N):
    """B [Q, S, 7, N, N], M_red [S, N, N], rhs [S, N] and keep [S, N] of a ``ParabolicReduced3D`` in the product's 7-slot layout,
    local bases of fewer than N vectors zero-padded."""
    o = red.o
    nbr = np.asarray(p['grid'].neighbor_slots).reshape(o.S, 7)
    B, M, rhs, keep = np.zeros((o.Q, o.S, 7, N, N)), np.zeros((o.S, N, N)), np.zeros((o.S, N)), np.zeros((o.S, N))
    for ii in range(o.S):
        ni = red.bases[ii].shape[1]
        assert nbr[ii, 3] == ii
        M[ii, :ni, :ni] = red.M_blocks[ii]
        rhs[ii, :ni] = red.rd.rhs[ii]
        keep[ii, :ni] = 1.0
        for slot in range(7):
            jj = int(nbr[ii, slot])
            if jj >= 0:
                nj = red.bases[jj].shape[1]
                for q in range(o.Q):
                    B[q, ii, slot, :ni, :nj] = red.rd.op[ii][jj][q]
    return nbr, B, M, rhs, keep


def test_dense_reference_reproduces_the_reduced_trajectory_of_the_3d_reference():
    """Both are direct solves of the same matrices: 1e-12.  Subdomain 1 has two vectors fewer (a ragged basis)."""
    p = c3.make_problem('aniso_2x2x1')
    o = c3.oracle_of(p)
    N, T, nt = 4, 0.2, 4
    V = c3.make_bases3d(o.S, o.n, N, seed=5)
    sizes = [N, N - 2, N, N]
    red = ParabolicReduced3D(o, [V[ii][:, :sizes[ii]] for ii in range(o.S)], T, nt)
    nbr, B, M, rhs, keep = padded_model(p, red, N)
    mus = (0.2, p['mu'], 0.9)
    thetas = [c3.theta_of(p, mu) for mu in mus]
    U = dense_euler_batch(B, M, nbr, thetas, T / nt, nt, rhs=rhs, keep=keep)
    assert U.shape == (nt + 1, o.S, N, len(mus))
    assert np.all(U[:, keep == 0, :] == 0.0)
    for m, mu in enumerate(mus):
        u_o = red.solve(mu)
        assert np.abs(u_o[1:]).max() > 0.0
        got = U[..., m].reshape(nt + 1, -1)[:, keep.ravel() == 1]
        assert np.abs(got - u_o).max() <= 1e-12 * np.abs(u_o).max(), mu
    # K components with a coefficient table: phi = (1, 1) over two parts of rhs is the plain trajectory; U0 is honoured
    rhs_K = np.stack([0.25 * rhs, 0.75 * rhs])
    U2 = dense_euler(B, M, nbr, thetas[1], T / nt, nt, rhs_K=rhs_K, phi=np.ones((nt + 1, 2)), keep=keep)
    assert np.abs(U2 - U[..., 1]).max() <= 1e-12 * np.abs(U[..., 1]).max()
    U3 = dense_euler(B, M, nbr, thetas[1], T / nt, 1, rhs=rhs, U0=U[2, :, :, 1], keep=keep)
    assert np.abs(U3[1] - U[3, :, :, 1]).max() <= 1e-12 * np.abs(U[3, :, :, 1]).max()


def test_restated_preconditioner_is_spd_and_loses_its_coarse_level_without_a_first_vector():
    """The two-level preconditioner of the step operator is symmetric positive definite and converges; with the first basis
    vector of one subdomain zeroed the coarse matrix has a zero row: no Cholesky factor, block-Jacobi alone."""
    p = c3.make_problem('aniso_2x2x1')
    o = c3.oracle_of(p)
    N, dt = 4, 0.05
    V = c3.make_bases3d(o.S, o.n, N, seed=5)
    red = ParabolicReduced3D(o, [V[ii] for ii in range(o.S)], 0.2, 4)
    nbr, B, M, rhs, _ = padded_model(p, red, N)
    th = c3.theta_of(p, 0.5)
    P = StepPrecond3D(B, M, nbr, th, dt)
    assert P.has_coarse
    Minv = P.matrix()
    assert np.abs(Minv - Minv.T).max() <= 1e-12 * np.abs(Minv).max() and np.linalg.eigvalsh(0.5 * (Minv + Minv.T)).min() > 0.0
    A = step_operator(B, M, nbr, th, dt).toarray()
    x, ratio = pcg_dense(A, Minv, dt * rhs.ravel(), 40)
    assert ratio < 1e-12 and np.abs(A @ x - dt * rhs.ravel()).max() <= 1e-11 * np.abs(dt * rhs).max()
    V[2, :, 0] = 0.0
    red0 = ParabolicReduced3D(o, [V[ii] for ii in range(o.S)], 0.2, 4)
    _, B0, M0, _, _ = padded_model(p, red0, N)
    assert not StepPrecond3D(B0, M0, nbr, th, dt).has_coarse
