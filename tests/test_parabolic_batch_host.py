"""Batched reduced trajectories (lrbms_reduced_implicit_euler_batch) on the host, without a GPU: the public surface is declared
everywhere it has to be, and the NumPy reference of the GPU tests (tests/parabolic_batch_ref.py) reproduces the oracle's
reduced implicit Euler."""
import os
import re

import numpy as np

from common import oracle_from_problem
from parabolic_batch_ref import dense_euler, dense_euler_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ('lrbms_reduced_implicit_euler_batch_work_size', 'lrbms_reduced_implicit_euler_batch',
           'lrbms_reduced_implicit_euler_batch_src')


def test_exports_are_declared_and_solve_batch_is_overridden():
    from pylrbms_amd._native import SIGNATURES
    from pylrbms_amd.reductor import InstationaryReducedDiscretization, ReducedDiscretization
    with open(os.path.join(ROOT, 'include', 'lrbms_hip.h')) as fh:
        header = fh.read()
    for name in EXPORTS:
        assert re.search(r'\b{}\s*\('.format(name), header), name
        assert name in SIGNATURES, name
    # argument counts: ctx + 15 / 17 (the header is the contract; test_capi_symbols.py checks the types one by one)
    assert len(SIGNATURES['lrbms_reduced_implicit_euler_batch'][1]) == 16
    assert len(SIGNATURES['lrbms_reduced_implicit_euler_batch_src'][1]) == 18
    # defined on the parabolic class itself: the inherited method returns STATIONARY solutions
    assert 'solve_batch' in vars(InstationaryReducedDiscretization)
    assert InstationaryReducedDiscretization.solve_batch is not ReducedDiscretization.solve_batch


def _fixed_slot_model(p, o, bases):
    """B [Q, S, 5, N, N], M_red [S, N, N], rhs [S, N] of the oracle's reduced model in the product's fixed-slot layout."""
    from oracle.lrbms import OracleReductor
    ored = OracleReductor(o, bases)
    rd = ored.reduce()
    nbr = np.asarray(p['grid'].neighbor_slots)
    S, N = o.S, bases[0].shape[1]
    B = np.zeros((o.Q, S, 5, N, N))
    for ii in range(S):
        assert nbr[ii, 2] == ii
        for slot in range(5):
            jj = int(nbr[ii, slot])
            if jj >= 0:
                for q in range(o.Q):
                    B[q, ii, slot] = rd.op[ii][jj][q]
    return ored, rd, nbr, B, np.stack(rd.l2), np.stack(rd.rhs)


def test_dense_reference_reproduces_the_oracle_reduced_trajectory():
    """Both are direct solves of the same matrices: 1e-12."""
    from oracle.parabolic import OracleParabolicReduced
    from pylrbms_amd import OS2015_academic_problem
    p = OS2015_academic_problem.init_grid_and_problem({'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 4})
    o = oracle_from_problem(p)
    rng = np.random.default_rng(2)
    N = 4
    bases = [np.column_stack([np.ones(o.n), rng.standard_normal((o.n, N - 1))]) for _ in range(o.S)]
    ored, rd, nbr, B, M_red, rhs = _fixed_slot_model(p, o, bases)
    T, nt = 0.5, 4
    opr = OracleParabolicReduced(ored, rd, T, nt)
    mus = (0.2, 0.4, 0.9)
    thetas = [o.theta(mu) for mu in mus]
    U = dense_euler_batch(B, M_red, nbr, thetas, T / nt, nt, rhs=rhs)
    assert U.shape == (nt + 1, o.S, N, len(mus))
    for m, mu in enumerate(mus):
        u_o = opr.solve(mu).reshape(nt + 1, o.S, N)
        assert np.abs(u_o[1:]).max() > 0.0
        assert np.abs(U[..., m] - u_o).max() <= 1e-12 * np.abs(u_o).max(), mu
    # K components with a coefficient table: phi = (1, 1) over two halves of rhs is the plain trajectory; U0 is honoured
    rhs_K = np.stack([0.25 * rhs, 0.75 * rhs])
    U2 = dense_euler(B, M_red, nbr, thetas[1], T / nt, nt, rhs_K=rhs_K, phi=np.ones((nt + 1, 2)))
    assert np.abs(U2 - U[..., 1]).max() <= 1e-12 * np.abs(U[..., 1]).max()
    U3 = dense_euler(B, M_red, nbr, thetas[1], T / nt, 1, rhs=rhs, U0=U[2, :, :, 1])
    assert np.abs(U3[1] - U[3, :, :, 1]).max() <= 1e-12 * np.abs(U[3, :, :, 1]).max()
