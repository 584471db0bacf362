"""Batched parabolic estimates of the 3D / P2 path (lrbms3_reduced_parabolic_estimate_batch) on the host, without a
GPU: the surface is declared where it has to be, the NumPy restatement of the GPU tests (tests/parabolic_estimate_batch3d_ref.py)
reproduces the estimate of tests/parabolic3d_ref.py and tests/affine_source3d_ref.py, its deliberately wrong variants are far from
it on the inputs of the GPU cells, and the clamp max(nc, 0) of the time derivative hides nothing there.

The operators come from the CPU oracle.  ``cfg5_template`` is left out of the cell loop here (its oracle takes 16 s; it has the
operators' structure of the other cells and differs in the launch sizes only); the GPU test asserts the clamp condition for every
cell, that one included, on the product's own operators."""
import os
import re

import numpy as np
import pytest

import common3d as c3
import parabolic_estimate_batch3d_ref as ref
from parabolic3d_ref import ParabolicReduced3D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ('lrbms3_reduced_parabolic_estimate_batch_work_size', 'lrbms3_reduced_parabolic_estimate_batch')
T, NT = 0.75, 3

_ORACLE = {}


def _oracle(name):
    if name not in _ORACLE:
        p = c3.make_problem(name)
        _ORACLE[name] = (p, c3.oracle_of(p))
    return _ORACLE[name]


def _reduced(name, N, T_=T, nt=NT):
    p, o = _oracle(name)
    V = c3.make_bases3d(o.S, o.n, N, seed=ref.BASIS_SEED)
    red = ParabolicReduced3D(o, [V[ii] for ii in range(o.S)], T_, nt)
    return p, o, V, red, ref.model_from_oracle(p, o, red.rd, red.M_blocks, N)


def _coef(o, mus):
    return np.array([[np.sqrt(o.gamma(mu, o.mu_bar) / o.alpha(mu, o.mu_bar)), 1.0 / np.sqrt(o.alpha(mu, o.mu_hat) * o.alpha(mu, o.mu_bar))]
                     for mu in mus])


def _against(out, m, est, parts, dt, tol, tag):
    nc, r, df, tres, tdnc = parts
    got = dict(eta_loc=np.stack([x[:, :, m].T for x in out['eta_loc']]), tdnc2=out['time_deriv_nc'][:, :, m].T ** 2 * dt,
               tr2=out['time_residual'][:, m] ** 2 * 3.0 / dt, est=out['est'][m])
    want = dict(eta_loc=np.stack([nc, r, df]), tdnc2=tdnc ** 2 * dt, tr2=tres ** 2 * 3.0 / dt, est=est)
    for k in want:
        err = float(np.abs(got[k] - want[k]).max() / np.abs(want[k]).max())
        assert err <= tol, (tag, k, err)


def test_exports_are_declared_and_bound():
    from pylrbms_amd._native3d import SIGNATURES3, Native3DContext
    with open(os.path.join(ROOT, 'include', 'lrbms3d_hip.h')) as fh:
        header = fh.read()
    for name in EXPORTS:
        assert re.search(r'\b{}\s*\('.format(name), header), name
        assert name in SIGNATURES3, name
    assert len(SIGNATURES3[EXPORTS[0]][1]) == 4 and len(SIGNATURES3[EXPORTS[1]][1]) == 41      # ctx + 3 / ctx + 40
    assert callable(Native3DContext.reduced_parabolic_estimate_batch)


def test_estimate_batch_of_the_reduced_model_keeps_the_loop_by_default():
    import inspect
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import InstationaryReducedDiscretization3D
    sig = inspect.signature(InstationaryReducedDiscretization3D.estimate_batch)
    assert list(sig.parameters) == ['self', 'U', 'mus', 'decompose', 'native'] and sig.parameters['native'].default is False


@pytest.mark.parametrize('name', ('aniso_2x2x1', 'q3_2x1x2'))
def test_restatement_is_the_estimate_of_the_3d_reference(name):
    """Columns = the reduced trajectories of three parameters: every part of ``ParabolicReduced3D.estimate`` to 1e-12."""
    N = c3.PROBLEMS[name][5]
    p, o, V, red, model = _reduced(name, N)
    mus = (0.2, p['mu'], 0.9)
    U = np.stack([red.solve(mu).reshape(NT + 1, o.S, N) for mu in mus], axis=3)
    out = ref.estimate_outputs(model, [c3.theta_of(p, mu) for mu in mus], _coef(o, mus), red.dt, U)
    for m, mu in enumerate(mus):
        est, parts = red.estimate(U[..., m].reshape(NT + 1, -1), mu)
        assert est > 0.0
        _against(out, m, est, parts, red.dt, 1e-12, (name, mu))


def _source_model():
    """aniso_2x2x1 with the two-component source of tests/affine_source3d_ref.py and its switching PARABOLIC coefficients: the
    model, the source dict (F2, dense r_fd_K from the reduced models of the single components) and the reference."""
    from affine_source3d_ref import PARABOLIC, AffineSource3D, ParabolicSourceReduced3D
    from oracle.lrbms3d import Reductor3D
    name = 'aniso_2x2x1'
    N = c3.PROBLEMS[name][5]
    p = c3.make_problem(name)
    src = AffineSource3D(p, coeffs=PARABOLIC)
    o = src.d
    V = c3.make_bases3d(o.S, o.n, N, seed=ref.BASIS_SEED)
    red = ParabolicSourceReduced3D(src, V, T, NT)
    model = ref.model_from_oracle(p, o, red.rd, red.M_blocks, N)
    r_fd_K = []
    for j in range(src.K):
        oj = src.component(j)
        rdj = Reductor3D(oj, [V[ii] for ii in range(o.S)]).reduce()
        r_fd_K.append(np.stack([c3.oracle_dense_blocks(dict(p, N=N), oj, rdj, ii)['r_fd'] for ii in range(o.S)]))
    return p, o, src, red, model, dict(F2=src.gram(), r_fd_K=np.stack(r_fd_K)), N


def test_restatement_with_a_source_is_the_estimate_of_the_source_reference_and_sees_a_shifted_row():
    """``ParabolicSourceReduced3D.estimate`` to 1e-12; the source row of step k + 1 used for U_k misses by more than 1e-6."""
    p, o, src, red, model, source, N = _source_model()
    mus = (0.2, p['mu'], 0.9)
    U = np.stack([red.solve(mu).reshape(NT + 1, o.S, N) for mu in mus], axis=3)
    phi = np.stack([red_table for red_table in (np.stack([src.coefficients(mu, k * red.dt) for k in range(NT + 1)]) for mu in mus)])
    assert len({tuple(row) for row in phi[0]}) > 1                  # the coefficient switches inside the trajectory
    thetas = [c3.theta_of(p, mu) for mu in mus]
    out = ref.estimate_outputs(model, thetas, _coef(o, mus), red.dt, U, phi=phi, source=source)
    for m, mu in enumerate(mus):
        est, parts = red.estimate(U[..., m].reshape(NT + 1, -1), mu)
        _against(out, m, est, parts, red.dt, 1e-12, ('source', mu))
    bad = ref.estimate_outputs(model, thetas, _coef(o, mus), red.dt, U, phi=phi, source=source, shift_source=True)
    miss = ref.worst(bad, out, red.dt)
    assert miss['eta_loc'] > 1e-6 and miss['est'] > 1e-6, miss


MUTANTS = {'drop_slot': ('tr2',), 'diagonal_inverse': ('tr2',), 'drop_boundary_elements': ('eta_loc', 'tdnc2'),
           'drop_cross': ('eta_loc', 'tdnc2'), 'swap_coef': ('eta',)}


@pytest.mark.parametrize('name, N, nmu, nt', [c for c in ref.CELLS if c[0] != 'cfg5_template'])
def test_wrong_variants_miss_and_the_clamp_hides_nothing_at_the_gpu_cells(name, N, nmu, nt):
    """On the inputs of the GPU cell: every mutant of the restatement is more than 1e-6 (of the largest entry) away from it in the
    outputs it touches and in est, and no entry of nc(U[k+1] - U[k]) lies below -1e-12 of the largest one."""
    p, o, V, red, model = _reduced(name, N)
    U = ref.panel(o.S, N, nmu, nt)
    thetas, coef = ref.cell_thetas(p, nmu), ref.coefficients(nmu)
    good = ref.estimate_outputs(model, thetas, coef, ref.DT, U)
    assert good['nc_dU'].min() >= -1e-12 * good['nc_dU'].max() and good['nc_dU'].max() > 0.0
    slot = next(sl for sl in range(7) if sl != ref.SELF and (model['nbr'][:, sl] >= 0).any())
    for mutant, touched in MUTANTS.items():
        bad = ref.estimate_outputs(model, thetas, coef, ref.DT, U, **{mutant: slot if mutant == 'drop_slot' else True})
        miss = ref.worst(bad, good, ref.DT)
        assert all(miss[k] > 1e-6 for k in touched + ('est',)), (mutant, miss)
