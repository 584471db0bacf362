"""Batched reduced trajectories on the GPU: lrbms_reduced_implicit_euler_batch(_src) -- nmu <= 64 parameters of the parabolic
reduced model, every time step one panel PCG -- against the dense reference tests/parabolic_batch_ref.py (pinned to the oracle
in tests/test_parabolic_batch_host.py), the single-parameter export, a NumPy PCG with the restated preconditioner, and through
``InstationaryReducedDiscretization.solve_batch``.

Shapes: the grid of the iterate tests (4 x 3 subdomains, k_c = 2, n_T = 32), nt <= 4, dt = 0.05 / nt."""
import numpy as np
import pytest

import pcg_ref
from parabolic_batch_ref import column_errors, dense_euler, dense_euler_batch, mass_operator, step_blocks, true_residuals
from test_pcg_iterates_gpu import (KC, SWEEP_GRID, _dev, _energy_bases, _model, _problem, _raw, _theta, check_iterates,
                                   check_mutant)
from test_work_poison_gpu import poisoned

pytestmark = pytest.mark.gpu

NMAX = 64
T_END = 0.05
TOL_TRAJ = 1e-8            # trajectories against a direct solve: the tolerance of tests/test_parabolic_gpu.py
DISPATCH_CELLS = ((5, 1), (40, 16), (3, 17), (24, 17), (40, 32), (16, 64), (32, 33), (40, 47), (48, 64), (64, 33))
SINGLE_CELLS = ((40, 16), (24, 17), (48, 64))
VALU_CELLS = ((48, 17), (64, 40))
ITERATE_CELLS = ((24, 17), (40, 47))
SRC_ITERATE_CELL = (6, 20, 3)

_SYS = {}
_REF = {}


def _system():
    """Engine, neighbour table and the reduced system (B_sys, rhs_red, M_red as host arrays) at NMAX energy-orthonormal columns."""
    if not _SYS:
        m = _model(SWEEP_GRID, NMAX)
        eng = m['eng']
        buf = eng.project_and_estimate(eng.ctx.from_numpy(_energy_bases(eng, NMAX, seed=5)))
        _SYS.update(eng=eng, nbr=m['nbr'], Q=m['Q'], B=buf['sys'][0].cpu().numpy(), rhs=buf['sys'][1].cpu().numpy(),
                    M=buf['sys'][3].cpu().numpy())
    return _SYS


def _cut(N):
    s = _system()
    return (np.ascontiguousarray(s['B'][..., :N, :N]), np.ascontiguousarray(s['M'][:, :N, :N]), np.ascontiguousarray(s['rhs'][:, :N]))


def _thetas(nmu):
    return np.ascontiguousarray(np.stack([_theta(2, mu) for mu in np.linspace(0.1, 1.0, nmu)]))


def _reference(N, nmu, nt):
    """The dense trajectories of a plain cell, computed once per (N, nmu, nt) and left unchanged."""
    key = (N, nmu, nt)
    if key not in _REF:
        B, M, rhs = _cut(N)
        _REF[key] = dense_euler_batch(B, M, _system()['nbr'], _thetas(nmu), T_END / nt, nt, rhs=rhs)
        _REF[key].setflags(write=False)
    return _REF[key]


def _run(N, nmu, nt, rtol=1e-13, **kw):
    s = _system()
    ctx = s['eng'].ctx
    B, M, rhs = _cut(N)
    U, info = ctx.reduced_implicit_euler_batch(_thetas(nmu), T_END / nt, nt, _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs), rtol=rtol, **kw)
    assert tuple(U.shape) == (nt + 1, s['eng'].S, N, nmu)
    return U, info


def _dense_check(N, nmu, nt, tag):
    U, info = _run(N, nmu, nt)
    err = column_errors(U.cpu().numpy(), _reference(N, nmu, nt))
    print('PARABOLIC-BATCH {} N={} nmu={}: {} iterations, worst column error {:.2e} (tolerance {:.0e})'.format(
        tag, N, nmu, info['iterations'], float(err.max()), TOL_TRAJ))
    assert info['relative_residual'] <= 1e-13 and info['iterations'] >= nt
    assert np.isfinite(err).all() and err.max() < TOL_TRAJ, (tag, N, nmu, float(err.max()))


# ------------------------------------------------------------------------------------------------ 3. dispatch coverage
@pytest.mark.parametrize('N, nmu', DISPATCH_CELLS)
def test_trajectories_over_the_panel_dispatch(N, nmu):
    _dense_check(N, nmu, 2, 'dispatch')


# ------------------------------------------------------------------------------ 4. as accurate as the single export
@pytest.mark.parametrize('N, nmu', SINGLE_CELLS)
def test_batch_columns_are_as_accurate_as_the_single_parameter_export(N, nmu):
    """e_batch <= 10 max(e_single, 1e-13): the two use preconditioners built at different parameters and stop at different
    iterates of the same tolerance."""
    s = _system()
    ctx = s['eng'].ctx
    nt = 2
    B, M, rhs = _cut(N)
    Bd, Md, rd = _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs)
    thetas, ref = _thetas(nmu), _reference(N, nmu, nt)
    U, _ = _run(N, nmu, nt)
    e_batch = column_errors(U.cpu().numpy(), ref).max(axis=0)
    for m in sorted({0, nmu // 2, nmu - 1}):
        U1, _ = ctx.reduced_implicit_euler(thetas[m], T_END / nt, nt, Bd, Md, rd)
        e_single = float(column_errors(U1.cpu().numpy()[..., None], ref[..., m:m + 1]).max())
        print('PARABOLIC-BATCH accuracy N={} nmu={} column {}: e_single {:.2e}, e_batch {:.2e}'.format(N, nmu, m, e_single,
                                                                                                       float(e_batch[m])))
        assert e_single < TOL_TRAJ, (N, nmu, m, e_single)          # (a wrong single export would make the next line easier)
        assert e_batch[m] <= 10.0 * max(e_single, 1e-13), (N, nmu, m, e_single, float(e_batch[m]))


# ----------------------------------------------------------------------------------------------------- 5. true residuals
@pytest.mark.parametrize('N, nmu', ((24, 17), (40, 47)))
def test_true_residuals_of_every_column_and_step(N, nmu):
    """rtol = 1e-10; the recomputed residual of every column and step is <= 1e-9 (the gap between the recurrence and the true
    residual is O(eps kappa), far below rtol): no column was disturbed after it converged, none was left behind."""
    nt = 4
    U, info = _run(N, nmu, nt, rtol=1e-10)
    assert info['relative_residual'] <= 1e-10
    B, M, rhs = _cut(N)
    res = true_residuals(U.cpu().numpy(), B, M, _system()['nbr'], _thetas(nmu), T_END / nt, rhs=rhs)
    print('PARABOLIC-BATCH true residuals N={} nmu={}: worst {:.2e}, best {:.2e}'.format(N, nmu, float(res.max()), float(res.min())))
    assert np.isfinite(res).all() and res.max() <= 1e-9, float(res.max())


# -------------------------------------------------------------------------------------- 6. iterates pin the preconditioner
def _iterate_cell(N, nmu, K=0, U0=None, seed=0):
    """(run, reference) of one step (nt = 1) of the raw export with max_iter = k; x = U[1] - U[0]."""
    from pylrbms_amd._native import _dblp, c_vp
    s = _system()
    ctx, S, nbr = s['eng'].ctx, s['eng'].S, s['nbr']
    dt = T_END
    B, M, rhs = _cut(N)
    thetas = _thetas(nmu)
    As = [pcg_ref.reduced_operator(step_blocks(B, M, th, dt), nbr) for th in thetas]
    P = pcg_ref.ReducedPrecond(step_blocks(B, M, thetas.mean(axis=0), dt), nbr)       # two-level, restated at the mean theta
    if K == 0:
        cols = dt * np.repeat(rhs.reshape(-1, 1), nmu, axis=1)
        phi = None
    else:
        rng = np.random.default_rng(seed)
        rhs = np.ascontiguousarray(rng.standard_normal((K, S, N)) * np.abs(rhs).max())
        phi = np.ascontiguousarray(rng.uniform(0.2, 1.0, (nmu, 2, K)))
        cols = dt * np.einsum('mk,kn->nm', phi[:, 1], rhs.reshape(K, -1))
    scale = np.ones(nmu)
    u0 = np.zeros((S * N, nmu))
    if U0 is not None:
        u0 = U0.reshape(S * N, nmu)
        full = mass_operator(M) @ u0 + cols                               # M u_0 + dt b: the export's reference norm
        cols = np.stack([full[:, j] - As[j] @ u0[:, j] for j in range(nmu)], axis=1)
        scale = np.linalg.norm(cols, axis=0) / np.linalg.norm(full, axis=0)
    Bd, Md, rd = _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs)
    phid = None if phi is None else _dev(ctx, phi)
    work = ctx.empty(int(ctx.lib.lrbms_reduced_implicit_euler_batch_work_size(ctx.handle, N, nmu)))

    def run(k, rtol=1e-14):
        U = ctx.zeros(2, S, N, nmu)
        if U0 is not None:
            U[0] = _dev(ctx, U0)
        info = np.zeros(2)
        if K == 0:
            rc = _raw(ctx, 'lrbms_reduced_implicit_euler_batch', 2, N, nmu, _dblp(thetas), dt, 1, c_vp(Bd.data_ptr()),
                      c_vp(Md.data_ptr()), c_vp(rd.data_ptr()), c_vp(work.data_ptr()), c_vp(U.data_ptr()), float(rtol), int(k),
                      _dblp(info), ctx._stream())
        else:
            rc = _raw(ctx, 'lrbms_reduced_implicit_euler_batch_src', 2, N, K, nmu, _dblp(thetas), dt, 1, c_vp(Bd.data_ptr()),
                      c_vp(Md.data_ptr()), c_vp(rd.data_ptr()), c_vp(phid.data_ptr()), c_vp(work.data_ptr()), c_vp(U.data_ptr()),
                      float(rtol), int(k), _dblp(info), ctx._stream())
        Uh = U.cpu().numpy().reshape(2, S * N, nmu)
        return rc, Uh[1] - Uh[0], info

    def reference(k):
        out = [pcg_ref.pcg_iterate(lambda p, A=A: A @ p, P.apply, cols[:, j], k) for j, A in enumerate(As)]
        return np.stack([x for x, _ in out], axis=1), np.array([r for _, r in out]) * scale
    return run, reference, P


@pytest.mark.parametrize('N, nmu', ITERATE_CELLS)
def test_first_step_iterates_against_numpy_pcg(N, nmu):
    run, ref, P = _iterate_cell(N, nmu)
    assert P.has_coarse
    check_iterates(run, ref, 'euler batch N={} nmu={}'.format(N, nmu))


def test_first_step_iterates_of_the_source_export():
    N, nmu, K = SRC_ITERATE_CELL
    run, ref, _ = _iterate_cell(N, nmu, K=K)
    check_iterates(run, ref, 'euler batch src N={} nmu={} K={}'.format(N, nmu, K))


def test_first_step_iterates_without_the_coarse_level_miss_the_two_level_reference():
    N, nmu = ITERATE_CELLS[0]
    ctx = _system()['eng'].ctx
    run, ref, P = _iterate_cell(N, nmu)
    assert P.has_coarse
    ctx.set_option('coarse', 0)
    try:
        check_mutant(run, ref, 'euler batch N={} nmu={}'.format(N, nmu))
    finally:
        ctx.set_option('coarse', 1)


def test_first_step_iterates_from_non_zero_initial_data():
    """U[1] - U0 is the k-th iterate for the right-hand side rhs - (M + dt A) U0; the export's ratio refers to |M U0 + dt b|."""
    N, nmu = 16, 33
    s = _system()
    rng = np.random.default_rng(11)
    B, M, rhs = _cut(N)
    u_scale = np.abs(dense_euler(B, M, s['nbr'], _thetas(nmu)[0], T_END, 1, rhs=rhs)).max()      # the size of a solution
    U0 = np.ascontiguousarray(rng.standard_normal((s['eng'].S, N, nmu)) * u_scale)
    run, ref, _ = _iterate_cell(N, nmu, U0=U0)
    check_iterates(run, ref, 'euler batch U0 N={} nmu={}'.format(N, nmu))


# ------------------------------------------------------------------------------------------------------------ 7. VALU form
@pytest.mark.parametrize('N, nmu', VALU_CELLS)
def test_trajectories_valu_form(N, nmu):
    ctx = _system()['eng'].ctx
    ctx.set_option('solve_valu', 1)
    try:
        _dense_check(N, nmu, 2, 'VALU')
    finally:
        ctx.set_option('solve_valu', 0)


# ----------------------------------------------------------------------------------------------------------------- 8. _src
def test_source_export_with_one_unit_component_is_the_plain_export():
    import torch
    N, nmu, nt = 24, 17, 3
    s = _system()
    ctx = s['eng'].ctx
    B, M, rhs = _cut(N)
    U, info = _run(N, nmu, nt)
    U1, info1 = ctx.reduced_implicit_euler_batch_src(_thetas(nmu), T_END / nt, nt, _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs[None]),
                                                     np.ones((nmu, nt + 1, 1)))
    assert torch.equal(U, U1) and info == info1       # the start kernel keeps the fma order: the same bits


def test_source_export_with_a_switching_coefficient_per_column():
    N, nmu, nt, K = 24, 20, 4, 2
    s = _system()
    ctx, S = s['eng'].ctx, s['eng'].S
    B, M, rhs = _cut(N)
    rng = np.random.default_rng(4)
    rhs_K = np.ascontiguousarray(np.stack([rhs, rng.standard_normal((S, N)) * np.abs(rhs).max()]))
    phis = np.empty((nmu, nt + 1, K))
    for m in range(nmu):
        phis[m, :, 0] = [(k + m) % 2 for k in range(nt + 1)]          # 0 / 1, switching every step, shifted per column
        phis[m, :, 1] = -1.0 + 0.02 * m
    thetas = _thetas(nmu)
    U, info = ctx.reduced_implicit_euler_batch_src(thetas, T_END / nt, nt, _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs_K), phis)
    ref = dense_euler_batch(B, M, s['nbr'], thetas, T_END / nt, nt, rhs_K=rhs_K, phis=phis)
    err = column_errors(U.cpu().numpy(), ref)
    print('PARABOLIC-BATCH src K=2: {} iterations, worst column error {:.2e}'.format(info['iterations'], float(err.max())))
    assert err.max() < TOL_TRAJ, float(err.max())


# -------------------------------------------------------------------------------------------------------- 9. ragged bases
def test_zero_padded_basis_columns_stay_exactly_zero():
    from common import oracle_from_problem, ragged_padded_bases
    s = _system()
    eng = s['eng']
    N, nmu, nt = 12, 20, 3
    V, sizes = ragged_padded_bases(oracle_from_problem(_problem(SWEEP_GRID, KC)), N, seed=2)
    assert min(sizes) < N
    keep = (np.arange(N)[None, :] < np.asarray(sizes)[:, None]).astype(np.float64)
    buf = eng.project_and_estimate(eng.ctx.from_numpy(V))
    Bd, rd, Md = buf['sys'][0], buf['sys'][1], buf['sys'][3]
    thetas = _thetas(nmu)
    U, info = eng.ctx.reduced_implicit_euler_batch(thetas, T_END / nt, nt, Bd, Md, rd)
    Uh = U.cpu().numpy()
    assert np.all(Uh[:, keep == 0, :] == 0.0)
    ref = dense_euler_batch(Bd.cpu().numpy(), Md.cpu().numpy(), s['nbr'], thetas, T_END / nt, nt, rhs=rd.cpu().numpy(), keep=keep)
    assert column_errors(Uh, ref).max() < TOL_TRAJ


# -------------------------------------------------------------------------------------- 10. work buffer and repeatability
@pytest.mark.parametrize('N, nmu, valu', ((24, 17, 0), (16, 40, 1)))
def test_result_does_not_depend_on_the_work_buffer_and_repeats(N, nmu, valu):
    import torch
    ctx = _system()['eng'].ctx
    ctx.set_option('solve_valu', valu)
    try:
        U, info = poisoned(ctx, lambda: _run(N, nmu, 2))
        U2, info2 = _run(N, nmu, 2)
        assert torch.equal(U, U2) and info == info2
    finally:
        ctx.set_option('solve_valu', 0)


def test_a_column_with_a_zero_right_hand_side_returns_zeros():
    N, nmu, nt = 24, 17, 2
    s = _system()
    ctx = s['eng'].ctx
    B, M, rhs = _cut(N)
    phis = np.ones((nmu, nt + 1, 1))
    phis[5] = 0.0
    U, info = ctx.reduced_implicit_euler_batch_src(_thetas(nmu), T_END / nt, nt, _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs[None]), phis)
    Uh = U.cpu().numpy()
    assert np.all(Uh[..., 5] == 0.0)
    others = [m for m in range(nmu) if m != 5]
    assert column_errors(Uh[..., others], _reference(N, nmu, nt)[..., others]).max() < TOL_TRAJ


# --------------------------------------------------------------------------------------------------------- 11. refusals
def test_refusals_before_any_launch():
    from pylrbms_amd._native import NativeError
    from pylrbms_amd import multiscale_problem
    from pylrbms_amd.engine import Engine
    from common import theta_bar_of
    s = _system()
    ctx, S = s['eng'].ctx, s['eng'].S
    B, M, rhs = _cut(8)
    Bd, Md, rd = _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs)

    def call(c, thetas, dt, nt, Bx=Bd, Mx=Md, rx=rd):
        return c.reduced_implicit_euler_batch(thetas, dt, nt, Bx, Mx, rx)

    call(ctx, _thetas(3), 0.01, 1)                                            # the arguments below are otherwise fine
    with pytest.raises(NativeError):
        call(ctx, _thetas(65), 0.01, 1)
    with pytest.raises(NativeError):
        call(ctx, _thetas(3), 0.01, 1, ctx.zeros(2, S, 5, 65, 65), ctx.zeros(S, 65, 65), ctx.zeros(S, 65))
    with pytest.raises(NativeError):
        call(ctx, np.ones((17, 5)), 0.01, 1, ctx.zeros(5, S, 5, 8, 8))
    with pytest.raises(NativeError):
        call(ctx, _thetas(3), 0.0, 1)
    with pytest.raises(NativeError):
        call(ctx, _thetas(3), 0.01, 0)

    class TwoRanks:
        rank, size = 0, 2

    p = multiscale_problem.init_grid_and_problem({'num_subdomains': list(SWEEP_GRID), 'coarse_per_subdomain': KC}, mpi_comm=TwoRanks())
    lam = p['lambda']
    sharded = Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar_of(p))
    c2, S2 = sharded.ctx, sharded.S
    assert sharded.S_ext > S2
    with pytest.raises(NativeError, match='one rank'):
        call(c2, _thetas(3), 0.01, 1, c2.zeros(2, S2, 5, 8, 8), c2.zeros(S2, 8, 8), c2.zeros(S2, 8))


# ----------------------------------------------------------------------------------------------------- 12. Python surface
@pytest.mark.parametrize('name', ('os2015', 'channels'))
def test_solve_batch_of_the_parabolic_reduced_model(name):
    """One-component source (os2015) and the time-dependent source of the artificial-channels problem on 2 x 2 subdomains."""
    from pylrbms_amd import OS2015_academic_problem, artificial_channels_problem
    from pylrbms_amd.discretize_parabolic_block_swipdg import discretize
    from pylrbms_amd.reductor import ParabolicLRBMSReductor, ReducedVectorArray
    if name == 'os2015':
        p = OS2015_academic_problem.init_grid_and_problem({'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 4})
        T, nt, mu_values = 0.5, 4, ([0.2], [0.5], [0.9])
    else:
        p = artificial_channels_problem.init_grid_and_problem({'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 8})
        T, nt, mu_values = 1.0, 4, ([0.1], [0.5], [0.9])
    d, _ = discretize(p, T, nt)
    assert (d._src is not None) == (name == 'channels')
    mus = [d.parse_parameter(v) for v in mu_values]
    reductor = ParabolicLRBMSReductor(d)
    reductor.extend_basis(d.solve(mus[1])[[1, 2, nt]])
    rd = reductor.reduce()
    assert (rd.rhs_red_K is not None) == (name == 'channels')
    out = rd.solve_batch(mus)
    assert isinstance(out, list) and len(out) == len(mus)
    nbr = np.asarray(p['grid'].neighbor_slots)
    B, M = rd.B_sys.cpu().numpy(), rd.M_red.cpu().numpy()
    for U_m, mu in zip(out, mus):
        assert isinstance(U_m, ReducedVectorArray) and len(U_m) == nt + 1
        u1 = rd.solve(mu)
        if rd.rhs_red_K is not None:
            ref = dense_euler(B, M, nbr, d.theta(mu), T / nt, nt, rhs_K=rd.rhs_red_K.cpu().numpy(), phi=d.source_coefficients(mu))
        else:
            ref = dense_euler(B, M, nbr, d.theta(mu), T / nt, nt, rhs=rd.rhs_red.cpu().numpy())
        as_traj = lambda V: V.tensor.permute(2, 0, 1).cpu().numpy()[..., None]      # noqa: E731  [nt + 1, S, N, 1]
        e_single = float(column_errors(as_traj(u1), ref[..., None]).max())
        e_batch = float(column_errors(as_traj(U_m), ref[..., None]).max())
        print('PARABOLIC-BATCH solve_batch {} mu={}: e_single {:.2e}, e_batch {:.2e}'.format(name, mu, e_single, e_batch))
        assert e_batch <= 10.0 * max(e_single, 1e-13), (name, mu, e_single, e_batch)
    est, parts = rd.estimate(out[0], mus[0])
    assert np.isfinite(est) and est > 0.0
