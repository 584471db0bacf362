"""Batched reduced trajectories of the 3D / P2 path on the GPU: lrbms3_reduced_implicit_euler_batch(_src) -- nmu <= 64 parameters
of the parabolic reduced model, every time step one panel PCG per group of 16 columns -- against the dense reference
tests/parabolic_batch3d_ref.py (pinned to tests/parabolic3d_ref.py in tests/test_parabolic_batch3d_host.py), the single-parameter
export, a NumPy PCG with the restated two-level preconditioner, and through ``InstationaryReducedDiscretization3D.solve_batch``.

Shapes: ``interior_3x3x3`` of tests/common3d.py (27 subdomains, one with all seven slots, k_c = 1, n = 60) with the leading N of 32
basis columns of ``make_bases3d``; nt = 3, dt = 0.05 unless stated."""
import ctypes

import numpy as np
import pytest

import common3d as c3
import pcg_ref
from parabolic_batch3d_ref import (StepPrecond3D, column_errors, dense_euler_batch, mass_operator, pcg_dense, step_operator,
                                   true_residuals)

pytestmark = pytest.mark.gpu

NMAX = 32
DT = 0.05
NT = 3
TOL_TRAJ = 1e-9           # per (step, column): the bound of test_reduced_implicit_euler_and_time_residual_match_dense_numpy
E_INVALID, E_NOT_CONVERGED = -1, -4
DISPATCH_CELLS = tuple((N, 17) for N in (5, 16, 17, 31, 32)) + tuple((17, nmu) for nmu in (1, 5, 16, 64))

_SYS = {}
_REF = {}


def _system(name='interior_3x3x3', N=NMAX, ragged=None):
    """Engine, neighbour table and the reduced system (B_sys, rhs_red, M_red as host arrays) of ``name`` at N basis columns.
    ragged = 'pad': subdomain 1 has N - 2 vectors, zero-padded; 'first': the first basis vector of subdomain 2 is zero."""
    key = (name, N, ragged)
    if key not in _SYS:
        from pylrbms_amd.engine3d import Engine3D
        p = c3.make_problem(name)
        base = _SYS.get((name, None))
        if base is None:
            base = Engine3D(p['grid'], p['lambdas'], p['f'], p['lambda_bar'], p['lambda_hat'],
                            theta_bar=c3.theta_of(p, p['mu_bar'])).assemble()
            _SYS[(name, None)] = base
        eng = base
        V = c3.make_bases3d(eng.S, eng.ctx.n, N, seed=3)
        keep = np.ones((eng.S, N))
        if ragged == 'pad':
            V[1, :, N - 2:] = 0.0
            keep[1, N - 2:] = 0.0
        elif ragged == 'first':
            V[2, :, 0] = 0.0
            keep[2, 0] = 0.0
        Vd = eng.ctx.from_numpy(V)
        out = eng.project_and_estimate(Vd)
        M = eng.ctx.project_mass(Vd)
        _SYS[key] = dict(p=p, eng=eng, nbr=np.asarray(eng.nbr).reshape(eng.S, 7), Q=len(p['lambdas']), keep=keep,
                         B=out['B_sys'].cpu().numpy().copy(), rhs=out['rhs_red'].cpu().numpy().copy(), M=M.cpu().numpy().copy())
    return _SYS[key]


def _cut(s, N):
    return (np.ascontiguousarray(s['B'][..., :N, :N]), np.ascontiguousarray(s['M'][:, :N, :N]), np.ascontiguousarray(s['rhs'][:, :N]))


def _thetas(s, nmu):
    return np.ascontiguousarray(np.stack([c3.theta_of(s['p'], mu) for mu in np.linspace(0.15, 1.2, nmu)]))


def _dev(ctx, a):
    return ctx.from_numpy(np.ascontiguousarray(a))


def _reference(N, nmu, nt=NT):
    """The dense trajectories of a plain cell on interior_3x3x3, computed once per (N, nmu, nt) and left unchanged."""
    key = (N, nmu, nt)
    if key not in _REF:
        s = _system()
        B, M, rhs = _cut(s, N)
        _REF[key] = dense_euler_batch(B, M, s['nbr'], _thetas(s, nmu), DT, nt, rhs=rhs)
        _REF[key].setflags(write=False)
    return _REF[key]


def _run(N, nmu, nt=NT, rtol=1e-13, s=None, **kw):
    s = _system() if s is None else s
    ctx = s['eng'].ctx
    B, M, rhs = _cut(s, N)
    U, info = ctx.reduced_implicit_euler_batch(s['Q'], _thetas(s, nmu), DT, nt, _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs), rtol=rtol,
                                               **kw)
    assert tuple(U.shape) == (nt + 1, s['eng'].S, N, nmu)
    return U, info


def _dense_check(N, nmu, tag):
    U, (it, res) = _run(N, nmu)
    err = column_errors(U.cpu().numpy(), _reference(N, nmu))
    print('PARABOLIC-BATCH3D {} N={} nmu={}: {} iterations, worst column error {:.2e} (tolerance {:.0e})'.format(
        tag, N, nmu, it, float(err.max()), TOL_TRAJ))
    assert res <= 1e-13 and it >= NT
    assert np.isfinite(err).all() and err.max() < TOL_TRAJ, (tag, N, nmu, float(err.max()))


# ------------------------------------------------------------------------------------------------------- dispatch coverage
@pytest.mark.parametrize('N, nmu', DISPATCH_CELLS)
def test_trajectories_over_the_panel_dispatch(N, nmu):
    """Both row-tile counts of the matrix-core matvec, odd and even N, clamped tiles; a partial group, a second group of one
    column, four groups."""
    _dense_check(N, nmu, 'dispatch')


@pytest.mark.parametrize('name, nmu', (('q3_2x1x2', 5), ('wide_basis', 17)))
def test_trajectories_on_other_problems(name, nmu):
    """Q = 3 (q3_2x1x2, N = 6) and S = 2 with N = 30 (wide_basis)."""
    s = _system(name, c3.PROBLEMS[name][5])
    N = c3.PROBLEMS[name][5]
    U, (it, res) = _run(N, nmu, s=s)
    B, M, rhs = _cut(s, N)
    ref = dense_euler_batch(B, M, s['nbr'], _thetas(s, nmu), DT, NT, rhs=rhs)
    err = column_errors(U.cpu().numpy(), ref)
    print('PARABOLIC-BATCH3D {} N={} nmu={}: {} iterations, worst column error {:.2e}'.format(name, N, nmu, it, float(err.max())))
    assert res <= 1e-13 and np.isfinite(err).all() and err.max() < TOL_TRAJ, (name, float(err.max()))


# ------------------------------------------------------------------------------------- as accurate as the single export
@pytest.mark.parametrize('N, nmu', ((17, 17), (32, 64)))
def test_batch_columns_are_as_accurate_as_the_single_parameter_export(N, nmu):
    """e_batch <= 10 max(e_single, 1e-13) per column against the same dense reference: the two use different preconditioners
    and stop at different iterates of the same tolerance."""
    s = _system()
    ctx = s['eng'].ctx
    B, M, rhs = _cut(s, N)
    Bd, Md, rd = _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs)
    thetas, ref = _thetas(s, nmu), _reference(N, nmu)
    U, _ = _run(N, nmu)
    e_batch = column_errors(U.cpu().numpy(), ref).max(axis=0)
    for m in sorted({0, nmu // 2, nmu - 1}):
        U1, _ = ctx.reduced_implicit_euler(s['Q'], thetas[m], DT, NT, Bd, Md, rd, rtol=1e-13)
        e_single = float(column_errors(U1.cpu().numpy()[..., None], ref[..., m:m + 1]).max())
        print('PARABOLIC-BATCH3D accuracy N={} nmu={} column {}: e_single {:.2e}, e_batch {:.2e}'.format(N, nmu, m, e_single,
                                                                                                         float(e_batch[m])))
        assert e_batch[m] <= 10.0 * max(e_single, 1e-13), (N, nmu, m, e_single, float(e_batch[m]))


# ------------------------------------------------------------------------------------------------------------ true residuals
def test_true_residuals_of_every_column_and_step():
    """rtol = 1e-10: the recomputed residual of every step and column is no worse than 10 x the worst true residual of the single
    export on the same inputs (floor: rtol) -- no column was disturbed after it converged, none was left behind."""
    N, nmu, rtol = 17, 33, 1e-10
    s = _system()
    ctx = s['eng'].ctx
    B, M, rhs = _cut(s, N)
    thetas = _thetas(s, nmu)
    U, (it, res) = _run(N, nmu, rtol=rtol)
    assert res <= rtol
    r_batch = true_residuals(U.cpu().numpy(), B, M, s['nbr'], thetas, DT, rhs=rhs)
    Bd, Md, rd = _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs)
    worst_single = 0.0
    for m in (0, nmu // 2, nmu - 1):
        U1, _ = ctx.reduced_implicit_euler(s['Q'], thetas[m], DT, NT, Bd, Md, rd, rtol=rtol)
        worst_single = max(worst_single, float(true_residuals(U1.cpu().numpy()[..., None], B, M, s['nbr'], thetas[m:m + 1], DT,
                                                              rhs=rhs).max()))
    print('PARABOLIC-BATCH3D true residuals N={} nmu={}: batch worst {:.2e}, best {:.2e}; single worst {:.2e}'.format(
        N, nmu, float(r_batch.max()), float(r_batch.min()), worst_single))
    assert np.isfinite(r_batch).all() and r_batch.max() <= 10.0 * max(worst_single, rtol), (float(r_batch.max()), worst_single)


# --------------------------------------------------------------------------------------------- iterates pin the preconditioner
def _raw(ctx, name, *args):
    """One raw export call with caller-owned buffers -> its return code (no exception on LRBMS_E_NOT_CONVERGED)."""
    rc = getattr(ctx.lib, name)(ctx.handle, *args)
    ctx.torch.cuda.synchronize(ctx.device)
    return rc


def _dblp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _first_step_iterates(N, nmu, U0=None):
    """One step (nt = 1) of the raw export with max_iter = k against the NumPy PCG; -> the tolerance used.

    x_k = U[1] - U[0] is the k-th PCG iterate for the right-hand side f - (M + dt A_m) u_0, f = M u_0 + dt b; the export's ratio
    refers to |f|.  The tolerance: the reference recurrences run on the CPU in float64 and in longdouble on the same operator
    and preconditioner (right-hand side formed in the respective precision), 100 x their largest relative difference over the
    columns at k = 5, floor 1e-12."""
    s = _system()
    ctx, S, nbr, Q = s['eng'].ctx, s['eng'].S, s['nbr'], s['Q']
    B, M, rhs = _cut(s, N)
    thetas = _thetas(s, nmu)
    As = [step_operator(B, M, nbr, th, DT) for th in thetas]
    P = StepPrecond3D(B, M, nbr, thetas.mean(axis=0), DT)
    PJ = StepPrecond3D(B, M, nbr, thetas.mean(axis=0), DT, coarse=False)
    assert P.has_coarse and not PJ.has_coarse
    Mop = mass_operator(M)
    u0 = np.zeros((S * N, nmu)) if U0 is None else U0.reshape(S * N, nmu)
    f = Mop @ u0 + DT * rhs.reshape(-1, 1)
    cols = np.stack([f[:, j] - As[j] @ u0[:, j] for j in range(nmu)], axis=1)
    scale = np.linalg.norm(cols, axis=0) / np.linalg.norm(f, axis=0)
    # tolerance: float64 against longdouble recurrences at k = 5
    Minv = P.matrix()
    ld = np.longdouble
    diff = 0.0
    for j in sorted({0, nmu // 2, nmu - 1}):
        Ad = As[j].toarray()
        b_ld = (Mop.toarray().astype(ld) @ u0[:, j].astype(ld) + ld(DT) * rhs.reshape(-1).astype(ld)) - Ad.astype(ld) @ u0[:, j].astype(ld)
        x64, _ = pcg_dense(Ad, Minv, cols[:, j], 5)
        xld, _ = pcg_dense(Ad, Minv, b_ld, 5, dtype=ld)
        diff = max(diff, float(np.linalg.norm(x64 - xld) / np.linalg.norm(xld)))
    tol = max(100.0 * diff, 1e-12)

    def reference(k, prec):
        out = [pcg_ref.pcg_iterate(lambda p, A=A: A @ p, prec.apply, cols[:, j], k) for j, A in enumerate(As)]
        return np.stack([x for x, _ in out], axis=1), np.array([r for _, r in out]) * scale

    Bd, Md, rd = _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs)
    work = ctx.empty(int(ctx.lib.lrbms3_reduced_implicit_euler_batch_work_size(ctx.handle, N, nmu)))
    worst = 0.0
    for k in (1, 2, 5):
        X_ref, ratios = reference(k, P)
        X_jac, _ = reference(k, PJ)
        nrm = np.linalg.norm(X_ref, axis=0)
        miss = float((np.linalg.norm(X_jac - X_ref, axis=0) / nrm).max())
        assert miss > 100.0 * tol, ('block-Jacobi alone is too close to the two-level reference', k, miss, tol)
        U = ctx.zeros(2, S, N, nmu)
        if U0 is not None:
            U[0] = _dev(ctx, U0)
        info = (ctypes.c_double * 2)()
        rc = _raw(ctx, 'lrbms3_reduced_implicit_euler_batch', Q, N, nmu, _dblp(thetas), DT, 1, _vp(Bd), _vp(Md), _vp(rd), _vp(work),
                  _vp(U), 1e-14, k, info, ctx._stream())
        assert rc == E_NOT_CONVERGED and int(info[0]) == k, (k, rc, info[0])
        Uh = U.cpu().numpy().reshape(2, S * N, nmu)
        err = np.linalg.norm((Uh[1] - Uh[0]) - X_ref, axis=0) / nrm
        print('PARABOLIC-BATCH3D iterates N={} nmu={} k={}: worst x_k error {:.2e} (tolerance {:.2e}), ratio {:.6e} (reference {:.6e}), '
              'block-Jacobi alone misses by {:.2e}'.format(N, nmu, k, float(err.max()), tol, info[1], float(ratios.max()), miss))
        assert np.isfinite(err).all() and err.max() < tol, (k, float(err.max()), tol)
        worst = max(worst, float(err.max()))
    return tol, worst


def test_first_step_iterates_against_numpy_pcg():
    """Zero initial data, max_iter = k for k in {1, 2, 5}: LRBMS_E_NOT_CONVERGED with x_k in U[1], equal to the NumPy PCG with the
    restated two-level preconditioner at the call-mean theta.  On the CPU the reference with block-Jacobi alone misses the
    two-level one by more than 100 x the tolerance, so a missing coarse level would be noticed.
    Tolerance (100 x float64-vs-longdouble at k = 5, floor 1e-12) at N = 17, nmu = 17: 1.00e-12, the floor -- the two
    precisions differ by 3.3e-16 ... 5.4e-16 at k = 5.  Measured on the MI355X: worst x_k error 1.2e-15 (k = 2); block-Jacobi
    alone misses the two-level reference by 3.5e-1 / 1.1e-1 / 7.6e-3 at k = 1 / 2 / 5."""
    _first_step_iterates(17, 17)


def test_first_step_iterates_from_random_initial_data():
    """The same from random U[0] of the size of a solution (N = 16, nmu = 5); the right-hand side f - (M + dt A) u_0 is formed in
    the respective precision, so the tolerance carries its cancellation.  Tolerance: 1.00e-12, the floor (the two precisions
    differ by 6.1e-16 ... 7.2e-16 at k = 5); measured on the MI355X: worst x_k error 1.4e-15 (k = 5)."""
    N, nmu = 16, 5
    s = _system()
    u_scale = np.abs(_reference(N, nmu, nt=1)).max()
    U0 = np.ascontiguousarray(np.random.default_rng(11).standard_normal((s['eng'].S, N, nmu)) * u_scale)
    _first_step_iterates(N, nmu, U0=U0)


# ------------------------------------------------------------------------------------------------------------------- VALU form
def test_trajectories_valu_form():
    ctx = _system()['eng'].ctx
    ctx.set_option('solve_valu', 1)
    try:
        _dense_check(17, 17, 'VALU')
    finally:
        ctx.set_option('solve_valu', 0)


# ------------------------------------------------------------------------------------------------------------------------ _src
def test_source_export_with_one_unit_component_is_the_plain_export():
    import torch
    N, nmu = 17, 17
    s = _system()
    ctx = s['eng'].ctx
    B, M, rhs = _cut(s, N)
    U, info = _run(N, nmu)
    U1, info1 = ctx.reduced_implicit_euler_batch_src(s['Q'], _thetas(s, nmu), DT, NT, _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs[None]),
                                                     np.ones((nmu, NT + 1, 1)), rtol=1e-13)
    assert torch.equal(U, U1) and info == info1       # the start kernel keeps the operation order: the same bits


def test_source_export_with_a_switching_coefficient_and_a_zero_column():
    """K = 2 with a coefficient that switches sign per column and per step, against dense stepping; a column whose phi rows are
    all zero comes back as exact zeros."""
    N, nmu, K = 17, 20, 2
    s = _system()
    ctx, S = s['eng'].ctx, s['eng'].S
    B, M, rhs = _cut(s, N)
    rng = np.random.default_rng(4)
    rhs_K = np.ascontiguousarray(np.stack([rhs, rng.standard_normal((S, N)) * np.abs(rhs).max()]))
    phis = np.empty((nmu, NT + 1, K))
    for m in range(nmu):
        phis[m, :, 0] = [1.0 if (k + m) % 2 else -1.0 for k in range(NT + 1)]       # +-1, switching every step, shifted per column
        phis[m, :, 1] = -1.0 + 0.02 * m
    phis[7] = 0.0
    thetas = _thetas(s, nmu)
    U, (it, res) = ctx.reduced_implicit_euler_batch_src(s['Q'], thetas, DT, NT, _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs_K), phis,
                                                        rtol=1e-13)
    Uh = U.cpu().numpy()
    assert np.all(Uh[..., 7] == 0.0)
    ref = dense_euler_batch(B, M, s['nbr'], thetas, DT, NT, rhs_K=rhs_K, phis=phis)
    others = [m for m in range(nmu) if m != 7]
    err = column_errors(Uh[..., others], ref[..., others])
    print('PARABOLIC-BATCH3D src K=2: {} iterations, worst column error {:.2e}'.format(it, float(err.max())))
    assert res <= 1e-13 and err.max() < TOL_TRAJ, float(err.max())


# ---------------------------------------------------------------------------------------------------------------- ragged bases
@pytest.mark.parametrize('ragged', ('pad', 'first'))
def test_ragged_bases(ragged):
    """Zero-padded basis columns stay exactly 0 in every step and column; with a first basis vector zeroed in one subdomain the
    coarse matrix is not positive definite and the call still converges (block-Jacobi alone)."""
    N, nmu = 6, 20
    s = _system(N=N, ragged=ragged)
    B, M, rhs = _cut(s, N)
    keep, thetas = s['keep'], _thetas(s, nmu)
    assert StepPrecond3D(B, M, s['nbr'], thetas.mean(axis=0), DT).has_coarse == (ragged == 'pad')
    U, (it, res) = _run(N, nmu, s=s)
    Uh = U.cpu().numpy()
    assert res <= 1e-13 and np.all(Uh[:, keep == 0, :] == 0.0)
    ref = dense_euler_batch(B, M, s['nbr'], thetas, DT, NT, rhs=rhs, keep=keep)
    err = column_errors(Uh, ref)
    print('PARABOLIC-BATCH3D ragged {}: {} iterations, worst column error {:.2e}'.format(ragged, it, float(err.max())))
    assert err.max() < TOL_TRAJ, float(err.max())


# ------------------------------------------------------------------------------------------------------------- work and state
@pytest.mark.parametrize('N, nmu, valu', ((17, 17, 0), (16, 40, 1)))
def test_result_does_not_depend_on_the_work_buffer_and_repeats(N, nmu, valu):
    import torch
    from test_work_poison_gpu import poisoned
    ctx = _system()['eng'].ctx
    ctx.set_option('solve_valu', valu)
    try:
        U, info = poisoned(ctx, lambda: _run(N, nmu, nt=2))
        U2, info2 = _run(N, nmu, nt=2)
        assert torch.equal(U, U2) and info == info2
    finally:
        ctx.set_option('solve_valu', 0)


def test_installed_preconditioner_and_the_next_stationary_batch_are_untouched():
    """A preconditioner installed with reduced_precond_use belongs to A: the call neither reads nor replaces it, and the next
    stationary reduced_solve_batch gives the bits it gave before the call."""
    import torch
    N, nmu = 17, 17
    s = _system()
    ctx, Q = s['eng'].ctx, s['Q']
    B, M, rhs = _cut(s, N)
    Bd, rd = _dev(ctx, B), _dev(ctx, rhs)
    thetas = _thetas(s, nmu)
    pc = ctx.reduced_precond_build(Q, c3.theta_of(s['p'], 0.6), Bd)
    pc0 = pc.clone()
    U_free, info_free = _run(N, nmu)
    ctx.reduced_precond_use(pc)
    try:
        u0, i0 = ctx.reduced_solve_batch(Q, thetas, Bd, rd, rtol=1e-12)
        U, info = _run(N, nmu)
        u1, i1 = ctx.reduced_solve_batch(Q, thetas, Bd, rd, rtol=1e-12)
    finally:
        ctx.reduced_precond_use(None)
    assert torch.equal(pc, pc0)
    assert torch.equal(U, U_free) and info == info_free
    assert torch.equal(u0, u1) and i0 == i1


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_before_any_launch_and_max_iter_misses():
    s = _system()
    ctx, S, Q = s['eng'].ctx, s['eng'].S, s['Q']
    N, nmu, nt = 8, 3, 2
    B, M, rhs = _cut(s, N)
    Bd, Md, rd, rKd = _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs), _dev(ctx, rhs[None])
    thetas = _thetas(s, 65)
    phid = _dev(ctx, np.ones((65, nt + 1, 1)))
    work = ctx.empty(int(ctx.lib.lrbms3_reduced_implicit_euler_batch_work_size(ctx.handle, 33, 64)))
    U = ctx.zeros(nt + 1, S, 33, 65)
    poison = float(np.pi)
    U[1:] = poison
    info = (ctypes.c_double * 2)()
    null = ctypes.c_void_p(None)

    def plain(N_=N, nmu_=nmu, dt=DT, nt_=nt, Bp=None, Up=None, th=_dblp(thetas)):
        return _raw(ctx, 'lrbms3_reduced_implicit_euler_batch', Q, N_, nmu_, th, dt, nt_, _vp(Bd) if Bp is None else Bp, _vp(Md), _vp(rd),
                    _vp(work), _vp(U) if Up is None else Up, 1e-12, 1000, info, ctx._stream())

    def src(K):
        return _raw(ctx, 'lrbms3_reduced_implicit_euler_batch_src', Q, N, K, nmu, _dblp(thetas), DT, nt, _vp(Bd), _vp(Md), _vp(rKd),
                    _vp(phid), _vp(work), _vp(U), 1e-12, 1000, info, ctx._stream())

    for rc in (plain(N_=33), plain(nmu_=0), plain(nmu_=65), plain(dt=0.0), plain(dt=-0.1), plain(nt_=0), plain(Bp=null), plain(Up=null),
               plain(th=ctypes.POINTER(ctypes.c_double)()), src(0), src(65)):
        assert rc == E_INVALID, rc
    assert bool((U[1:] == poison).all())                 # nothing was launched
    assert ctx.lib.lrbms3_reduced_implicit_euler_batch_work_size(ctx.handle, N, 0) == -1
    assert plain() == 0 and src(1) == 0                  # the arguments above are otherwise fine
    # max_iter caps ONE step: the miss in step 0 leaves the iterate in U[1]; later slabs are untouched
    Um = ctx.zeros(nt + 1, S, N, nmu)
    Um[2:] = poison
    rc = _raw(ctx, 'lrbms3_reduced_implicit_euler_batch', Q, N, nmu, _dblp(thetas), DT, nt, _vp(Bd), _vp(Md), _vp(rd), _vp(work), _vp(Um),
              1e-12, 3, info, ctx._stream())
    assert rc == E_NOT_CONVERGED and int(info[0]) == 3 and info[1] > 1e-12
    assert bool((Um[2:] == poison).all()) and float(Um[1].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------- Python surface
def _pd(p):
    return {'grid': p['grid'], 'lambda': {'functions': p['lambdas'], 'coefficients': p['thetas']}, 'lambda_bar': p['lambda_bar'],
            'lambda_hat': p['lambda_hat'], 'f': p['f'], 'mu_bar': p['mu_bar'], 'mu_hat': p['mu_hat']}


@pytest.mark.parametrize('source', (False, True))
def test_solve_batch_of_the_parabolic_reduced_model(source):
    """``rd.solve_batch(mus)`` -> [len(mus), nt + 1, S, N]; entry m equals ``rd.solve(mus[m])`` to 1e-10; 70 parameters are two
    native calls.  With and without a time-dependent affine source (as tests/test_parabolic_source3d_gpu.py builds it)."""
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D, discretize
    p = c3.make_problem('aniso_2x2x1')
    T, nt = 0.75, 3
    if source:
        from affine_source3d_ref import PARABOLIC, problem_dict
        d, _ = discretize(problem_dict(p, coeffs=PARABOLIC), T, nt)
    else:
        d, _ = discretize(_pd(p), T, nt)
    assert (d._src is not None) == source
    reductor = ParabolicLRBMSReductor3D(d)
    reductor.extend_basis(d.solve(p['mu'])[:, :, [1, 2, nt]])
    rd = reductor.reduce()
    assert (rd.rhs_red_K is not None) == source
    S, N = d.engine.S, reductor.basis_size()
    mus = [0.2, p['mu'], 0.9]
    out, (it, res) = rd.solve_batch(mus, return_info=True)
    assert tuple(out.shape) == (len(mus), nt + 1, S, N) and it >= nt and res <= 1e-12
    singles = {}
    for m, mu in enumerate(mus):
        singles[mu] = rd.solve(mu)
        assert tuple(singles[mu].shape) == (nt + 1, S, N)
        assert float(singles[mu].abs().max()) > 0.0
        err = c3.rel(out[m].cpu().numpy(), singles[mu].cpu().numpy())
        print('PARABOLIC-BATCH3D solve_batch source={} mu={}: {:.2e}'.format(source, mu, err))
        assert err < 1e-10, (mu, err)
    many = list(np.linspace(0.2, 0.9, 70))
    out70 = rd.solve_batch(many)
    assert tuple(out70.shape) == (70, nt + 1, S, N)
    assert c3.rel(out70[0].cpu().numpy(), singles[0.2].cpu().numpy()) < 1e-10
    assert c3.rel(out70[69].cpu().numpy(), singles[0.9].cpu().numpy()) < 1e-10
    assert c3.rel(out70[65].cpu().numpy(), rd.solve(many[65]).cpu().numpy()) < 1e-10
    est, parts = rd.estimate(out[0], mus[0])
    assert np.isfinite(est) and est > 0.0
