"""lrbms_fom_implicit_euler_batch (batched full-order trajectories: implicit Euler, panels of 16 columns) against the NumPy
restatement tests/fom_euler_batch_ref.py (pinned to the oracle in tests/test_fom_euler_batch_host.py): the PCG of tests/pcg_ref.py
on the step operators M + dt A(theta_m) with the column's own inverse element blocks and ONE coarse level per call at the mean
theta, and a direct solve per step.

As in tests/test_fom_batch_gpu.py (whose cells are used here, with ``_model``, ``check_iterates``, ``check_mutant``, K_STEPS and the
tolerances of tests/test_pcg_iterates_gpu.py and TOL_TRAJ of tests/test_parabolic_batch_gpu.py) the raw export runs one step with
max_iter = k and must leave the k-th PCG iterate of every column behind: x_k - u_0 = U[1] - U[0] is the k-th iterate from zero on
the start residual, and the reported ratio is relative to the step's full right-hand side.  Three mutant references show that the
iterates can tell the preconditioners apart: the product run with LRBMS_OPT_COARSE 0 misses the two-level reference, and the
product misses a reference whose coarse level is built at theta_0 and one whose inverse element blocks lack the mass.

dt = 0.05 / nt, nt <= 3; work and U[1:] are NaN-poisoned before every raw call."""
import numpy as np
import pytest

import fom_euler_batch_ref
import test_pcg_iterates_gpu as cells
from test_fom_batch_gpu import OTHER_CELLS, PANEL_WIDTHS, SWEEP, _mus
from test_parabolic_batch_gpu import T_END, TOL_TRAJ
from test_pcg_iterates_gpu import K_STEPS, MUTANT_FLOOR, TOL_RES, TOL_X, check_iterates, check_mutant

pytestmark = pytest.mark.gpu

E_INVALID, E_NOT_CONVERGED = -1, -4


def _thetas(nmu):
    return np.stack([[1.0, mu] for mu in _mus(nmu)])


class Call:
    """One call of the raw export on a cell: device inputs, caller-owned (NaN-poisoned) work and U, and its reference."""

    def __init__(self, shape, kc, thetas, nt=1, K=1, coarse=1, phis=None, U0=None, seed=0, reference=True):
        m = cells._model(shape, 0, kc=kc)
        self.m, self.eng = m, m['eng']
        eng = self.eng
        self.ctx, self.S, self.t = eng.ctx, eng.S, eng.ctx.t
        self.thetas = np.ascontiguousarray(thetas, dtype=np.float64)
        self.nmu, self.Q = self.thetas.shape
        self.nt, self.dt = int(nt), T_END / nt
        rng = np.random.default_rng(seed)
        b = eng.b.cpu().numpy()
        if K == 1:
            self.b_K = eng.b.reshape(1, self.S, self.t.n).contiguous()
            phis = np.ones((self.nmu, nt + 1, 1)) if phis is None else phis
        else:
            self.b_K = cells._dev(self.ctx, rng.standard_normal((K, self.S, self.t.n)) * np.abs(b).max())
            phis = rng.uniform(0.2, 1.0, (self.nmu, nt + 1, K)) if phis is None else phis
        self.K = K
        self.phis_host = np.ascontiguousarray(phis, dtype=np.float64)
        self.phis = cells._dev(self.ctx, self.phis_host)
        self.U0_host = None if U0 is None else np.ascontiguousarray(U0, dtype=np.float64).reshape(self.S, self.t.n, self.nmu)
        self.U0 = None if U0 is None else cells._dev(self.ctx, self.U0_host)
        self.coarse = coarse
        self._parts = None
        self.ref = self.reference() if reference else None
        size = int(self.ctx.lib.lrbms_fom_implicit_euler_batch_work_size(self.ctx.handle, self.nmu))
        assert size > 0
        self.work = self.ctx.empty(size)

    def reference(self, **kw):
        eng = self.eng
        if self._parts is None:
            self._parts = (fom_euler_batch_ref.component_operators(eng.A_diag.cpu().numpy(), eng.A_cpl.cpu().numpy(), self.t, self.m['nbr']),
                           fom_euler_batch_ref.p1_mass(self.t.area, self.S))
        return fom_euler_batch_ref.BatchFomEulerRef(self._parts[0], self._parts[1], self.S, self.t.n, self.thetas, self.dt, self.nt,
                                                    self.phis_host, self.b_K.cpu().numpy(),
                                                    U0=None if self.U0_host is None else self.U0_host.reshape(-1, self.nmu),
                                                    coarse=self.coarse, **kw)

    def raw(self, k, rtol=1e-14, **over):
        """-> (rc, U tensor [nt + 1, S, n, nmu], info); ``over`` replaces single arguments (the refusal tests)."""
        from pylrbms_amd._native import _dblp, c_vp
        ctx, eng = self.ctx, self.eng
        self.work.fill_(float('nan'))
        U = ctx.empty(self.nt + 1, self.S, self.t.n, self.nmu)
        U.fill_(float('nan'))
        U[0] = 0.0 if self.U0 is None else self.U0
        info = np.zeros(2)
        a = dict(Q=self.Q, K=self.K, nmu=self.nmu, theta=_dblp(self.thetas), dt=float(self.dt), nt=self.nt, A_diag=c_vp(eng.A_diag.data_ptr()),
                 A_cpl=c_vp(eng.A_cpl.data_ptr()), b_K=c_vp(self.b_K.data_ptr()), phi=c_vp(self.phis.data_ptr()),
                 work=c_vp(self.work.data_ptr()), U=c_vp(U.data_ptr()), rtol=float(rtol), max_iter=int(k))
        a.update(over)
        rc = cells._raw(ctx, 'lrbms_fom_implicit_euler_batch', a['Q'], a['K'], a['nmu'], a['theta'], a['dt'], a['nt'], a['A_diag'], a['A_cpl'],
                        a['b_K'], a['phi'], a['work'], a['U'], a['rtol'], a['max_iter'], _dblp(info), ctx._stream())
        return rc, U, info

    def panels(self):
        from pylrbms_amd._native import _dblp
        out = np.zeros(8)
        assert self.ctx.lib.lrbms_fom_implicit_euler_batch_panel_info(self.ctx.handle, _dblp(out)) == 0
        return out

    def run(self, k, rtol=1e-14):
        """The ``run(k)`` of ``check_iterates`` (one step): (rc, U[1] - U[0] [S n, nmu], (iterations of a panel, worst ratio)).  The
        export reports the iterations summed over the panels; every panel must have run exactly k."""
        assert self.nt == 1
        rc, U, info = self.raw(k, rtol)
        pan, npan = self.panels(), (self.nmu + 15) // 16
        assert info[0] == pan[0:2 * npan:2].sum() and info[1] == pan[1::2].max(), (info, pan)
        assert all(v == pan[0] for v in pan[0:2 * npan:2]) and not pan[2 * npan:].any(), pan
        Uh = U.cpu().numpy().reshape(2, -1, self.nmu)
        return rc, Uh[1] - Uh[0], np.array([pan[0], info[1]])

    def trajectories(self, rtol, max_iter=100000):
        rc, U, info = self.raw(max_iter, rtol)
        assert rc == 0 and 0.0 <= info[1] <= rtol, (rc, info)
        return U.cpu().numpy().reshape(self.nt + 1, -1, self.nmu), info


def _miss(c, ref, tag, what):
    X_ref, _ = ref.iterate(2)
    _, X2, _ = c.run(2)
    err = float((np.linalg.norm(X2 - X_ref, axis=0) / np.linalg.norm(X_ref, axis=0)).max())
    print('FOM-EULER-BATCH {}: misses {} by {:.2e}'.format(tag, what, err))
    assert err > MUTANT_FLOOR, (tag, what, err)


def _cell(shape, kc, coarse, nmu, U0=None):
    ths = _thetas(nmu)
    tag = 'fom euler batch {} kc={} coarse={} nmu={}{}'.format(shape, kc, coarse, nmu, '' if U0 is None else ' U0')
    ctx = cells._model(shape, 0, kc=kc)['eng'].ctx
    ctx.set_option('coarse', coarse)
    try:
        c = Call(shape, kc, ths, coarse=coarse, U0=U0)
        assert c.ref.has_coarse == (coarse != 0 and c.S >= 4)
        check_iterates(c.run, c.ref.iterate, tag, tol_x=TOL_X, tol_res=TOL_RES, steps=K_STEPS)
        _miss(c, c.reference(mass_in_blocks=False), tag, 'inverse element blocks without the mass')
        if c.ref.has_coarse:
            if nmu > 1:           # (one column: theta_0 is the call mean)
                _miss(c, c.reference(coarse_theta=ths[0]), tag, 'a coarse level built at theta_0')
            ctx.set_option('coarse', 0)
            check_mutant(c.run, c.ref.iterate, tag)
    finally:
        ctx.set_option('coarse', 1)
    return c


# ----------------------------------------------------------------------------------------------------------- iterates
@pytest.mark.parametrize('nmu', PANEL_WIDTHS)
def test_iterates_over_the_panel_widths(nmu):
    _cell(SWEEP[0], SWEEP[1], 1, nmu)


def test_iterates_from_a_start_value_that_differs_per_column():
    """x_0 = u_0 != 0: the start residual is not the right-hand side, and the ratio is relative to the latter."""
    m = cells._model(SWEEP[0], 0, kc=SWEEP[1])
    eng = m['eng']
    nmu = 17
    x, _ = eng.ctx.fom_solve(np.array([1.0, 0.5]), eng.A_diag, eng.A_cpl, eng.b, rtol=1e-10)          # the scale of a solution
    rng = np.random.default_rng(11)
    U0 = np.abs(x.cpu().numpy()).max() * rng.uniform(0.1, 1.0, nmu) * rng.standard_normal((eng.S, eng.ctx.t.n, nmu))
    c = _cell(SWEEP[0], SWEEP[1], 1, nmu, U0=U0)
    _, r0 = c.ref.iterate(0)
    assert np.abs(r0 - 1.0).min() > 1e-3, r0                                 # (the two references differ in every column)


@pytest.mark.parametrize('shape, kc, coarse, nmu', OTHER_CELLS)
def test_iterates_over_the_cells(shape, kc, coarse, nmu):
    _cell(shape, kc, coarse, nmu)


# ------------------------------------------------------------------------------------------------------- trajectories
def test_trajectories_against_the_dense_reference_and_the_single_export():
    nmu, nt = 17, 3
    c = Call(SWEEP[0], SWEEP[1], _thetas(nmu), nt=nt)
    U, info = c.trajectories(1e-13)
    err = c.ref.column_errors(U)
    print('FOM-EULER-BATCH trajectories nmu={} nt={}: {} iterations, worst column error {:.2e} (tolerance {:.0e})'.format(
        nmu, nt, int(info[0]), float(err.max()), TOL_TRAJ))
    assert info[0] >= nt * 2 and np.isfinite(err).all() and err.max() < TOL_TRAJ, float(err.max())
    eng = c.eng
    e_batch = err.max(axis=0)
    ref = c.ref.trajectories()
    for m in sorted({0, nmu // 2, nmu - 1}):
        U1, _ = eng.ctx.fom_implicit_euler(c.thetas[m], c.dt, nt, eng.A_diag, eng.A_cpl, eng.b, rtol=1e-13)
        U1 = U1.cpu().numpy().reshape(nt + 1, -1)
        e_single = float((np.abs(U1[1:] - ref[1:, :, m]).max(axis=1) / np.abs(ref[1:, :, m]).max(axis=1)).max())
        print('FOM-EULER-BATCH accuracy column {}: e_single {:.2e}, e_batch {:.2e}'.format(m, e_single, float(e_batch[m])))
        assert e_batch[m] <= 10.0 * max(e_single, 1e-13), (m, e_single, float(e_batch[m]))


def test_true_residual_of_every_step_and_column():
    nmu, nt = 33, 3
    c = Call(SWEEP[0], SWEEP[1], _thetas(nmu), nt=nt)
    U, info = c.trajectories(1e-10)
    res = c.ref.true_residuals(U)
    print('FOM-EULER-BATCH true residuals nmu={} nt={}: worst {:.2e}, reported {:.2e}'.format(nmu, nt, float(res.max()), info[1]))
    assert np.isfinite(res).all() and res.max() <= 1e-9, float(res.max())


# ------------------------------------------------------------------------------------------------------------ sources
def test_time_dependent_sources_and_zero_columns():
    nmu, K, nt = 20, 3, 3
    phis = np.random.default_rng(7).uniform(0.2, 1.0, (nmu, nt + 1, K))
    phis[4] = 0.0                                                   # one zero column in each panel
    phis[17] = 0.0
    phis[9, 1] = 0.0                                                # nothing to do at step 1, a source from step 2 on
    c = Call(SWEEP[0], SWEEP[1], _thetas(nmu), nt=nt, K=K, phis=phis, seed=3)
    U, info = c.trajectories(1e-13)
    assert not U[:, :, 4].any() and not U[:, :, 17].any()           # exact zeros through all steps, and the call still converged
    assert not U[1, :, 9].any() and U[2, :, 9].any()
    err = c.ref.column_errors(U)
    print('FOM-EULER-BATCH K=3 with zero columns: {} iterations, worst column error {:.2e}'.format(int(info[0]), float(err.max())))
    assert err.max() < TOL_TRAJ, float(err.max())
    zero = Call(SWEEP[0], SWEEP[1], _thetas(3), nt=2, K=K, phis=np.zeros((3, 3, K)), reference=False)      # nothing to solve at all
    rc, U0, info0 = zero.raw(50)
    assert rc == 0 and not U0.cpu().numpy().any() and info0[0] == 0 and info0[1] == 0.0


# ----------------------------------------------------------------------------------------------------- column hygiene
def test_equal_columns_are_bitwise_equal_across_the_panel_boundary():
    nt = 2
    c = Call(SWEEP[0], SWEEP[1], np.tile([1.0, 0.37], (17, 1)), nt=nt, reference=False)
    rc, U, _ = c.raw(6)
    U = U.cpu().numpy().reshape(nt + 1, -1, 17)
    assert rc == E_NOT_CONVERGED and np.isfinite(U[1]).all() and U[1, :, 0].any() and np.isnan(U[2]).all()
    assert all(np.array_equal(U[1, :, 0], U[1, :, j]) for j in range(1, 17))
    Uc, _ = c.trajectories(1e-12)
    assert Uc[nt, :, 0].any() and all(np.array_equal(Uc[:, :, 0], Uc[:, :, j]) for j in range(1, 17))


def test_two_calls_give_the_same_bits_and_inputs_stay_unchanged():
    c = Call(SWEEP[0], SWEEP[1], _thetas(33), nt=2, K=3, seed=1, reference=False)
    eng = c.eng
    before = [t.clone() for t in (eng.A_diag, eng.A_cpl, c.b_K, c.phis)]
    (_, Ua, ia), (_, Ub, ib) = c.raw(6), c.raw(6)
    assert bool((Ua[:2] == Ub[:2]).all()) and np.array_equal(ia, ib)
    (Ua, ia), (Ub, ib) = c.trajectories(1e-12), c.trajectories(1e-12)
    assert np.isfinite(Ua).all() and np.array_equal(Ua, Ub) and np.array_equal(ia, ib)
    for was, now in zip(before, (eng.A_diag, eng.A_cpl, c.b_K, c.phis)):
        assert bool((was == now).all())


def test_panel_info_and_the_panels_after_a_missed_one():
    nmu, nt = 33, 2
    ths = _thetas(nmu)
    c = Call(SWEEP[0], SWEEP[1], ths, nt=nt, reference=False)
    eng = c.eng
    _, info = eng.ctx.fom_implicit_euler_batch(ths, c.dt, nt, eng.A_diag, eng.A_cpl, c.b_K, np.ones((nmu, nt + 1, 1)), rtol=1e-10)
    assert len(info['panel_iterations']) == 3 and min(info['panel_iterations']) >= nt
    assert sum(info['panel_iterations']) == info['iterations'] and 0.0 < info['relative_residual'] <= 1e-10
    rc, U, raw_info = c.raw(2)                                      # every panel misses its first step at max_iter
    pan = c.panels()
    assert rc == E_NOT_CONVERGED and list(pan[0::2]) == [2, 2, 2, 0] and raw_info[0] == 6
    assert pan[1:6:2].min() > 1e-14 and pan[1::2].max() == raw_info[1] and pan[7] == 0.0
    U = U.cpu().numpy()
    assert np.isfinite(U[1]).all() and all(U[1, :, :, m].any() for m in (0, 16, 32))     # the later panels still wrote their step
    assert np.isnan(U[2]).all()                                     # ... and no panel went past the step it missed


# ------------------------------------------------------------------------------------------------ buffers and refusals
def test_refusals_before_any_launch():
    from pylrbms_amd._native import _dblp, c_vp
    from pylrbms_amd import multiscale_problem
    from pylrbms_amd.engine import Engine
    from common import theta_bar_of
    ths = _thetas(3)
    c = Call(SWEEP[0], SWEEP[1], ths, nt=2, reference=False)
    assert c.raw(100000, rtol=1e-8)[0] == 0                          # the arguments below are otherwise fine
    wide = np.ones((65, 2))
    nan = float('nan')
    bad = [dict(nmu=0), dict(nmu=65, theta=_dblp(wide)), dict(K=0), dict(K=65), dict(Q=0), dict(Q=9), dict(nt=0), dict(nt=-1),
           dict(dt=0.0), dict(dt=-1.0), dict(dt=nan), dict(rtol=0.0), dict(rtol=-1.0), dict(rtol=nan), dict(max_iter=0)]
    bad += [{name: None} for name in ('theta', 'A_diag', 'A_cpl', 'b_K', 'phi', 'work', 'U')]
    for over in bad:
        rc, U, info = c.raw(10, **over)
        assert rc == E_INVALID, (over, rc)
        assert bool(U[1:].isnan().all()) and bool(c.work.isnan().all()), over      # nothing was launched
    assert c.ctx.lib.lrbms_fom_implicit_euler_batch_work_size(c.ctx.handle, 0) < 0
    assert c.ctx.lib.lrbms_fom_implicit_euler_batch_work_size(c.ctx.handle, 65) < 0
    assert c.raw(100000, rtol=1e-8)[0] == 0                          # the context goes on

    class TwoRanks:
        rank, size = 0, 2

    p = multiscale_problem.init_grid_and_problem({'num_subdomains': list(SWEEP[0]), 'coarse_per_subdomain': SWEEP[1]}, mpi_comm=TwoRanks())
    lam = p['lambda']
    sharded = Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar_of(p)).assemble()
    c2, S2, t = sharded.ctx, sharded.S, sharded.ctx.t
    assert sharded.S_ext > S2
    U = c2.empty(2, S2, t.n, 3)
    U.fill_(nan)
    U[0] = 0.0
    work = c2.empty(max(1, int(c2.lib.lrbms_fom_implicit_euler_batch_work_size(c2.handle, 3))))
    work.fill_(nan)
    info = np.zeros(2)
    rc = cells._raw(c2, 'lrbms_fom_implicit_euler_batch', 2, 1, 3, _dblp(ths), 0.05, 1, c_vp(sharded.A_diag.data_ptr()),
                    c_vp(sharded.A_cpl.data_ptr()), c_vp(sharded.b.data_ptr()), c_vp(c2.zeros(3, 2, 1).data_ptr()), c_vp(work.data_ptr()),
                    c_vp(U.data_ptr()), 1e-8, 10, _dblp(info), c2._stream())
    assert rc == E_INVALID and bool(U[1].isnan().all()) and bool(work.isnan().all())


# ------------------------------------------------------------------------------------------------------------- Python
def _discretization(name, nt=3):
    from pylrbms_amd import OS2015_academic_problem, artificial_channels_problem
    from pylrbms_amd.discretize_parabolic_block_swipdg import discretize
    if name == 'os2015':
        p = OS2015_academic_problem.init_grid_and_problem({'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 4})
        d, data = discretize(p, 0.5, nt)
    else:
        p = artificial_channels_problem.init_grid_and_problem({'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 8})
        d, data = discretize(p, 1.0, nt)
    assert (d._src is not None) == (name == 'channels')
    return d, data


@pytest.mark.parametrize('name, count', (('os2015', 70), ('channels', 7)))
def test_solve_batch_entries_are_the_single_trajectories(name, count):
    nt = 3
    d, _ = _discretization(name, nt)
    mus = [[float(v)] for v in np.linspace(0.1, 1.0, count)]       # 70 crosses the chunk of 64
    out = d.solve_batch(mus)
    assert isinstance(out, list) and len(out) == count
    its, rel = d.last_solve_info['iterations'], d.last_solve_info['relative_residual']
    assert its >= nt and 0.0 < rel <= 1e-10
    for m, mu in enumerate(mus):
        assert len(out[m]) == nt + 1 and tuple(out[m].tensor.shape) == (d.engine.S, d.engine.t.n, nt + 1)
        ref = d.solve(mu).tensor.cpu().numpy()
        assert np.abs(ref[..., nt]).max() > 0.0
        assert np.abs(out[m].tensor.cpu().numpy() - ref).max() <= 1e-8 * np.abs(ref).max(), (name, m)
    stationary = d.solve_stationary_batch if name == 'os2015' else None
    if stationary is not None:                                      # the elliptic batch is still there, under its own name
        X = stationary(mus[:3])
        ref = d.solve_stationary(mus[1]).tensor.cpu().numpy()[..., 0]
        assert len(X) == 3 and np.abs(X.tensor.cpu().numpy()[..., 1] - ref).max() <= 1e-8 * np.abs(ref).max()


def test_solve_batch_snapshots_feed_the_local_pod():
    from pylrbms_amd.reductor import ParabolicLRBMSReductor
    nt = 3
    d, data = _discretization('os2015', nt)
    reductor = ParabolicLRBMSReductor(d)
    before = list(reductor.local_sizes())
    mus = [[float(v)] for v in np.linspace(0.1, 1.0, 9)]
    snaps = d.solve_batch(mus, as_snapshots=True)
    assert len(snaps) == 9 * nt
    last = d.solve(mus[-1]).tensor.cpu().numpy()
    assert np.abs(snaps.tensor.cpu().numpy()[..., -nt:] - last[..., 1:]).max() <= 1e-8 * np.abs(last).max()      # parameter-major
    reductor.extend_basis(snaps, method='pod', pod_modes=3)
    after = list(reductor.local_sizes())
    assert all(a > b for a, b in zip(after, before)), (before, after)
