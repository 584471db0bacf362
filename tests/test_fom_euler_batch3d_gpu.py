"""lrbms3_fom_implicit_euler_batch (batched full-order trajectories in 3D: implicit Euler, panels of 16 columns on the fp64
matrix cores) against the NumPy restatement tests/fom_euler_batch3d_ref.py (pinned to the oracle in
tests/test_fom_euler_batch3d_host.py): the PCG of tests/pcg_ref.py on the step operators M + dt A(theta_m) with ONE preconditioner
per call, both levels on M + dt A(theta_bar) at the call mean, and a direct solve per step.

As in tests/test_fom_batch3d_gpu.py (whose engines and cells are used here, with ``check_iterates``, ``check_mutant``, K_STEPS,
TOL_X = 1e-10 and TOL_RES = 1e-8 of tests/test_pcg_iterates_gpu.py, unchanged) the raw export runs one step with max_iter = k and
must leave the k-th PCG iterate of every column behind: U[1] - U[0] is the k-th iterate from zero on the start residual, every
panel reports k iterations (``info[0]`` is their sum), and the reported ratio is relative to the step's full right-hand side.
The one-step cells start from a value per column (``fom_euler_batch3d_ref.start_values``), so the start residual is not the
right-hand side.  Three mutant references show that the iterates can tell the preconditioners apart: the product run with
LRBMS3_OPT_FOM_COARSE 0 misses the two-level reference, and the product misses a reference whose coarse level is built at theta_0
and one whose inverse element blocks lack the mass.  Every cell asserts from the reference alone that no k of K_STEPS is skipped.

Every raw call runs with work and U[1:] NaN-poisoned and with sentinel bands around U and work, checked after the call; slab 0
is compared with what went in.  DT = 0.05 (tests/test_pcg_iterates3d_gpu.py); trajectories have nt = 3.

The cell ``LOOP_CELL`` (7 x 7 x 6 subdomains, 294 workgroup rows) is the one size at which k3fb_scalars goes round more than once
over the partials of |M u_k + dt sum_j phi b_j|^2 that k3fb_step_residual leaves."""
import numpy as np
import pytest

import common3d as c3
import fom_batch3d_ref as ref3
import fom_euler_batch3d_ref as ref
import test_pcg_iterates_gpu as cells
from fom_euler_batch3d_ref import DT, SWEEP
from test_fom_batch3d_gpu import LOOP_CELL, PANEL_WIDTHS, _engine, _with_space
from test_pcg_iterates_gpu import K_STEPS, MIN_RATIO, MUTANT_FLOOR, TOL_RES, TOL_X, check_iterates, check_mutant

pytestmark = pytest.mark.gpu

E_INVALID, E_NOT_CONVERGED = -1, -4
NAN = float('nan')
GUARD, SENTINEL = 64, 12345.0             # doubles in front of and behind U and work (an even count keeps the 16-byte alignment)
EXPORT = 'lrbms3_fom_implicit_euler_batch'
OTHER_CELLS = (('q1_strip', 'p1', 17), ('interior_3x3x3', 'p1', 17), ('kc_3x1x2', 'p1', 17), ('aniso_2x2x1', 'p1', 17),
               ('interior_3x3x3', 'off', 17), ('interior_3x3x3', 'constants', 17))
TOL_TRAJ = 1e-8                           # against the dense stepping, of max |u|: the bound of ``_fom_converged``

_PARTS = {}


def _parts(name):
    """(components A_q, mass in the product's TM layout, b [S, n]) of a cell on the host, kept per name."""
    if name not in _PARTS:
        _, eng = _engine(name)
        Aq = ref3.component_operators(eng.ops['A_diag'].cpu().numpy(), eng.ops['A_cpl'].cpu().numpy(), eng.t, eng.nbr)
        mass = ref.mass_from_tables(eng.t.tables(eng.spec)['TM'], eng.t.elem_type, eng.S)
        _PARTS[name] = (Aq, mass, eng.ops['b'].cpu().numpy().copy())
    return _PARTS[name]


def _thetas(p, nmu):
    return np.stack([c3.theta_of(p, mu) for mu in ref.cell_mus(nmu)])


def _banded(ctx, count):
    """A buffer of ``count`` doubles between two sentinel bands -> (whole buffer, the view between the bands)."""
    buf = ctx.empty(count + 2 * GUARD)
    buf.fill_(SENTINEL)
    return buf, buf[GUARD:GUARD + count]


def _bands_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


class Call:
    """One call of the raw export on a problem: device inputs, caller-owned work and U (NaN-poisoned, between sentinel bands),
    and its reference.  ``U0``: None (zeros), 'start' (``ref.start_values``: a value per column) or an array [S n, nmu]."""

    def __init__(self, name, thetas, nt=1, K=1, space='p1', phis=None, U0=None, seed=0, reference=True):
        self.name = name
        self.p, self.eng = _engine(name)
        eng = self.eng
        self.ctx, self.S, self.t = eng.ctx, eng.S, eng.t
        self.thetas = np.ascontiguousarray(thetas, dtype=np.float64)
        self.nmu, self.Q = self.thetas.shape
        self.nt, self.dt = int(nt), DT
        rng = np.random.default_rng(seed)
        Aq, mass, b = _parts(name)
        if K == 1:
            self.b_K = eng.ops['b'].reshape(1, self.S, self.t.n).contiguous()
            phis = np.ones((self.nmu, nt + 1, 1)) if phis is None else phis
        else:
            self.b_K = cells._dev(self.ctx, rng.standard_normal((K, self.S, self.t.n)) * np.abs(b).max())
            phis = rng.uniform(0.2, 1.0, (self.nmu, nt + 1, K)) if phis is None else phis
        self.K = K
        self.phis_host = np.ascontiguousarray(phis, dtype=np.float64)
        assert self.phis_host.shape == (self.nmu, nt + 1, K)
        self.phis = cells._dev(self.ctx, self.phis_host)
        N = self.S * self.t.n
        if U0 is None:
            self.U0_host = np.zeros((N, self.nmu))
        elif isinstance(U0, str):
            self.U0_host = ref.start_values(Aq, self.thetas, b)
        else:
            self.U0_host = np.ascontiguousarray(U0, dtype=np.float64).reshape(N, self.nmu)
        self.U0 = cells._dev(self.ctx, self.U0_host.reshape(self.S, self.t.n, self.nmu))
        self.space = space
        self.Phi = {'p1': ref3.default_phi(self.t), 'constants': np.ones((self.t.n, 1)), 'off': None}[space]
        self.ref = self.reference() if reference else None
        size = int(self.ctx.lib.lrbms3_fom_implicit_euler_batch_work_size(self.ctx.handle, self.nmu))
        assert size > int(self.ctx.lib.lrbms3_fom_solve_batch_work_size(self.ctx.handle, self.nmu)) > 0
        self.work_buf, self.work = _banded(self.ctx, size)

    def reference(self, **kw):
        Aq, mass, _ = _parts(self.name)
        return ref.BatchFomEuler3DRef(Aq, mass, self.S, self.t.n, self.thetas, self.dt, self.nt, self.phis_host,
                                      self.b_K.cpu().numpy(), U0=self.U0_host, Phi=self.Phi, **kw)

    def raw(self, k, rtol=1e-14, **over):
        """-> (rc, U tensor [nt + 1, S, n, nmu], info); ``over`` replaces single arguments (the refusal tests).  Checks the sentinel
        bands around U and work and that slab 0 came back as it went in."""
        from pylrbms_amd._native import _dblp, c_vp
        ctx, ops = self.ctx, self.eng.ops
        self.work.fill_(NAN)
        shape = (self.nt + 1, self.S, self.t.n, self.nmu)
        U_buf, U = _banded(ctx, int(np.prod(shape)))
        U = U.view(shape)
        U.fill_(NAN)
        U[0] = self.U0
        info = np.zeros(2)
        a = dict(Q=self.Q, K=self.K, nmu=self.nmu, theta=_dblp(self.thetas), dt=float(self.dt), nt=self.nt,
                 A_diag=c_vp(ops['A_diag'].data_ptr()), A_cpl=c_vp(ops['A_cpl'].data_ptr()), b_K=c_vp(self.b_K.data_ptr()),
                 phi=c_vp(self.phis.data_ptr()), work=c_vp(self.work.data_ptr()), U=c_vp(U.data_ptr()), rtol=float(rtol),
                 max_iter=int(k))
        a.update(over)
        rc = cells._raw(ctx, EXPORT, a['Q'], a['K'], a['nmu'], a['theta'], a['dt'], a['nt'], a['A_diag'], a['A_cpl'], a['b_K'],
                        a['phi'], a['work'], a['U'], a['rtol'], a['max_iter'], _dblp(info), ctx._stream())
        assert _bands_intact(U_buf) and _bands_intact(self.work_buf), 'a write outside U or work'
        assert bool((U[0] == self.U0).all()), 'slab 0 was written'
        return rc, U, info

    def panels(self):
        from pylrbms_amd._native import _dblp
        out = np.zeros(8)
        assert self.ctx.lib.lrbms3_fom_implicit_euler_batch_panel_info(self.ctx.handle, _dblp(out)) == 0
        return out

    def run(self, k, rtol=1e-14):
        """The ``run(k)`` of ``check_iterates`` (one step): (rc, U[1] - U[0] [S n, nmu], (iterations of a panel, worst ratio)).  The
        export reports the iterations summed over the panels; every panel must have run exactly the same count."""
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


def _miss(c, other, tag, what):
    X_ref, _ = other.iterate(2)
    _, X2, _ = c.run(2)
    nrm = np.linalg.norm(X_ref, axis=0)
    err = float((np.linalg.norm(X2 - X_ref, axis=0) / nrm).max())
    print('FOM-EULER-BATCH-3D {}: misses {} by {:.2e}'.format(tag, what, err))
    assert err > MUTANT_FLOOR, (tag, what, err)


def _cell(name, space, nmu):
    p, eng = _engine(name)
    ctx = eng.ctx
    tag = 'fom euler batch 3D {} space={} nmu={}'.format(name, space, nmu)
    undo = _with_space(ctx, eng.t, space)
    try:
        c = Call(name, _thetas(p, nmu), space=space, U0='start')
        assert c.ref.has_coarse == (space != 'off')
        for k in K_STEPS:                                  # check_iterates must not skip a k: decided by the reference alone
            X, ratios = c.ref.iterate(k)
            assert ratios.min() >= MIN_RATIO, (tag, k, float(ratios.min()))
        lost = float((np.abs(c.U0_host).max(axis=0) / np.abs(c.ref.iterate(1)[0]).max(axis=0)).max())
        assert lost <= 10.0, (tag, lost)                   # U[1] - U[0] keeps the digits TOL_X reads (the host test pins 1.65 on its cells)
        cell, res = check_iterates(c.run, c.ref.iterate, tag, tol_x=TOL_X, tol_res=TOL_RES, steps=K_STEPS)
        _miss(c, c.reference(mass_in_blocks=False), tag, 'inverse element blocks without the mass')
        if c.ref.has_coarse:
            if nmu > 1:           # (one column: theta_0 is the call mean)
                _miss(c, c.reference(coarse_theta=c.thetas[0]), tag, 'a coarse level built at theta_0')
            ctx.set_option('fom_coarse', 0)
            check_mutant(c.run, c.ref.iterate, tag)
    finally:
        undo()
    return c


# ----------------------------------------------------------------------------------------------------------- iterates
@pytest.mark.parametrize('nmu', PANEL_WIDTHS)
def test_iterates_over_the_panel_widths(nmu):
    _cell(SWEEP, 'p1', nmu)


@pytest.mark.parametrize('name, space, nmu', OTHER_CELLS + (LOOP_CELL,))
def test_iterates_over_the_cells(name, space, nmu):
    c = _cell(name, space, nmu)
    _, first = c.ref.iterate(0)
    assert np.abs(first - 1.0).min() > 1e-3, first         # the start residual is not the right-hand side, in every column


def test_iterates_from_zero_with_the_plain_source():
    """U0 = 0, K = 1, phi = 1: the start residual is dt b, the ratio starts at 1."""
    p, _ = _engine(SWEEP)
    c = Call(SWEEP, _thetas(p, 17))
    assert np.array_equal(c.ref.iterate(0)[1], np.ones(17))
    check_iterates(c.run, c.ref.iterate, 'fom euler batch 3D from zero', tol_x=TOL_X, tol_res=TOL_RES, steps=K_STEPS)


# ------------------------------------------------------------------------------------------------------- trajectories
def _source_call(name, nmu, nt=3):
    """K = 2, a time-dependent phi with all-zero columns (column 2 also starts from zero), a start value per column otherwise."""
    p, _ = _engine(name)
    ths = _thetas(p, nmu)
    phis = np.random.default_rng(7).uniform(0.2, 1.0, (nmu, nt + 1, 2))
    phis[:, 2, 0] *= -1.0                                   # the first component changes sign inside the trajectory
    zero_cols = [2, 5] + ([20] if nmu > 20 else [])
    for m in zero_cols:
        phis[m] = 0.0
    Aq, _, b = _parts(name)
    U0 = ref.start_values(Aq, ths, b)
    U0[:, 2] = 0.0
    return Call(name, ths, nt=nt, K=2, phis=phis, U0=U0, seed=3), zero_cols


@pytest.mark.parametrize('name, nmu', (('aniso_2x2x1', 17), ('aniso_2x2x1', 33), (SWEEP, 17), (SWEEP, 33)))
def test_trajectories_against_the_dense_stepping(name, nmu):
    nt, rtol = 3, 1e-12
    c, zero_cols = _source_call(name, nmu, nt)
    U, info = c.trajectories(rtol)
    assert np.isfinite(U).all() and info[0] >= nt
    assert not U[:, :, 2].any()                             # zero source from zero: exactly 0 in every slab
    assert U[nt, :, 5].any() and np.abs(U[nt, :, 5]).max() < np.abs(U[0, :, 5]).max()      # zero source: the start value decays
    err = c.ref.column_errors(U)
    # true residuals: the reported ratio is the recurrence's; it parts from the true one by rounding, O(eps |A| |u| / |f|) per update
    res = c.ref.true_residuals(U)
    eps = np.finfo(np.float64).eps
    attain = max(np.linalg.norm(abs(c.ref.As[m]) @ np.abs(U[k + 1, :, m])) / max(np.linalg.norm(c.ref.rhs(m, k, U[k, :, m])), 1e-300)
                 for m in range(nmu) if m != 2 for k in range(nt))
    bound = 10.0 * rtol + 100.0 * eps * attain
    print('FOM-EULER-BATCH-3D trajectories {} nmu={} nt={}: {} iterations, worst column error {:.2e} (tolerance {:.0e}), worst true '
          'residual {:.2e} (bound {:.2e}), reported {:.2e}'.format(name, nmu, nt, int(info[0]), float(err.max()), TOL_TRAJ,
                                                                   float(res.max()), bound, info[1]))
    assert err.max() < TOL_TRAJ, float(err.max())
    assert res.max() <= bound, (float(res.max()), bound)
    if nmu == 17:                                           # one column against the single export with the same table
        eng, m = c.eng, 9
        U1, _ = eng.ctx.fom_implicit_euler_src(c.Q, c.thetas[m], c.dt, nt, eng.ops['A_diag'], eng.ops['A_cpl'], c.b_K, c.phis_host[m],
                                               U0=cells._dev(c.ctx, c.U0_host[:, m].reshape(c.S, c.t.n)), rtol=rtol)
        U1 = U1.cpu().numpy().reshape(nt + 1, -1)
        assert np.abs(U1 - U[:, :, m]).max() < TOL_TRAJ * np.abs(U1).max()


# ----------------------------------------------------------------------------------------------------- column hygiene
def test_equal_columns_are_bitwise_equal_across_the_panel_boundary():
    p, _ = _engine(SWEEP)
    nmu, nt = 33, 2
    c, _ = _source_call(SWEEP, nmu, nt)
    ths, phis, U0 = c.thetas.copy(), c.phis_host.copy(), c.U0_host.copy()
    ths[19], phis[19], U0[:, 19] = ths[3], phis[3], U0[:, 3]          # column 3 of panel 0 again as column 3 of panel 1
    c = Call(SWEEP, ths, nt=nt, K=2, phis=phis, U0=U0, seed=3, reference=False)
    rc, U, _ = c.raw(6)
    U = U.cpu().numpy().reshape(nt + 1, -1, nmu)
    assert rc == E_NOT_CONVERGED and np.isfinite(U[1]).all() and U[1, :, 3].any() and np.isnan(U[2]).all()
    assert np.array_equal(U[1, :, 3], U[1, :, 19]) and not np.array_equal(U[1, :, 3], U[1, :, 4])
    Uc, _ = c.trajectories(1e-12)
    assert Uc[nt, :, 3].any() and np.array_equal(Uc[:, :, 3], Uc[:, :, 19])


def test_two_calls_give_the_same_bits_and_inputs_stay_unchanged():
    c, _ = _source_call(SWEEP, 33, 2)
    c.ref = None
    ops = c.eng.ops
    watched = (ops['A_diag'], ops['A_cpl'], c.b_K, c.phis, c.U0)
    before = [t.clone() for t in watched]
    (_, Ua, ia), (_, Ub, ib) = c.raw(6), c.raw(6)
    assert bool((Ua[:2] == Ub[:2]).all()) and np.array_equal(ia, ib)
    (Ua, ia), (Ub, ib) = c.trajectories(1e-12), c.trajectories(1e-12)
    assert np.isfinite(Ua).all() and np.array_equal(Ua, Ub) and np.array_equal(ia, ib)
    for was, now in zip(before, watched):
        assert bool((was == now).all())


def test_panel_info_adds_up_to_info():
    p, eng = _engine(SWEEP)
    nmu, nt = 33, 2
    ths = _thetas(p, nmu)
    c = Call(SWEEP, ths, nt=nt, reference=False)
    U, info = eng.ctx.fom_implicit_euler_batch(ths, c.dt, nt, eng.ops['A_diag'], eng.ops['A_cpl'], c.b_K, np.ones((nmu, nt + 1, 1)), rtol=1e-10)
    assert tuple(U.shape) == (nt + 1, c.S, c.t.n, nmu)
    assert len(info['panel_iterations']) == 3 and min(info['panel_iterations']) >= nt
    assert sum(info['panel_iterations']) == info['iterations'] and 0.0 < info['relative_residual'] <= 1e-10
    rc, U, raw_info = c.raw(2)                                      # every panel misses its first step at max_iter
    pan = c.panels()
    assert rc == E_NOT_CONVERGED and list(pan[0::2]) == [2, 2, 2, 0] and raw_info[0] == 6
    assert pan[1:6:2].min() > 1e-14 and pan[1::2].max() == raw_info[1] and pan[7] == 0.0
    U = U.cpu().numpy()
    assert np.isfinite(U[1]).all() and all(U[1, :, :, m].any() for m in (0, 16, 32))     # the later panels still wrote their step
    assert np.isnan(U[2]).all()                                     # ... and no panel went past the step it missed


# -------------------------------------------------------------------------------------------------------- missed steps
def test_a_panel_that_misses_a_step_stops_and_the_others_run_on():
    p, _ = _engine(SWEEP)
    nmu, nt = 17, 2
    ths = _thetas(p, nmu)
    Aq, _, b = _parts(SWEEP)
    U0 = ref.start_values(Aq, ths, b)
    U0[:, 16] = 0.0
    phis = np.ones((nmu, nt + 1, 1))
    phis[16] = 0.0                                                  # panel 1 is this one column: nothing to solve, it converges at once
    c = Call(SWEEP, ths, nt=nt, phis=phis, U0=U0, reference=False)
    rc, U, info = c.raw(1)
    pan = c.panels()
    U = U.cpu().numpy().reshape(nt + 1, -1, nmu)
    assert rc == E_NOT_CONVERGED and list(pan[0::2]) == [1, 0, 0, 0] and info[0] == 1 and info[1] == pan[1] > 1e-14 and pan[3] == 0.0
    one = Call(SWEEP, ths, nt=1, phis=phis[:, :2], U0=U0)           # the reference of the first step
    X_ref, ratios = one.ref.iterate(1)
    d = U[1, :, :16] - U[0, :, :16]
    err = np.linalg.norm(d - X_ref[:, :16], axis=0) / np.linalg.norm(X_ref[:, :16], axis=0)
    assert err.max() < TOL_X, float(err.max())                      # slab 1 of panel 0 holds the first iterate u_0 + d_1
    assert abs(info[1] - ratios.max()) < TOL_RES * ratios.max()
    assert np.isnan(U[2, :, :16]).all()                             # ... and its slab 2 was never written
    assert not U[1, :, 16].any() and not U[2, :, 16].any()          # panel 1 ran to the end: exact zeros in both slabs


# ------------------------------------------------------------------------------------------------ buffers and refusals
def test_refusals_before_any_launch():
    from pylrbms_amd._native import _dblp, c_vp
    p, _ = _engine(SWEEP)
    ths = _thetas(p, 3)
    c = Call(SWEEP, ths, nt=2, reference=False)
    assert c.raw(100000, rtol=1e-8)[0] == 0                          # the arguments below are otherwise fine
    wide = np.ones((65, 3))
    bad = [dict(nmu=0), dict(nmu=65, theta=_dblp(wide)), dict(K=0), dict(K=65), dict(Q=0), dict(Q=9), dict(nt=0), dict(nt=-1),
           dict(dt=0.0), dict(dt=-1.0), dict(dt=NAN), dict(rtol=0.0), dict(rtol=-1.0), dict(rtol=NAN), dict(max_iter=0)]
    bad += [{name: None} for name in ('theta', 'A_diag', 'A_cpl', 'b_K', 'phi', 'work', 'U')]
    for over in bad:
        rc, U, info = c.raw(10, **over)
        assert rc == E_INVALID, (over, rc)
        assert bool(U[1:].isnan().all()) and bool(c.work.isnan().all()), over      # nothing was launched
    assert c.ctx.lib.lrbms3_fom_implicit_euler_batch_work_size(c.ctx.handle, 0) < 0
    assert c.ctx.lib.lrbms3_fom_implicit_euler_batch_work_size(c.ctx.handle, 65) < 0
    assert c.raw(100000, rtol=1e-8)[0] == 0                          # the context goes on


def test_a_sharded_engine_is_refused():
    from pylrbms_amd import multiscale_problem3d
    from pylrbms_amd._native import _dblp, c_vp
    from pylrbms_amd.engine3d import Engine3D
    p = multiscale_problem3d.init_grid_and_problem({'num_subdomains': (4, 2, 1), 'cubes_per_subdomain': 1}, rank=0, world_size=2)
    lam = p['lambda']
    sharded = Engine3D(p['grid'], lam['functions'], p['f'], p['lambda_bar'], p['lambda_hat']).assemble()
    c2, S2, t = sharded.ctx, sharded.S, sharded.t
    assert sharded.S_ext > S2
    ths = np.stack([[float(f(mu)) for f in lam['coefficients']] for mu in (0.2, 0.5, 0.9)])
    U = c2.empty(2, S2, t.n, 3)
    U.fill_(NAN)
    U[0] = 0.0
    work = c2.empty(max(1, int(c2.lib.lrbms3_fom_implicit_euler_batch_work_size(c2.handle, 3))))
    work.fill_(NAN)
    info = np.zeros(2)
    ops = sharded.ops
    rc = cells._raw(c2, EXPORT, ths.shape[1], 1, 3, _dblp(ths), DT, 1, c_vp(ops['A_diag'].data_ptr()), c_vp(ops['A_cpl'].data_ptr()),
                    c_vp(ops['b'].data_ptr()), c_vp(c2.zeros(3, 2, 1).data_ptr()), c_vp(work.data_ptr()), c_vp(U.data_ptr()), 1e-8, 10,
                    _dblp(info), c2._stream())
    assert rc == E_INVALID and bool(U[1].isnan().all()) and bool(work.isnan().all())


# ------------------------------------------------------------------------------------------------------------- Python
def _discretization(affine, nt=3, T=0.15):
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import discretize
    import affine_source3d_ref
    p = c3.make_problem('aniso_2x2x1')
    pd = affine_source3d_ref.problem_dict(p, coeffs=affine_source3d_ref.PARABOLIC if affine else None)
    if not affine:
        pd['f'] = p['f']
    d, _ = discretize(pd, T, nt)
    assert (d._src is not None) == affine
    return d


def _counted(ctx):
    native, calls = ctx.fom_implicit_euler_batch, []

    def counted(thetas, *args, **kw):
        calls.append(len(thetas))
        return native(thetas, *args, **kw)
    ctx.fom_implicit_euler_batch = counted
    return calls


@pytest.mark.parametrize('affine', (False, True))
def test_solve_batch_entries_are_the_single_trajectories(affine):
    nt = 6 if affine else 3
    d = _discretization(affine, nt, T=0.75 if affine else 0.15)     # (affine: the grid of tests/test_parabolic_source3d_gpu.py)
    ctx = d.engine.ctx
    mus = [float(v) for v in np.linspace(0.1, 1.0, 7 if affine else 70)]        # 70 crosses the chunk of 64
    calls = _counted(ctx)
    try:
        out, (its, rel) = d.solve_batch(mus, return_info=True)
    finally:
        del ctx.fom_implicit_euler_batch
    assert calls == ([7] if affine else [64, 6])
    assert isinstance(out, list) and len(out) == len(mus)
    assert d.last_solve_info == (its, rel) and its >= nt and 0.0 < rel <= 1e-10
    if affine:
        assert len(set(d.source_coefficients(mus[0])[1:, 0])) == 2
    for m, mu in enumerate(mus):
        assert tuple(out[m].shape) == (d.engine.S, d.engine.t.n, nt + 1)
        want = d.solve(mu).cpu().numpy()
        assert np.abs(want[..., nt]).max() > 0.0
        assert np.abs(out[m].cpu().numpy() - want).max() <= 1e-9 * np.abs(want).max(), (affine, m)
    assert not out[3].is_contiguous()                               # a view of the panel goes where a trajectory goes
    est, _ = d.estimate(out[3], mus[3])
    est1, _ = d.estimate(out[3].contiguous(), mus[3])
    assert np.isfinite(est) and est > 0.0 and abs(est - est1) <= 1e-12 * est1
    if not affine:                                                  # the elliptic batch is still there, under its own name
        X = d.solve_stationary_batch(mus[:3])
        want = d.solve_stationary(mus[1]).cpu().numpy()
        assert tuple(X.shape) == (d.engine.S, d.engine.t.n, 3)
        assert np.abs(X.cpu().numpy()[..., 1] - want).max() <= 1e-8 * np.abs(want).max()
    else:
        with pytest.raises(NotImplementedError):
            d.solve_stationary_batch(mus[:3])


def test_solve_batch_snapshots_feed_the_local_pod():
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D
    nt = 3
    d = _discretization(False, nt)
    reductor = ParabolicLRBMSReductor3D(d)
    before = list(reductor.local_sizes())
    mus = [float(v) for v in np.linspace(0.1, 1.0, 9)]
    snaps = d.solve_batch(mus, as_snapshots=True)
    assert tuple(snaps.shape) == (d.engine.S, d.engine.t.n, 9 * nt) and snaps.is_contiguous()
    last = d.solve(mus[-1]).cpu().numpy()
    assert np.abs(snaps.cpu().numpy()[..., -nt:] - last[..., 1:]).max() <= 1e-9 * np.abs(last).max()      # parameter-major
    reductor.extend_basis(snaps, method='pod', pod_modes=3)
    after = list(reductor.local_sizes())
    assert all(a > b for a, b in zip(after, before)), (before, after)
    with pytest.raises(ValueError):
        d.solve_batch([0.5] * 43, as_snapshots=True)                # 43 x 3 > 128 vectors
