"""lrbms3_fom_solve_batch (batched full-order snapshots in 3D, panels of 16 columns on the fp64 matrix cores) against the NumPy
PCG of tests/pcg_ref.py with the preconditioner restated in tests/fom_batch3d_ref.py: ONE preconditioner per call, the inverse
10 x 10 element blocks and the P1-per-subdomain coarse level both built at the mean theta of the call.

As in tests/test_fom_batch_gpu.py (whose ``check_iterates``, ``check_mutant``, K_STEPS and tolerances come from
tests/test_pcg_iterates_gpu.py) the raw export runs with max_iter = k, work and X NaN-poisoned before every call, and must
leave the k-th PCG iterate of every column behind; a converged call is closed against a direct solve per column.  Every cell
asserts from the reference alone that no k of K_STEPS is skipped.  Three mutant references show that the iterates can tell the
preconditioners apart: the product run with LRBMS3_OPT_FOM_COARSE 0 misses the two-level reference, and the product misses a
reference whose coarse level is built at theta_0 and one whose element blocks are the column's own.

Tolerances: TOL_X = 1e-10 and TOL_RES = 1e-8, the figures of the 2D solvers, unchanged.

Cells: the panel widths on ``q3_2x1x2`` (Q = 3); with 17 columns ``q1_strip`` (Q = 1, S = 3), ``interior_3x3x3`` (a subdomain with
six neighbours; n_T = 6: the second round of every element loop is half filled), ``kc_3x1x2`` (n_T = 36: two workgroups per
subdomain, the second half filled, sides with unequal face counts), ``aniso_2x2x1`` (n_T = 48), and ``interior_3x3x3`` again
without a coarse level and with the constants-only space.

Looping kernels: k3fb_matvec and k3fb_update walk the elements of a workgroup four at a time (more than one round from n_T = 5
on: every cell); k3fb_coarse_r0 loops over the workgroups of a subdomain (two in ``kc_3x1x2`` and ``aniso_2x2x1``);
k3fb_coarse_apply walks a row of the coarse inverse 16 entries per round (more than one round from 33 coarse unknowns on:
``interior_3x3x3`` has 108); k3fb_scalars sums 256 partial rows per round, and only the cell ``LOOP_CELL`` -- 7 x 7 x 6
subdomains of one cube: 294 workgroup rows and 1 176 coarse rows -- makes both of its loops go round more than once."""
import numpy as np
import pytest

import common3d as c3
import fom_batch3d_ref as ref3
import test_pcg_iterates_gpu as cells
from test_pcg_iterates_gpu import K_STEPS, MIN_RATIO, MUTANT_FLOOR, TOL_RES, TOL_X, check_iterates, check_mutant

pytestmark = pytest.mark.gpu

E_INVALID, E_NOT_CONVERGED = -1, -4
SWEEP = 'q3_2x1x2'
PANEL_WIDTHS = (1, 5, 16, 17, 33, 64)
# (problem, coarse space: 'p1' (the default of mesh upload) | 'constants' | 'off' (LRBMS3_OPT_FOM_COARSE 0), nmu)
OTHER_CELLS = (('q1_strip', 'p1', 17), ('interior_3x3x3', 'p1', 17), ('kc_3x1x2', 'p1', 17), ('aniso_2x2x1', 'p1', 17),
               ('interior_3x3x3', 'off', 17), ('interior_3x3x3', 'constants', 17))
LOOP_CELL = ('loop_7x7x6', 'p1', 2)
LOOP_SPEC = ([7, 7, 6], 1, [c3._one, c3._lam1], [lambda mu: 1.0, lambda mu: mu], np.eye(3), 4, 0.5)

_ENGINES = {}


def _mus(nmu):
    return np.linspace(0.1, 1.0, nmu) if nmu > 1 else np.array([0.1])


def _engine(name):
    if name not in _ENGINES:
        p = c3.make_problem(name, spec=LOOP_SPEC if name == LOOP_CELL[0] else None)
        _ENGINES[name] = (p, c3.engine_of(p).assemble())
    return _ENGINES[name]


def _thetas(p, nmu):
    return np.stack([c3.theta_of(p, mu) for mu in _mus(nmu)])


class Call:
    """One call of the raw export on a problem: device inputs, caller-owned (NaN-poisoned) work and X, and its reference."""

    def __init__(self, name, thetas, K=1, space='p1', phi=None, seed=0, reference=True):
        self.p, self.eng = _engine(name)
        eng = self.eng
        self.ctx, self.S, self.t = eng.ctx, eng.S, eng.t
        self.thetas = np.ascontiguousarray(thetas, dtype=np.float64)
        self.nmu, self.Q = self.thetas.shape
        rng = np.random.default_rng(seed)
        b = eng.ops['b'].cpu().numpy()
        if K == 1:
            self.b_K = eng.ops['b'].reshape(1, self.S, self.t.n).contiguous()
            phi = np.ones((self.nmu, 1)) if phi is None else phi
        else:
            self.b_K = cells._dev(self.ctx, rng.standard_normal((K, self.S, self.t.n)) * np.abs(b).max())
            phi = rng.uniform(0.2, 1.0, (self.nmu, K)) if phi is None else phi
        self.K = K
        self.phi_host = np.ascontiguousarray(phi, dtype=np.float64)
        self.phi = cells._dev(self.ctx, self.phi_host)
        self.space = space
        self.Phi = {'p1': ref3.default_phi(self.t), 'constants': np.ones((self.t.n, 1)), 'off': None}[space]
        self.ref = self.reference() if reference else None
        size = int(self.ctx.lib.lrbms3_fom_solve_batch_work_size(self.ctx.handle, self.nmu))
        assert size > 0
        self.work = self.ctx.empty(size)

    def reference(self, **kw):
        eng = self.eng
        ref = ref3.BatchFom3DRef(eng.ops['A_diag'].cpu().numpy(), eng.ops['A_cpl'].cpu().numpy(), self.t, eng.nbr, self.thetas,
                                 self.phi_host, self.b_K.cpu().numpy(), Phi=self.Phi, Aq=getattr(self, '_Aq', None), **kw)
        self._Aq = ref.Aq
        return ref

    def raw(self, k, rtol=1e-14, **over):
        """-> (rc, X tensor [S, n, nmu], info); ``over`` replaces single arguments (the refusal tests)."""
        from pylrbms_amd._native import _dblp, c_vp
        ctx, ops = self.ctx, self.eng.ops
        self.work.fill_(float('nan'))
        X = ctx.empty(self.S, self.t.n, self.nmu)
        X.fill_(float('nan'))
        info = np.zeros(2)
        a = dict(Q=self.Q, nmu=self.nmu, theta=_dblp(self.thetas), A_diag=c_vp(ops['A_diag'].data_ptr()), A_cpl=c_vp(ops['A_cpl'].data_ptr()),
                 K=self.K, phi=c_vp(self.phi.data_ptr()), b_K=c_vp(self.b_K.data_ptr()), work=c_vp(self.work.data_ptr()),
                 X=c_vp(X.data_ptr()), rtol=float(rtol), max_iter=int(k))
        a.update(over)
        rc = cells._raw(ctx, 'lrbms3_fom_solve_batch', a['Q'], a['nmu'], a['theta'], a['A_diag'], a['A_cpl'], a['K'], a['phi'], a['b_K'],
                        a['work'], a['X'], a['rtol'], a['max_iter'], _dblp(info), ctx._stream())
        return rc, X, info

    def run(self, k, rtol=1e-14):
        rc, X, info = self.raw(k, rtol)
        return rc, X.cpu().numpy().reshape(-1, self.nmu), info

    def converged(self, rtol=1e-12):
        rc, X, info = self.run(100000, rtol=rtol)
        assert rc == 0 and info[1] <= rtol, (rc, info)
        return X, info


def _with_space(ctx, t, space):
    """Install the coarse space of a cell; returns the undo."""
    if space == 'constants':
        ctx.fom_coarse_space(np.ones((t.n, 1)))
    if space == 'off':
        ctx.set_option('fom_coarse', 0)

    def undo():
        ctx.set_option('fom_coarse', 1)
        ctx.fom_coarse_space(ref3.default_phi(t))
    return undo


def _miss(X, X_ref):
    return float((np.linalg.norm(X - X_ref, axis=0) / np.linalg.norm(X_ref, axis=0)).max())


def _cell(name, space, nmu):
    p, eng = _engine(name)
    ctx = eng.ctx
    tag = 'fom batch 3D {} space={} nmu={}'.format(name, space, nmu)
    undo = _with_space(ctx, eng.t, space)
    try:
        c = Call(name, _thetas(p, nmu), space=space)
        assert c.ref.has_coarse == (space != 'off')
        for k in K_STEPS:                                  # check_iterates must not skip a k: decided by the reference alone
            _, ratios = c.ref.iterate(k)
            assert ratios.min() >= MIN_RATIO, (tag, k, float(ratios.min()))
        check_iterates(c.run, c.ref.iterate, tag, tol_x=TOL_X, tol_res=TOL_RES, steps=K_STEPS)
        X, _ = c.converged()
        for j in range(nmu):
            ref = c.ref.solve(j)
            assert np.abs(X[:, j] - ref).max() < 1e-8 * np.abs(ref).max(), (tag, j)
        if nmu > 1:               # (one column: theta_0 and the column's own theta are the call mean)
            _, X2, _ = c.run(2)
            X_ref, _ = c.reference(block_theta='own').iterate(2)
            err = _miss(X2, X_ref)
            print('FOM-BATCH-3D {}: misses element blocks inverted at the column\'s own theta by {:.2e}'.format(tag, err))
            assert err > MUTANT_FLOOR, (tag, err)
            if c.ref.has_coarse:
                X_ref, _ = c.reference(coarse_theta=c.thetas[0]).iterate(2)
                err = _miss(X2, X_ref)
                print('FOM-BATCH-3D {}: misses a coarse level built at theta_0 by {:.2e}'.format(tag, err))
                assert err > MUTANT_FLOOR, (tag, err)
                ctx.set_option('fom_coarse', 0)
                check_mutant(c.run, c.ref.iterate, tag)
    finally:
        undo()


# ----------------------------------------------------------------------------------------------------------- iterates
@pytest.mark.parametrize('nmu', PANEL_WIDTHS)
def test_iterates_over_the_panel_widths(nmu):
    _cell(SWEEP, 'p1', nmu)


@pytest.mark.parametrize('name, space, nmu', OTHER_CELLS + (LOOP_CELL,))
def test_iterates_over_the_cells(name, space, nmu):
    _cell(name, space, nmu)


# ------------------------------------------------------------------------------------------------------------ sources
def test_affine_sources_and_zero_columns():
    nmu, K = 20, 3
    p, _ = _engine(SWEEP)
    phi = np.random.default_rng(7).uniform(0.2, 1.0, (nmu, K))
    phi[4] = 0.0                                                    # one zero right-hand side in each panel
    phi[17] = 0.0
    c = Call(SWEEP, _thetas(p, nmu), K=K, phi=phi, seed=3)
    assert not c.ref.cols[:, 4].any() and not c.ref.cols[:, 17].any() and c.ref.cols[:, 5].any()
    check_iterates(c.run, c.ref.iterate, 'fom batch 3D K=3 with zero columns')
    X, info = c.converged()
    assert not X[:, 4].any() and not X[:, 17].any()                 # exact zeros, and the call still converged
    for j in (0, 5, 16, 19):
        ref = c.ref.solve(j)
        assert np.abs(X[:, j] - ref).max() < 1e-8 * np.abs(ref).max(), j
    zero = Call(SWEEP, _thetas(p, 3), K=K, phi=np.zeros((3, K)), reference=False)     # nothing to solve at all
    rc, X0, info0 = zero.run(50)
    assert rc == 0 and not X0.any() and info0[0] == 0 and info0[1] == 0.0


# ----------------------------------------------------------------------------------------------------- column hygiene
def test_equal_columns_are_bitwise_equal_across_the_panel_boundary():
    p, _ = _engine(SWEEP)
    c = Call(SWEEP, np.tile(c3.theta_of(p, 0.37), (17, 1)), reference=False)
    _, X, _ = c.run(6)
    assert np.isfinite(X).all() and X[:, 0].any()
    assert all(np.array_equal(X[:, 0], X[:, j]) for j in range(1, 17))
    Xc, _ = c.converged()
    assert all(np.array_equal(Xc[:, 0], Xc[:, j]) for j in range(1, 17))


def test_one_column_is_the_single_solve():
    p, eng = _engine('kc_3x1x2')
    th = c3.theta_of(p, 0.37)
    c = Call('kc_3x1x2', th[None], reference=False)
    X, _ = c.converged(rtol=1e-13)
    x1, _ = eng.ctx.fom_solve(eng.Q, th, eng.ops['A_diag'], eng.ops['A_cpl'], eng.ops['b'], rtol=1e-13)
    x1 = x1.cpu().numpy().ravel()
    assert np.linalg.norm(X[:, 0] - x1) < 1e-9 * np.linalg.norm(x1)


def test_two_calls_give_the_same_bits():
    p, _ = _engine(SWEEP)
    c = Call(SWEEP, _thetas(p, 33), reference=False)
    (_, Xa, ia), (_, Xb, ib) = c.run(6), c.run(6)
    assert np.array_equal(Xa, Xb) and np.array_equal(ia, ib)
    (Xa, ia), (Xb, ib) = c.converged(), c.converged()
    assert np.array_equal(Xa, Xb) and np.array_equal(ia, ib)


def test_panel_info_reports_every_panel_of_the_last_call():
    from pylrbms_amd._native import _dblp
    p, eng = _engine(SWEEP)
    ths = _thetas(p, 33)
    c = Call(SWEEP, ths, reference=False)
    _, info = eng.ctx.fom_solve_batch(ths, eng.ops['A_diag'], eng.ops['A_cpl'], np.ones((33, 1)), c.b_K, rtol=1e-10)
    assert len(info['panel_iterations']) == 3 and min(info['panel_iterations']) >= 1
    assert max(info['panel_iterations']) == info['iterations'] and 0.0 < info['relative_residual'] <= 1e-10
    rc, _, raw_info = c.run(2)                                      # every panel is capped at max_iter
    panels = np.zeros(8)
    assert c.ctx.lib.lrbms3_fom_solve_batch_panel_info(c.ctx.handle, _dblp(panels)) == 0
    assert rc == E_NOT_CONVERGED and list(panels[0::2]) == [2, 2, 2, 0] and panels[1::2].max() == raw_info[1] and panels[7] == 0.0


# ------------------------------------------------------------------------------------------------ buffers and refusals
def test_inputs_stay_unchanged_under_poisoned_buffers():
    p, eng = _engine(SWEEP)
    c = Call(SWEEP, _thetas(p, 17), K=3, seed=1, reference=False)
    watched = (eng.ops['A_diag'], eng.ops['A_cpl'], c.b_K, c.phi)
    before = [t.clone() for t in watched]
    X, _ = c.converged()                                            # (work and X are NaN-poisoned by every raw call)
    assert np.isfinite(X).all()
    for was, now in zip(before, watched):
        assert bool((was == now).all())


def test_refusals_before_any_launch():
    from pylrbms_amd._native import _dblp, c_vp
    p, _ = _engine(SWEEP)
    ths = _thetas(p, 3)
    c = Call(SWEEP, ths, reference=False)
    assert c.raw(100000, rtol=1e-8)[0] == 0                          # the arguments below are otherwise fine
    wide = np.ones((65, 3))
    bad = [dict(nmu=0), dict(nmu=65, theta=_dblp(wide)), dict(K=0), dict(K=65), dict(Q=0), dict(Q=9), dict(rtol=0.0), dict(rtol=-1.0),
           dict(rtol=float('nan')), dict(max_iter=0)]
    bad += [{name: None} for name in ('theta', 'A_diag', 'A_cpl', 'phi', 'b_K', 'work', 'X')]
    for over in bad:
        rc, X, info = c.raw(10, **over)
        assert rc == E_INVALID, (over, rc)
        assert bool(X.isnan().all()) and bool(c.work.isnan().all()), over      # nothing was launched
    assert c.ctx.lib.lrbms3_fom_solve_batch_work_size(c.ctx.handle, 0) < 0
    assert c.ctx.lib.lrbms3_fom_solve_batch_work_size(c.ctx.handle, 65) < 0
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
    X = c2.empty(S2, t.n, 3)
    X.fill_(float('nan'))
    work = c2.empty(max(1, int(c2.lib.lrbms3_fom_solve_batch_work_size(c2.handle, 3))))
    work.fill_(float('nan'))
    info = np.zeros(2)
    ops = sharded.ops
    rc = cells._raw(c2, 'lrbms3_fom_solve_batch', ths.shape[1], 3, _dblp(ths), c_vp(ops['A_diag'].data_ptr()), c_vp(ops['A_cpl'].data_ptr()), 1,
                    c_vp(c2.zeros(3, 1).data_ptr()), c_vp(ops['b'].data_ptr()), c_vp(work.data_ptr()), c_vp(X.data_ptr()), 1e-8, 10,
                    _dblp(info), c2._stream())
    assert rc == E_INVALID and bool(X.isnan().all()) and bool(work.isnan().all())


# ------------------------------------------------------------------------------------------------------------- Python
def _discretization(affine):
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import discretize
    import affine_source3d_ref
    p = c3.make_problem('aniso_2x2x1')
    pd = affine_source3d_ref.problem_dict(p)
    if not affine:
        pd['f'] = p['f']
    d, _ = discretize(pd)
    assert (d._src is not None) == affine
    return d


@pytest.mark.parametrize('affine', (False, True))
def test_solve_batch_columns_are_the_single_solves(affine):
    d = _discretization(affine)
    ctx = d.engine.ctx
    mus = [float(v) for v in np.linspace(0.1, 1.0, 70 if not affine else 7)]        # 70 crosses the chunk of 64
    native, calls = ctx.fom_solve_batch, []

    def counted(thetas, *args, **kw):
        calls.append(len(thetas))
        return native(thetas, *args, **kw)
    ctx.fom_solve_batch = counted
    try:
        U, (its, rel) = d.solve_batch(mus, return_info=True)
    finally:
        del ctx.fom_solve_batch
    assert calls == ([64, 6] if not affine else [7])
    assert tuple(U.shape) == (d.engine.S, d.engine.t.n, len(mus))
    assert its >= 1 and 0.0 < rel <= 1e-10
    X = U.cpu().numpy()
    for m, mu in enumerate(mus):
        ref = d.solve(mu).cpu().numpy()
        assert np.abs(X[..., m] - ref).max() <= 1e-9 * np.abs(ref).max(), (affine, m)


@pytest.mark.parametrize('affine', (False, True))
def test_solve_batch_feeds_the_local_pod(affine):
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    d = _discretization(affine)
    reductor = LRBMSReductor3D(d)
    before = list(reductor.local_sizes())
    mu = 0.55
    ref = d.solve(mu, rtol=1e-12).cpu().numpy()
    err_before = np.linalg.norm(reductor.reconstruct(reductor.reduce().solve(mu, rtol=1e-13)).cpu().numpy() - ref)
    mus = [float(v) for v in np.linspace(0.1, 1.0, 9)]
    reductor.extend_basis(d.solve_batch(mus), method='pod', pod_modes=3)
    after = list(reductor.local_sizes())
    assert all(a > b for a, b in zip(after, before)), (before, after)
    rd = reductor.reduce()
    U = reductor.reconstruct(rd.solve(mu, rtol=1e-13)).cpu().numpy()
    assert np.isfinite(U).all() and np.linalg.norm(U - ref) < err_before        # the enlarged space contains the old one
