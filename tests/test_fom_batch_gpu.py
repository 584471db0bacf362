"""lrbms_fom_solve_batch (batched full-order snapshots, panels of 16 columns) against the NumPy PCG of tests/pcg_ref.py with
the preconditioner restated in tests/fom_batch_ref.py: the column's own inverse element blocks plus ONE coarse level per call,
built at the mean theta of the call.

As in tests/test_pcg_iterates_gpu.py (whose ``_model``, ``check_iterates``, ``check_mutant``, K_STEPS and tolerances are used
here) the raw export runs with max_iter = k and must leave the k-th PCG iterate of every column behind; a converged call is
closed against a direct solve per column.  Two mutant references show that the iterates can tell the preconditioners apart:
the product run with LRBMS_OPT_COARSE 0 misses the two-level reference, and the product misses a reference whose coarse level
is built at theta_0 instead of the call mean.

Cells: the smallest full-order cells of the iterate tests (no coarse level at S < 4; n_T = 32 with and without the coarse level;
n_T = 128; n_T = 512), and one cell of 6 x 6 subdomains with n_T = 512 (18 432 elements): the only one where the workgroups
of both panel kernels (at most 256, 16 resp. 64 elements per pass) loop over the elements, the update kernel with a partly
filled last round."""
import numpy as np
import pytest

import fom_batch_ref
import test_pcg_iterates_gpu as cells
from test_pcg_iterates_gpu import K_STEPS, MUTANT_FLOOR, TOL_RES, TOL_X, check_iterates, check_mutant

pytestmark = pytest.mark.gpu

E_INVALID, E_NOT_CONVERGED = -1, -4
SWEEP = ((4, 3), 2)                                          # grid, k_c
PANEL_WIDTHS = (1, 5, 16, 17, 33, 64)
OTHER_CELLS = (((3, 1), 2, 1, 17), ((4, 3), 2, 0, 17), ((4, 3), 4, 1, 17), ((2, 2), 8, 1, 17), ((6, 6), 8, 1, 3))


def _mus(nmu):
    return np.linspace(0.1, 1.0, nmu) if nmu > 1 else np.array([0.1])


class Call:
    """One call of the raw export on a cell: device inputs, caller-owned (NaN-poisoned) work and X, and its reference."""

    def __init__(self, shape, kc, thetas, K=1, coarse=1, phi=None, seed=0, reference=True):
        m = cells._model(shape, 0, kc=kc)
        self.m, self.eng = m, m['eng']
        eng = self.eng
        self.ctx, self.S, self.t = eng.ctx, eng.S, eng.ctx.t
        self.thetas = np.ascontiguousarray(thetas, dtype=np.float64)
        self.nmu, self.Q = self.thetas.shape
        rng = np.random.default_rng(seed)
        b = eng.b.cpu().numpy()
        if K == 1:
            self.b_K = eng.b.reshape(1, self.S, self.t.n).contiguous()
            phi = np.ones((self.nmu, 1)) if phi is None else phi
        else:
            self.b_K = cells._dev(self.ctx, rng.standard_normal((K, self.S, self.t.n)) * np.abs(b).max())
            phi = rng.uniform(0.2, 1.0, (self.nmu, K)) if phi is None else phi
        self.K = K
        self.phi_host = np.ascontiguousarray(phi, dtype=np.float64)
        self.phi = cells._dev(self.ctx, self.phi_host)
        self.coarse = coarse
        self.ref = None
        if reference:
            self.ref = self.reference()
        size = int(self.ctx.lib.lrbms_fom_solve_batch_work_size(self.ctx.handle, self.nmu))
        assert size > 0
        self.work = self.ctx.empty(size)

    def reference(self, coarse_theta=None):
        eng = self.eng
        return fom_batch_ref.BatchFomRef(eng.A_diag.cpu().numpy(), eng.A_cpl.cpu().numpy(), self.t, self.m['nbr'], self.thetas,
                                         self.phi_host, self.b_K.cpu().numpy(), self.coarse, coarse_theta)

    def raw(self, k, rtol=1e-14, **over):
        """-> (rc, X tensor [S, n, nmu], info); ``over`` replaces single arguments (the refusal tests)."""
        from pylrbms_amd._native import _dblp, c_vp
        ctx, eng = self.ctx, self.eng
        self.work.fill_(float('nan'))
        X = ctx.empty(self.S, self.t.n, self.nmu)
        X.fill_(float('nan'))
        info = np.zeros(2)
        a = dict(Q=self.Q, nmu=self.nmu, theta=_dblp(self.thetas), A_diag=c_vp(eng.A_diag.data_ptr()), A_cpl=c_vp(eng.A_cpl.data_ptr()),
                 K=self.K, phi=c_vp(self.phi.data_ptr()), b_K=c_vp(self.b_K.data_ptr()), work=c_vp(self.work.data_ptr()),
                 X=c_vp(X.data_ptr()), rtol=float(rtol), max_iter=int(k))
        a.update(over)
        rc = cells._raw(ctx, 'lrbms_fom_solve_batch', a['Q'], a['nmu'], a['theta'], a['A_diag'], a['A_cpl'], a['K'], a['phi'], a['b_K'],
                        a['work'], a['X'], a['rtol'], a['max_iter'], _dblp(info), ctx._stream())
        return rc, X, info

    def run(self, k, rtol=1e-14):
        rc, X, info = self.raw(k, rtol)
        return rc, X.cpu().numpy().reshape(-1, self.nmu), info

    def converged(self, rtol=1e-12):
        rc, X, info = self.run(100000, rtol=rtol)
        assert rc == 0 and info[1] <= rtol, (rc, info)
        return X, info


def _cell(shape, kc, coarse, nmu):
    ths = np.stack([[1.0, mu] for mu in _mus(nmu)])
    tag = 'fom batch {} kc={} coarse={} nmu={}'.format(shape, kc, coarse, nmu)
    ctx = cells._model(shape, 0, kc=kc)['eng'].ctx
    ctx.set_option('coarse', coarse)
    try:
        c = Call(shape, kc, ths, coarse=coarse)
        assert c.ref.has_coarse == (coarse != 0 and c.S >= 4)
        check_iterates(c.run, c.ref.iterate, tag, tol_x=TOL_X, tol_res=TOL_RES, steps=K_STEPS)
        X, _ = c.converged()
        for j in range(nmu):
            ref = c.ref.solve(j)
            assert np.abs(X[:, j] - ref).max() < 1e-8 * np.abs(ref).max(), (tag, j)
        if c.ref.has_coarse:
            if nmu > 1:           # (one column: theta_0 is the call mean)
                X_ref, _ = c.reference(coarse_theta=ths[0]).iterate(2)
                _, X2, _ = c.run(2)
                err = float((np.linalg.norm(X2 - X_ref, axis=0) / np.linalg.norm(X_ref, axis=0)).max())
                print('FOM-BATCH {}: misses a coarse level built at theta_0 by {:.2e}'.format(tag, err))
                assert err > MUTANT_FLOOR, (tag, err)
            ctx.set_option('coarse', 0)
            check_mutant(c.run, c.ref.iterate, tag)
    finally:
        ctx.set_option('coarse', 1)


# ----------------------------------------------------------------------------------------------------------- iterates
@pytest.mark.parametrize('nmu', PANEL_WIDTHS)
def test_iterates_over_the_panel_widths(nmu):
    _cell(SWEEP[0], SWEEP[1], 1, nmu)


@pytest.mark.parametrize('shape, kc, coarse, nmu', OTHER_CELLS)
def test_iterates_over_the_cells(shape, kc, coarse, nmu):
    _cell(shape, kc, coarse, nmu)


# ------------------------------------------------------------------------------------------------------------ sources
def test_affine_sources_and_zero_columns():
    nmu, K = 20, 3
    ths = np.stack([[1.0, mu] for mu in _mus(nmu)])
    phi = np.random.default_rng(7).uniform(0.2, 1.0, (nmu, K))
    phi[4] = 0.0                                                    # one zero right-hand side in each panel
    phi[17] = 0.0
    c = Call(SWEEP[0], SWEEP[1], ths, K=K, phi=phi, seed=3)
    assert not c.ref.cols[:, 4].any() and not c.ref.cols[:, 17].any() and c.ref.cols[:, 5].any()
    check_iterates(c.run, c.ref.iterate, 'fom batch K=3 with zero columns')
    X, info = c.converged()
    assert not X[:, 4].any() and not X[:, 17].any()                 # exact zeros, and the call still converged
    for j in (0, 5, 16, 19):
        ref = c.ref.solve(j)
        assert np.abs(X[:, j] - ref).max() < 1e-8 * np.abs(ref).max(), j
    zero = Call(SWEEP[0], SWEEP[1], ths[:3], K=K, phi=np.zeros((3, K)), reference=False)     # nothing to solve at all
    rc, X0, info0 = zero.run(50)
    assert rc == 0 and not X0.any() and info0[0] == 0 and info0[1] == 0.0


# ----------------------------------------------------------------------------------------------------- column hygiene
def test_equal_columns_are_bitwise_equal_across_the_panel_boundary():
    c = Call(SWEEP[0], SWEEP[1], np.tile([1.0, 0.37], (17, 1)), reference=False)
    _, X, _ = c.run(6)
    assert np.isfinite(X).all() and X[:, 0].any()
    assert all(np.array_equal(X[:, 0], X[:, j]) for j in range(1, 17))
    Xc, _ = c.converged()
    assert all(np.array_equal(Xc[:, 0], Xc[:, j]) for j in range(1, 17))


def test_one_column_is_the_single_solve():
    th = np.array([[1.0, 0.37]])
    c = Call(SWEEP[0], SWEEP[1], th, reference=False)
    X, _ = c.converged(rtol=1e-13)
    eng = c.eng
    x1, _ = eng.ctx.fom_solve(th[0], eng.A_diag, eng.A_cpl, eng.b, rtol=1e-13)
    x1 = x1.cpu().numpy().ravel()
    assert np.linalg.norm(X[:, 0] - x1) < 1e-10 * np.linalg.norm(x1)


def test_two_calls_give_the_same_bits():
    ths = np.stack([[1.0, mu] for mu in _mus(33)])
    c = Call(SWEEP[0], SWEEP[1], ths, reference=False)
    (_, Xa, ia), (_, Xb, ib) = c.run(6), c.run(6)
    assert np.array_equal(Xa, Xb) and np.array_equal(ia, ib)
    (Xa, ia), (Xb, ib) = c.converged(), c.converged()
    assert np.array_equal(Xa, Xb) and np.array_equal(ia, ib)


def test_panel_info_reports_every_panel_of_the_last_call():
    from pylrbms_amd._native import _dblp
    ths = np.stack([[1.0, mu] for mu in _mus(33)])
    c = Call(SWEEP[0], SWEEP[1], ths, reference=False)
    eng = c.eng
    _, info = eng.ctx.fom_solve_batch(ths, eng.A_diag, eng.A_cpl, np.ones((33, 1)), c.b_K, rtol=1e-10)
    assert len(info['panel_iterations']) == 3 and min(info['panel_iterations']) >= 1
    assert max(info['panel_iterations']) == info['iterations'] and 0.0 < info['relative_residual'] <= 1e-10
    rc, _, raw_info = c.run(2)                                      # every panel is capped at max_iter
    panels = np.zeros(8)
    assert c.ctx.lib.lrbms_fom_solve_batch_panel_info(c.ctx.handle, _dblp(panels)) == 0
    assert rc == E_NOT_CONVERGED and list(panels[0::2]) == [2, 2, 2, 0] and panels[1::2].max() == raw_info[1] and panels[7] == 0.0


# ------------------------------------------------------------------------------------------------ buffers and refusals
def test_inputs_stay_unchanged_under_poisoned_buffers():
    ths = np.stack([[1.0, mu] for mu in _mus(17)])
    c = Call(SWEEP[0], SWEEP[1], ths, K=3, seed=1, reference=False)
    eng = c.eng
    before = [t.clone() for t in (eng.A_diag, eng.A_cpl, c.b_K, c.phi)]
    X, _ = c.converged()                                            # (work and X are NaN-poisoned by every raw call)
    assert np.isfinite(X).all()
    for was, now in zip(before, (eng.A_diag, eng.A_cpl, c.b_K, c.phi)):
        assert bool((was == now).all())


def test_refusals_before_any_launch():
    from pylrbms_amd._native import c_vp
    from pylrbms_amd import multiscale_problem
    from pylrbms_amd.engine import Engine
    from common import theta_bar_of
    ths = np.stack([[1.0, mu] for mu in _mus(3)])
    c = Call(SWEEP[0], SWEEP[1], ths, reference=False)
    assert c.raw(100000, rtol=1e-8)[0] == 0                          # the arguments below are otherwise fine
    wide = np.ones((65, 2))
    from pylrbms_amd._native import _dblp
    bad = [dict(nmu=0), dict(nmu=65, theta=_dblp(wide)), dict(K=0), dict(K=65), dict(Q=0), dict(Q=9), dict(rtol=0.0), dict(rtol=-1.0),
           dict(rtol=float('nan')), dict(max_iter=0)]
    bad += [{name: None} for name in ('theta', 'A_diag', 'A_cpl', 'phi', 'b_K', 'work', 'X')]
    for over in bad:
        rc, X, info = c.raw(10, **over)
        assert rc == E_INVALID, (over, rc)
        assert bool(X.isnan().all()) and bool(c.work.isnan().all()), over      # nothing was launched
    assert c.ctx.lib.lrbms_fom_solve_batch_work_size(c.ctx.handle, 0) < 0
    assert c.ctx.lib.lrbms_fom_solve_batch_work_size(c.ctx.handle, 65) < 0
    assert c.raw(100000, rtol=1e-8)[0] == 0                          # the context goes on

    class TwoRanks:
        rank, size = 0, 2

    p = multiscale_problem.init_grid_and_problem({'num_subdomains': list(SWEEP[0]), 'coarse_per_subdomain': SWEEP[1]}, mpi_comm=TwoRanks())
    lam = p['lambda']
    sharded = Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar_of(p)).assemble()
    c2, S2, t = sharded.ctx, sharded.S, sharded.ctx.t
    assert sharded.S_ext > S2
    X = c2.empty(S2, t.n, 3)
    X.fill_(float('nan'))
    work = c2.empty(max(1, int(c2.lib.lrbms_fom_solve_batch_work_size(c2.handle, 3))))
    info = np.zeros(2)
    rc = cells._raw(c2, 'lrbms_fom_solve_batch', 2, 3, _dblp(ths), c_vp(sharded.A_diag.data_ptr()), c_vp(sharded.A_cpl.data_ptr()), 1,
                    c_vp(c2.zeros(3, 1).data_ptr()), c_vp(sharded.b.data_ptr()), c_vp(work.data_ptr()), c_vp(X.data_ptr()), 1e-8, 10,
                    _dblp(info), c2._stream())
    assert rc == E_INVALID and bool(X.isnan().all())


# ------------------------------------------------------------------------------------------------------------- Python
def _discretization(affine):
    from pylrbms_amd import OS2015_academic_problem
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    import affine_source_ref
    p = affine_source_ref.make_problem() if affine else OS2015_academic_problem.init_grid_and_problem(affine_source_ref.SMALL)
    d, data = discretize(p)
    assert (d._affine_f is not None) == affine
    return d, data


@pytest.mark.parametrize('affine', (False, True))
def test_solve_batch_columns_are_the_single_solves(affine):
    d, _ = _discretization(affine)
    mus = [[float(v)] for v in np.linspace(0.1, 1.0, 70 if not affine else 7)]        # 70 crosses the chunk of 64
    U = d.solve_batch(mus)
    assert len(U) == len(mus) and tuple(U.tensor.shape) == (d.engine.S, d.engine.t.n, len(mus))
    its, rel = d.last_solve_info['iterations'], d.last_solve_info['relative_residual']
    assert its >= 1 and 0.0 < rel <= 1e-10
    X = U.tensor.cpu().numpy()
    for m, mu in enumerate(mus):
        ref = d.solve(mu).tensor.cpu().numpy()[..., 0]
        assert np.abs(X[..., m] - ref).max() <= 1e-8 * np.abs(ref).max(), (affine, m)


def test_solve_batch_feeds_the_local_pod():
    from pylrbms_amd.reductor import LRBMSReductor
    d, data = _discretization(False)
    reductor = LRBMSReductor(d, products=[d.operators['local_energy_dg_product_{}'.format(ii)]
                                          for ii in range(data['block_space'].num_blocks)])
    before = list(reductor.local_sizes())
    reductor.extend_basis(d.solve_batch([[float(v)] for v in np.linspace(0.1, 1.0, 9)]), method='pod', pod_modes=3)
    after = list(reductor.local_sizes())
    assert all(a > b for a, b in zip(after, before)), (before, after)
