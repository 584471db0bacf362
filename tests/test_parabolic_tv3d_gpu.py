"""Time-dependent diffusion coefficients theta_q(t, mu) on the 3D / P2 parabolic path on the GPU:
lrbms3_fom_implicit_euler_batch_tv, lrbms3_reduced_implicit_euler_batch_tv and lrbms3_reduced_parabolic_estimate_batch_tv against the
NumPy restatement tests/parabolic_tv3d_ref.py (pinned to the 3D references, and its faults shown to be visible at these cells, in
tests/test_parabolic_tv3d_host.py), against their twins in the bits where the table gives the twin's arithmetic, and end to end
through the Python layer on the switched-channels problem.

Cells, tables and tolerances: ``tv.RED_CELLS`` ... ``tv.EST_CELLS`` on the small problems of tests/common3d.py; ``tv.switch_table``
(a smooth factor per row and a 10 x switch between the steps 1 and 2); the tolerances of the twins' tests -- 1e-9 per step and
column for the reduced trajectories, 1e-8 for the full-order ones at rtol 1e-12, 1e-10 of the largest entry for the estimate."""
import ctypes

import numpy as np
import pytest

import common3d as c3
import fom_euler_batch3d_ref as fe
import parabolic_batch3d_ref as rb
import parabolic_estimate_batch3d_ref as pe
import parabolic_tv3d_ref as tv

pytestmark = pytest.mark.gpu

DT = tv.DT
TOL_TRAJ = 1e-9
TOL_FOM = 1e-8
TOL = 1e-10
E_INVALID, E_NOT_CONVERGED = -1, -4
NAN = float('nan')
OUTS = ('eta_loc', 'time_deriv_nc', 'time_residual', 'eta', 'est')


def _system(name, N, pad=0):
    """The system of tests/test_parabolic_estimate_batch3d_gpu.py (engine, pass, M_red, dense model; bases ``make_bases3d`` with N
    columns, the last ``pad`` of subdomain 1 zero) plus host copies of the reduced operators."""
    from test_parabolic_estimate_batch3d_gpu import _system as est_system
    s = est_system(name, N, pad)
    if 'B' not in s:
        s.update(B=s['out']['B_sys'].cpu().numpy().copy(), Mh=s['M'].cpu().numpy().copy(), rhs=s['out']['rhs_red'].cpu().numpy().copy(),
                 nbr=s['model']['nbr'])
    return s


def _table(s, nmu, nt):
    return tv.switch_table(nmu, nt, s['Q'], base=pe.cell_thetas(s['p'], nmu))


def _dev(ctx, a):
    return ctx.from_numpy(np.ascontiguousarray(a))


def _dblp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if a is not None else ctypes.POINTER(ctypes.c_double)()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(None)


def _raw(ctx, name, *args):
    rc = getattr(ctx.lib, name)(ctx.handle, *args)
    ctx.torch.cuda.synchronize(ctx.device)
    return rc


# ------------------------------------------------------------------------------------------------------- reduced trajectories
def _red_run(s, tab, nt, rhs_K=None, phis=None, U0=None, rtol=1e-13, **kw):
    ctx = s['ctx']
    rhs = s['out']['rhs_red'] if rhs_K is None else _dev(ctx, rhs_K)
    U, info = ctx.reduced_implicit_euler_batch_tv(s['Q'], tab, DT, nt, s['out']['B_sys'], s['M'], rhs, phi=phis,
                                                  U0=None if U0 is None else _dev(ctx, U0), rtol=rtol, **kw)
    assert tuple(U.shape) == (nt + 1, s['S'], s['N'], tab.shape[0])
    return U, info


def _red_check(s, tab, nt, tag, keep=None, **kw):
    U, (it, res) = _red_run(s, tab, nt, **kw)
    ref = tv.dense_euler_batch_tv(s['B'], s['Mh'], s['nbr'], tab, DT, nt, rhs=None if 'rhs_K' in kw else s['rhs'], keep=keep, **kw)
    err = rb.column_errors(U.cpu().numpy(), ref)
    print('TV3D reduced {}: {} iterations, worst (step, column) error {:.2e} (tolerance {:.0e})'.format(tag, it, float(err.max()), TOL_TRAJ))
    assert res <= 1e-13 and it >= nt
    assert np.isfinite(err).all() and err.max() < TOL_TRAJ, (tag, float(err.max()))
    return U, ref


@pytest.mark.parametrize('name, N, nmu, nt', tv.RED_CELLS)
def test_reduced_trajectories_against_row_by_row_stepping(name, N, nmu, nt):
    """Odd N on one row tile with one column and with a second group of one column, nt = 2 and 3; N = 30 on two row tiles with four
    groups on four streams; Q = 3 with three groups."""
    s = _system(name, N)
    _red_check(s, _table(s, nmu, nt), nt, '{} N={} nmu={} nt={}'.format(name, N, nmu, nt))


def test_reduced_trajectories_with_sources_and_a_coefficient_that_switches_sign():
    name, N, nmu, nt, K = tv.RED_SOURCE_CELL
    s = _system(name, N)
    _red_check(s, _table(s, nmu, nt), nt, 'K=3 sources', rhs_K=tv.source_rhs(s['rhs'], K), phis=tv.switching_phis(nmu, nt, K))


def test_reduced_trajectories_from_a_nonzero_start():
    name, N, nmu, nt = tv.RED_START_CELL
    s = _system(name, N)
    tab = _table(s, nmu, nt)
    zero = tv.dense_euler_batch_tv(s['B'], s['Mh'], s['nbr'], tab, DT, nt, rhs=s['rhs'])
    U0 = tv.start_panel(s['S'], N, nmu, np.abs(zero).max())
    U, _ = _red_check(s, tab, nt, 'non-zero U[0]', U0=U0)
    assert np.array_equal(U[0].cpu().numpy(), U0)


def test_reduced_trajectories_on_a_zero_padded_basis():
    """Subdomain 1 keeps N - 2 vectors: its padded unknowns stay exactly at U[0] = 0 in every step and column."""
    name, N, nmu, nt = tv.RED_PAD_CELL
    s = _system(name, N, pad=2)
    keep = s['keep'].astype(np.float64)
    U, _ = _red_check(s, _table(s, nmu, nt), nt, 'zero-padded basis', keep=keep)
    assert np.all(U.cpu().numpy()[:, keep == 0, :] == 0.0)


# ---------------------------------------------------------------------------------------------------- full-order trajectories
class TvCall:
    """One call of the raw lrbms3_fom_implicit_euler_batch_tv: the inputs, buffers and checks of ``Call`` in
    tests/test_fom_euler_batch3d_gpu.py (NaN-poisoned work and U[1:] between sentinel bands, slab 0 compared with what went in) with
    the table theta_t [nmu, nt + 1, Q]; ``twin``: the same call of the twin at row 1."""

    def __init__(self, name, nmu, nt, K, start, table=None):
        import test_fom_euler_batch3d_gpu as fg
        self.fg = fg
        p, eng = fg._engine(name)
        base = np.stack([c3.theta_of(p, mu) for mu in fe.cell_mus(nmu)])
        self.theta_t = tv.switch_table(nmu, nt, base.shape[1], base=base) if table is None else table
        b = eng.ops['b'].cpu().numpy()
        _, phis = tv.fom_source(b, K, nmu, nt)
        self.c = fg.Call(name, self.theta_t[:, 1], nt=nt, K=K, phis=phis, U0='start' if start else None, reference=False)
        Aq, mass, _ = fg._parts(name)
        self.kw = dict(Aq=Aq, mass=mass)
        self.ref = self.reference()

    def reference(self, fault=None):
        c = self.c
        return tv.BatchFomEulerTv3DRef(self.kw['Aq'], self.kw['mass'], c.S, c.t.n, self.theta_t, DT, c.nt, c.phis_host, c.b_K.cpu().numpy(),
                                       U0=c.U0_host, Phi=c.Phi, fault=fault)

    def raw(self, k, rtol=1e-14, twin=False, **over):
        c, fg = self.c, self.fg
        ctx, ops = c.ctx, c.eng.ops
        c.work.fill_(NAN)
        shape = (c.nt + 1, c.S, c.t.n, c.nmu)
        U_buf, U = fg._banded(ctx, int(np.prod(shape)))
        U = U.view(shape)
        U.fill_(NAN)
        U[0] = c.U0
        info = np.zeros(2)
        th = np.ascontiguousarray(self.theta_t[:, 1]) if twin else self.theta_t
        a = dict(Q=c.Q, K=c.K, nmu=c.nmu, theta=_dblp(th), dt=float(DT), nt=c.nt, A_diag=_vp(ops['A_diag']), A_cpl=_vp(ops['A_cpl']),
                 b_K=_vp(c.b_K), phi=_vp(c.phis), work=_vp(c.work), U=_vp(U), rtol=float(rtol), max_iter=int(k))
        a.update(over)
        rc = _raw(ctx, fg.EXPORT if twin else fg.EXPORT + '_tv', a['Q'], a['K'], a['nmu'], a['theta'], a['dt'], a['nt'], a['A_diag'],
                  a['A_cpl'], a['b_K'], a['phi'], a['work'], a['U'], a['rtol'], a['max_iter'], _dblp(info), ctx._stream())
        assert fg._bands_intact(U_buf) and fg._bands_intact(c.work_buf), 'a write outside U or work'
        assert bool((U[0] == c.U0).all()), 'slab 0 was written'
        return rc, U, info

    def run(self, k):
        """The ``run(k)`` of ``check_iterates``: nt = 2 with max_iter = k stops after the capped first step (slab 2 untouched)."""
        c = self.c
        rc, U, info = self.raw(k)
        pan, npan = c.panels(), (c.nmu + 15) // 16
        assert info[0] == pan[0:2 * npan:2].sum() and all(v == pan[0] for v in pan[0:2 * npan:2]), (info, pan)
        assert bool(U[2:].isnan().all()), 'a slab behind the capped step was written'
        Uh = U[:2].cpu().numpy().reshape(2, -1, c.nmu)
        return rc, Uh[1] - Uh[0], np.array([pan[0], info[1]])


@pytest.mark.parametrize('name, nmu, nt, K, start', tv.FOM_CELLS)
def test_full_order_trajectories_against_sparse_lu_stepping(name, nmu, nt, K, start):
    """q3_2x1x2: 17 columns, nt = 3 -- two panels, the last of one column.  interior_3x3x3: 33 columns, nt = 2, K = 2, a start
    value per column."""
    c = TvCall(name, nmu, nt, K, start)
    rc, U, info = c.raw(100000, rtol=1e-12)
    assert rc == 0 and 0.0 <= info[1] <= 1e-12, (rc, info)
    err = c.ref.column_errors(U.cpu().numpy())
    print('TV3D full order {} nmu={} nt={} K={}: {} iterations, worst (step, column) error {:.2e} (tolerance {:.0e})'.format(
        name, nmu, nt, K, int(info[0]), float(err.max()), TOL_FOM))
    assert np.isfinite(err).all() and err.max() < TOL_FOM, (name, float(err.max()))
    pan = c.c.panels()
    assert (pan[0:2 * ((nmu + 15) // 16):2] > 0).all() and info[0] == pan[0::2].sum()


# ------------------------------------------------------------------------------------------ preconditioner pinned by iterates
def test_full_order_iterates_pin_the_preconditioner_at_the_time_mean():
    """nt = 2, max_iter = k: U[1] - U[0] is the k-th PCG iterate on the row-1 operator with both levels at the mean over columns and
    rows 1 .. nt (``check_iterates``, TOL_X = 1e-10, TOL_RES = 1e-8 of tests/test_pcg_iterates_gpu.py); the references with the
    preconditioner at row 1 alone and at the rows 0 .. nt are missed by more than MUTANT_FLOOR at the same k."""
    from test_pcg_iterates_gpu import MIN_RATIO, MUTANT_FLOOR, TOL_RES, TOL_X, check_iterates
    name, nmu = tv.FOM_ITERATE_CELL
    c = TvCall(name, nmu, 2, 1, True)
    assert c.ref.has_coarse
    for k in tv.K_ITER:
        assert c.ref.iterate(k)[1].min() >= MIN_RATIO
    check_iterates(c.run, c.ref.iterate, 'fom euler batch tv 3D {} nmu={}'.format(name, nmu), tol_x=TOL_X, tol_res=TOL_RES, steps=tv.K_ITER)
    for k in tv.K_ITER:
        _, X, _ = c.run(k)
        for fault in tv.PRECOND_FAULTS:
            X_bad, _ = c.reference(fault).iterate(k)
            miss = float((np.linalg.norm(X - X_bad, axis=0) / np.linalg.norm(X_bad, axis=0)).max())
            print('TV3D full order iterates k={}: misses {} by {:.2e}'.format(k, fault, miss))
            assert miss > MUTANT_FLOOR, (k, fault, miss)


def test_reduced_iterates_pin_the_preconditioner_at_the_time_mean():
    """The same for the reduced solver from zero.  Tolerance as in tests/test_parabolic_batch3d_gpu.py: 100 x the difference of the
    float64 and the longdouble recurrences at k = 5, floor 1e-12; both mutants are missed by more than 100 x that at every k."""
    name, N, nmu = tv.ITERATE_CELL
    s = _system(name, N)
    ctx, S, Q = s['ctx'], s['S'], s['Q']
    B, M, nbr, rhs = s['B'], s['Mh'], s['nbr'], s['rhs']
    tab = _table(s, nmu, 2)
    P = tv.reduced_precond(B, M, nbr, tab, DT)
    assert P.has_coarse
    Minv, b = P.matrix(), DT * rhs.ravel()
    diff = 0.0
    for j in sorted({0, nmu // 2, nmu - 1}):
        Ad = rb.step_operator(B, M, nbr, tab[j, 1], DT).toarray()
        x64, _ = rb.pcg_dense(Ad, Minv, b, 5)
        xld, _ = rb.pcg_dense(Ad, Minv, np.longdouble(DT) * rhs.ravel().astype(np.longdouble), 5, dtype=np.longdouble)
        diff = max(diff, float(np.linalg.norm(x64 - xld) / np.linalg.norm(xld)))
    tol = max(100.0 * diff, 1e-12)
    work = ctx.empty(int(ctx.lib.lrbms3_reduced_implicit_euler_batch_work_size(ctx.handle, N, nmu)))
    for k in tv.K_ITER:
        X_ref, ratios = tv.reduced_first_step_iterates(B, M, nbr, tab, DT, rhs, k)
        U = ctx.zeros(3, S, N, nmu)
        U[2] = NAN
        info = (ctypes.c_double * 2)()
        rc = _raw(ctx, 'lrbms3_reduced_implicit_euler_batch_tv', Q, N, 0, nmu, _dblp(tab), DT, 2, _vp(s['out']['B_sys']), _vp(s['M']),
                  _vp(s['out']['rhs_red']), _vp(None), _vp(work), _vp(U), 1e-14, k, info, ctx._stream())
        assert rc == E_NOT_CONVERGED and int(info[0]) == k, (k, rc, info[0])
        assert bool(U[2].isnan().all()), 'the slab behind the capped step was written'
        X = U[1].cpu().numpy().reshape(S * N, nmu)
        nrm = np.linalg.norm(X_ref, axis=0)
        err = float((np.linalg.norm(X - X_ref, axis=0) / nrm).max())
        res = abs(info[1] - ratios.max()) / ratios.max()
        print('TV3D reduced iterates k={}: worst x_k error {:.2e} (tolerance {:.2e}), ratio error {:.2e}'.format(k, err, tol, res))
        assert np.isfinite(err) and err < tol and res < 1e-8, (k, err, tol, res)
        for fault in tv.PRECOND_FAULTS:
            X_bad, _ = tv.reduced_first_step_iterates(B, M, nbr, tab, DT, rhs, k, fault=fault)
            miss = float((np.linalg.norm(X - X_bad, axis=0) / np.linalg.norm(X_bad, axis=0)).max())
            print('TV3D reduced iterates k={}: misses {} by {:.2e}'.format(k, fault, miss))
            assert miss > 100.0 * tol, (k, fault, miss)


# ------------------------------------------------------------------------------------------------------------------ estimates
def _est_call(s, tab, coef, U, nt, out=None, ops=None, twin=False, **kw):
    ctx = s['ctx']
    Ud = U if hasattr(U, 'data_ptr') else _dev(ctx, U)
    fn = ctx.reduced_parabolic_estimate_batch if twin else ctx.reduced_parabolic_estimate_batch_tv
    r = fn(s['Q'], tab, coef, DT, nt, Ud, s['out']['B_sys'], s['M'], s['out'] if out is None else out,
           s['eng'].ops if ops is None else ops, s['eng'].hdiam, **kw)
    ctx.torch.cuda.synchronize()
    return r


def _host(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _check(got, want, tag):
    miss = pe.worst(got, want, DT)
    print('TV3D estimate {}: '.format(tag) + ', '.join('{} {:.2e}'.format(k, v) for k, v in miss.items()))
    for k, v in miss.items():
        assert np.isfinite(v) and v <= TOL, (tag, k, v)


@pytest.mark.parametrize('name, N, nmu, nt', tv.EST_CELLS)
def test_estimates_against_the_restatement_and_the_slab_export(name, N, nmu, nt):
    """nmu in {1, 16, 17, 33} x nt in {1, 3} on three problems; coef of (33, 3) needs two put chunks, the cell (64, 1) fills its one
    chunk exactly.  Slab by slab: the rows of U[k] are those of lrbms3_reduced_estimate_batch at row k."""
    s = _system(name, N)
    ctx, Q, S, eng = s['ctx'], s['Q'], s['S'], s['eng']
    U = pe.panel(S, N, nmu, nt)
    tab, coef = _table(s, nmu, nt), tv.coef_table(nmu, nt)
    got = _host(_est_call(s, tab, coef, U, nt))
    assert got['eta_loc'].shape == (3, nt + 1, S, nmu) and got['time_deriv_nc'].shape == (nt, S, nmu)
    assert all(np.isfinite(got[k]).all() for k in OUTS) and got['est'].min() > 0.0
    want = tv.estimate_outputs_tv(s['model'], tab, coef, DT, U)
    assert want['nc_dU'].min() >= -1e-12 * want['nc_dU'].max() and want['nc_dU'].max() > 0.0
    _check(got, want, '{} N={} nmu={} nt={} numpy'.format(name, N, nmu, nt))
    sc = 2.0 * np.sqrt(DT / 3.0)
    Ud = _dev(ctx, U)
    dUd = (Ud[1:] - Ud[:-1]).contiguous()
    rows = np.stack([ctx.reduced_estimate_batch(Q, np.ascontiguousarray(tab[:, k]), Ud[k].contiguous(), s['out'], eng.ops,
                                                eng.hdiam).cpu().numpy() for k in range(nt + 1)], axis=1)
    tr2 = np.stack([np.stack([ctx.reduced_time_residual(Q, np.ascontiguousarray(tab[m, k + 1]), s['out']['B_sys'], s['M'],
                                                        dUd[k:k + 1, :, :, m].contiguous()).sum(dim=1).cpu().numpy()[0]
                              for m in range(nmu)]) for k in range(nt)])
    e = {'eta_loc': c3.rel(got['eta_loc'], rows * sc), 'tr2': c3.rel(got['time_residual'] ** 2 * 3.0 / DT, tr2)}
    print('TV3D estimate {} N={} nmu={} nt={} exports: '.format(name, N, nmu, nt) + ', '.join('{} {:.2e}'.format(k, v) for k, v in e.items()))
    assert all(v <= TOL for v in e.values()), e


def test_estimate_with_a_switching_source_against_the_column_loop():
    """K = 3, the first source coefficient switching from row to row: the r rows are those of the call without f terms plus
    lrbms3_reduced_source_terms of U[k] with row k of BOTH tables, column by column."""
    from pylrbms_amd.sources3d import zeroed
    name, N, nmu, nt, K = 'interior_3x3x3', 5, 17, 3, 3
    s = _system(name, N)
    ctx, eng, Q, S = s['ctx'], s['eng'], s['Q'], s['S']
    F2, r_fd_K, bdiv_K, phi = tv.source_data(S, Q * N, ctx.n_T, K, nmu, nt)
    F2d, rKd, bKd = (_dev(ctx, x) for x in (F2, r_fd_K, bdiv_K))
    U = pe.panel(S, N, nmu, nt)
    tab, coef = _table(s, nmu, nt), tv.coef_table(nmu, nt)
    out0, ops0 = zeroed(eng, s['out'])
    got = _host(_est_call(s, tab, coef, U, nt, out=out0, ops=ops0, phi=phi, F2=F2d, r_fd_K=rKd, bdiv_K=bKd))
    base = _host(_est_call(s, tab, coef, U, nt, out=out0, ops=ops0))
    Ud = _dev(ctx, U)
    add = np.zeros((nt + 1, S, nmu))
    for k in range(nt + 1):
        add[k] = ctx.reduced_source_terms(Q, np.ascontiguousarray(tab[:, k]), np.ascontiguousarray(phi[:, k]), F2d, rKd, bKd,
                                          s['out']['Rb'], Ud[k].contiguous(), eng.ops['ceps'], eng.hdiam).cpu().numpy()
    sc = 2.0 * np.sqrt(DT / 3.0)
    e_r = c3.rel(got['eta_loc'][1], base['eta_loc'][1] + add * sc)
    raw = got['eta_loc'] / sc
    eta = sc * (coef[:, :, 0].T * np.linalg.norm(raw[0], axis=1) + coef[:, :, 1].T * np.linalg.norm(raw[1] + raw[2], axis=1))
    e_eta = c3.rel(got['eta'], eta)
    shifted = np.stack([ctx.reduced_source_terms(Q, np.ascontiguousarray(tab[:, min(k + 1, nt)]), np.ascontiguousarray(phi[:, k]), F2d, rKd,
                                                 bKd, s['out']['Rb'], Ud[k].contiguous(), eng.ops['ceps'], eng.hdiam).cpu().numpy()
                        for k in range(nt + 1)])
    print('TV3D estimate source K=3: r rows {:.2e}, eta {:.2e}; theta row k + 1 in the source terms would miss by {:.2e}'.format(
        e_r, e_eta, c3.rel(shifted, add)))
    assert np.abs(add).max() > 0.0 and e_r <= TOL and e_eta <= TOL and c3.rel(shifted, add) > 1e-6
    for k in ('time_deriv_nc', 'time_residual'):
        assert np.array_equal(got[k], base[k]), k


@pytest.mark.parametrize('option', ('estimate_valu', 'solve_valu'))
@pytest.mark.parametrize('name, N, nmu, nt', (('interior_3x3x3', 5, 33, 1), ('q3_2x1x2', 6, 33, 3)))
def test_estimate_valu_forms_agree_with_the_matrix_core_forms(option, name, N, nmu, nt):
    s = _system(name, N)
    ctx = s['ctx']
    U = pe.panel(s['S'], N, nmu, nt)
    tab, coef = _table(s, nmu, nt), tv.coef_table(nmu, nt)
    mfma = _host(_est_call(s, tab, coef, U, nt))
    ctx.set_option(option, 1)
    try:
        valu = _host(_est_call(s, tab, coef, U, nt))
    finally:
        ctx.set_option(option, 0)
    _check(valu, mfma, '{} {} N={}'.format(option, name, N))
    _check(valu, tv.estimate_outputs_tv(s['model'], tab, coef, DT, U), '{} {} N={} numpy'.format(option, name, N))
    assert any(not np.array_equal(valu[k], mfma[k]) for k in OUTS)          # the option reached a kernel of the call


# ----------------------------------------------------------------------------------------------------------------------- bits
def test_one_step_calls_give_the_bits_of_the_twins_at_row_one():
    """nt = 1: the time mean is row 1, the twin's arithmetic -- trajectories, info and panel info of both solvers are the twin's at
    theta = row 1, bit for bit (row 0 is not read by a solver).  The estimate reads row 0 for U[0]: with row 0 = row 1 and one coef
    row it gives the bits of its twin."""
    import torch
    c = TvCall('q3_2x1x2', 17, 1, 1, True)
    rc, U, info = c.raw(100000, rtol=1e-12)
    pan = c.c.panels().copy()
    rc2, U2, info2 = c.raw(100000, rtol=1e-12, twin=True)
    assert rc == rc2 == 0 and torch.equal(U, U2) and np.array_equal(info, info2) and np.array_equal(pan, c.c.panels())
    for name, N, nmu, K in (('interior_3x3x3', 5, 17, 0), ('aniso_2x2x1', 4, 16, 3)):
        s = _system(name, N)
        ctx, tab = s['ctx'], _table(s, nmu, 1)
        row1 = np.ascontiguousarray(tab[:, 1])
        if K:
            rhs_K, phis = _dev(ctx, tv.source_rhs(s['rhs'], K)), tv.switching_phis(nmu, 1, K)
            Ua, ia = ctx.reduced_implicit_euler_batch_tv(s['Q'], tab, DT, 1, s['out']['B_sys'], s['M'], rhs_K, phi=phis, rtol=1e-13)
            Ub, ib = ctx.reduced_implicit_euler_batch_src(s['Q'], row1, DT, 1, s['out']['B_sys'], s['M'], rhs_K, phis, rtol=1e-13)
        else:
            Ua, ia = ctx.reduced_implicit_euler_batch_tv(s['Q'], tab, DT, 1, s['out']['B_sys'], s['M'], s['out']['rhs_red'], rtol=1e-13)
            Ub, ib = ctx.reduced_implicit_euler_batch(s['Q'], row1, DT, 1, s['out']['B_sys'], s['M'], s['out']['rhs_red'], rtol=1e-13)
        assert torch.equal(Ua, Ub) and ia == ib and float(Ua[1].abs().max()) > 0.0, name
    s = _system('interior_3x3x3', 5)
    nmu = 33
    U = pe.panel(s['S'], 5, nmu, 1)
    row1, cf = np.ascontiguousarray(_table(s, nmu, 1)[:, 1]), np.ascontiguousarray(tv.coef_table(nmu, 1)[:, 1])
    a = _est_call(s, tv.constant_table(row1, 1), np.repeat(cf[:, None], 2, axis=1), U, 1)
    b = _est_call(s, row1, cf, U, 1, twin=True)
    for k in OUTS:
        assert torch.equal(a[k], b[k]), k


def test_a_constant_table_gives_the_bits_of_the_twin_estimate_swaps_swap_and_repeats_are_equal():
    """k3pe_combine_tv keeps the thread mapping and the summation order of k3pe_combine: a table that is constant in time gives the
    twin's bits in every output (nt = 3, three groups, with a source).  Columns 2 and 20 (two groups) exchanged in every input
    exchange the output bits; a second call gives the same bits."""
    import torch
    from pylrbms_amd.sources3d import zeroed
    name, N, nmu, nt, K = 'interior_3x3x3', 5, 33, 3, 2
    s = _system(name, N)
    ctx, eng = s['ctx'], s['eng']
    U = pe.panel(s['S'], N, nmu, nt)
    F2, r_fd_K, bdiv_K, phi = tv.source_data(s['S'], s['Q'] * N, ctx.n_T, K, nmu, nt)
    src = dict(F2=_dev(ctx, F2), r_fd_K=_dev(ctx, r_fd_K), bdiv_K=_dev(ctx, bdiv_K))
    out0, ops0 = zeroed(eng, s['out'])
    th, cf = pe.cell_thetas(s['p'], nmu), pe.coefficients(nmu)
    a = _est_call(s, tv.constant_table(th, nt), np.repeat(cf[:, None], nt + 1, axis=1), U, nt, out=out0, ops=ops0, phi=phi, **src)
    b = _est_call(s, th, cf, U, nt, out=out0, ops=ops0, twin=True, phi=phi, **src)
    for k in OUTS:
        assert torch.equal(a[k], b[k]), k
    tab, coef = _table(s, nmu, nt), tv.coef_table(nmu, nt)
    x = _host(_est_call(s, tab, coef, U, nt, out=out0, ops=ops0, phi=phi, **src))
    perm = np.arange(nmu)
    perm[[2, 20]] = [20, 2]
    y = _host(_est_call(s, np.ascontiguousarray(tab[perm]), np.ascontiguousarray(coef[perm]), np.ascontiguousarray(U[..., perm]), nt,
                        out=out0, ops=ops0, phi=np.ascontiguousarray(phi[perm]), **src))
    z = _host(_est_call(s, tab, coef, U, nt, out=out0, ops=ops0, phi=phi, **src))
    for k in OUTS:
        assert np.array_equal(x[k][..., perm], y[k]), k
        assert np.array_equal(x[k], z[k]), k
    assert not np.array_equal(x['est'][2], x['est'][20])


def test_repeat_calls_of_the_solvers_are_equal():
    import torch
    c = TvCall('q3_2x1x2', 17, 2, 1, True)
    (rc, U, info), (rc2, U2, info2) = c.raw(100000, rtol=1e-12), c.raw(100000, rtol=1e-12)
    assert rc == rc2 == 0 and torch.equal(U, U2) and np.array_equal(info, info2)
    s = _system('interior_3x3x3', 5)
    tab = _table(s, 33, 3)
    (Ua, ia), (Ub, ib) = _red_run(s, tab, 3), _red_run(s, tab, 3)
    assert torch.equal(Ua, Ub) and ia == ib


# -------------------------------------------------------------------------------------------------------------------- hygiene
def _banded(ctx, a):
    """A device copy of ``a`` between two NaN bands -> (view, whole buffer)."""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64)
    big = torch.full((a.size + 128,), NAN, dtype=torch.float64, device=ctx.device)
    big[64:64 + a.size] = ctx.from_numpy(a.reshape(-1))
    return big[64:64 + a.size].view(a.shape), big


def test_poisoned_work_guard_bands_and_untouched_inputs():
    """The wrappers' work and outputs NaN-filled between sentinel bands (tests/test_work_poison_gpu.py), the device inputs between NaN
    bands: the NaN-filled run gives the bits of the zero-filled one, the bands are intact, the inputs unchanged -- the reduced
    solver with sources and the estimate with a source, so that every stage writes.  (The full-order cells run every call that
    way: ``TvCall.raw``.)"""
    import torch
    from test_work_poison_gpu import poisoned
    from pylrbms_amd.sources3d import zeroed
    name, N, nmu, nt, K = 'interior_3x3x3', 5, 33, 3, 2
    s = _system(name, N)
    ctx, eng = s['ctx'], s['eng']
    tab, coef = _table(s, nmu, nt), tv.coef_table(nmu, nt)
    F2, r_fd_K, bdiv_K, phi = tv.source_data(s['S'], s['Q'] * N, ctx.n_T, K, nmu, nt)
    out0, ops0 = zeroed(eng, s['out'])
    ins = {k: _banded(ctx, v) for k, v in dict(U=pe.panel(s['S'], N, nmu, nt), phi=phi, F2=F2, r_fd_K=r_fd_K, bdiv_K=bdiv_K, B_sys=s['B'],
                                               M=s['Mh'], rhs_K=tv.source_rhs(s['rhs'], K), phis=tv.switching_phis(nmu, nt, K)).items()}
    before = {k: big.clone() for k, (_, big) in ins.items()}
    tab0, coef0 = tab.copy(), coef.copy()

    def estimate():
        r = ctx.reduced_parabolic_estimate_batch_tv(s['Q'], tab, coef, DT, nt, ins['U'][0], ins['B_sys'][0], ins['M'][0], out0, ops0,
                                                    eng.hdiam, phi=ins['phi'][0], F2=ins['F2'][0], r_fd_K=ins['r_fd_K'][0],
                                                    bdiv_K=ins['bdiv_K'][0])
        torch.cuda.synchronize()
        return r

    def solve():
        U, info = ctx.reduced_implicit_euler_batch_tv(s['Q'], tab, DT, nt, ins['B_sys'][0], ins['M'][0], ins['rhs_K'][0], phi=ins['phis'][0],
                                                      rtol=1e-13)
        torch.cuda.synchronize()
        return U, info

    first = poisoned(ctx, estimate)
    for k in OUTS:
        assert bool(torch.isfinite(first[k]).all()), k
    U, info = poisoned(ctx, solve)
    assert bool(torch.isfinite(U).all()) and info[1] <= 1e-13
    for k, (_, big) in ins.items():
        assert torch.equal(big.view(torch.int64), before[k].view(torch.int64)), k
    assert np.array_equal(tab, tab0) and np.array_equal(coef, coef0)


def test_installed_preconditioner_and_the_next_stationary_batch_are_untouched():
    import torch
    name, N, nmu, nt = 'interior_3x3x3', 5, 17, 2
    s = _system(name, N)
    ctx, Q = s['ctx'], s['Q']
    tab, coef = _table(s, nmu, nt), tv.coef_table(nmu, nt)
    U = pe.panel(s['S'], N, nmu, nt)
    B, rhs = s['out']['B_sys'], s['out']['rhs_red']
    thetas = np.ascontiguousarray(tab[:, 1])
    pc = ctx.reduced_precond_build(Q, c3.theta_of(s['p'], 0.6), B)
    pc0 = pc.clone()
    free_e, (free_U, free_i) = _est_call(s, tab, coef, U, nt), _red_run(s, tab, nt)
    ctx.reduced_precond_use(pc)
    try:
        u0, i0 = ctx.reduced_solve_batch(Q, thetas, B, rhs, rtol=1e-12)
        got_e, (got_U, got_i) = _est_call(s, tab, coef, U, nt), _red_run(s, tab, nt)
        u1, i1 = ctx.reduced_solve_batch(Q, thetas, B, rhs, rtol=1e-12)
    finally:
        ctx.reduced_precond_use(None)
    assert torch.equal(pc, pc0) and torch.equal(u0, u1) and i0 == i1
    assert torch.equal(got_U, free_U) and got_i == free_i
    for k in OUTS:
        assert torch.equal(got_e[k], free_e[k]), k


def test_refusals_leave_outputs_and_work_untouched():
    """Every limit and null pointer of the three exports: LRBMS_E_INVALID before any launch; a valid call succeeds afterwards."""
    name, N, nmu, nt = 'interior_3x3x3', 5, 3, 2
    s = _system(name, N)
    ctx, eng, Q, S = s['ctx'], s['eng'], s['Q'], s['S']
    poison = float(np.pi)
    tab, coef = _table(s, 65, nt), tv.coef_table(65, nt)
    # ---- reduced solver
    work = ctx.empty(int(ctx.lib.lrbms3_reduced_implicit_euler_batch_work_size(ctx.handle, 32, 64)))
    U = ctx.zeros(nt + 1, S, 33, 65)
    work.fill_(poison)
    U[1:] = poison
    info = (ctypes.c_double * 2)()
    B, M, rhs = s['out']['B_sys'], s['M'], s['out']['rhs_red']
    rKd, phid = _dev(ctx, s['rhs'][None]), _dev(ctx, np.ones((65, nt + 1, 1)))

    def red(N_=N, K=0, nmu_=nmu, dt=DT, nt_=nt, Bp=B, Up=U, th=tab, rp=rhs, ph=None):
        return _raw(ctx, 'lrbms3_reduced_implicit_euler_batch_tv', Q, N_, K, nmu_, _dblp(th), dt, nt_, _vp(Bp), _vp(M), _vp(rp), _vp(ph),
                    _vp(work), _vp(Up), 1e-12, 1000, info, ctx._stream())

    bad = [red(N_=33), red(nmu_=0), red(nmu_=65), red(dt=0.0), red(nt_=0), red(Bp=None), red(Up=None), red(th=None), red(rp=None),
           red(K=1, rp=rKd), red(K=0, ph=phid), red(K=65, rp=rKd, ph=phid), red(K=-1)]
    assert all(rc == E_INVALID for rc in bad), bad
    assert bool((U[1:] == poison).all()) and bool((work == poison).all())
    Uok = ctx.zeros(nt + 1, S, N, nmu)
    assert red(Up=Uok) == 0 and red(K=1, rp=rKd, ph=phid, Up=Uok) == 0
    # ---- full-order solver
    c = TvCall('q3_2x1x2', 3, 2, 1, False)
    null = ctypes.c_void_p(None)
    for over in (dict(Q=0), dict(Q=9), dict(nmu=0), dict(nmu=65), dict(K=0), dict(K=65), dict(nt=0), dict(dt=0.0), dict(rtol=0.0),
                 dict(max_iter=0), dict(theta=_dblp(None)), dict(A_diag=null), dict(A_cpl=null), dict(b_K=null), dict(phi=null),
                 dict(work=null)):
        rc, Uf, _ = c.raw(10, **over)
        assert rc == E_INVALID and bool(Uf[1:].isnan().all()) and bool(c.c.work.isnan().all()), over
    assert c.raw(100000, rtol=1e-12)[0] == 0
    # ---- estimate
    names = ('G_nc', 'G_bb', 'G_rdd', 'G_ab', 'G_aa', 'r_fd', 'Rb', 'Yb', 'Dp', 'Xab', 'As', 'Cn')
    dev = [_dev(ctx, pe.panel(S, N, nmu, nt)), B, M] + [s['out'][k] for k in names] + [eng.ops[k] for k in ('ebar', 'Bbb', 'bdiv', 'f2', 'ceps')]
    F2, r_fd_K, bdiv_K, phi = tv.source_data(S, Q * N, ctx.n_T, 2, nmu, nt)
    srcs = [_dev(ctx, x) for x in (phi, F2, r_fd_K, bdiv_K)]
    wsz = ctx.lib.lrbms3_reduced_parabolic_estimate_batch_tv_work_size
    size = int(wsz(ctx.handle, N, nmu, nt))
    twin_size = int(ctx.lib.lrbms3_reduced_parabolic_estimate_batch_work_size(ctx.handle, N, nmu, nt))
    assert size >= twin_size + (nt + 1) * nmu * Q + nmu * (nt + 1) * 2
    assert wsz(ctx.handle, 33, 3, 2) == -1 and wsz(ctx.handle, 5, 65, 2) == -1 and wsz(ctx.handle, 5, 3, 0) == -1 and wsz(ctx.handle, 0, 3, 2) == -1
    bufs = [ctx.empty(size), ctx.empty(3, nt + 1, S, nmu), ctx.empty(nt, S, nmu), ctx.empty(nt, nmu), ctx.empty(nt + 1, nmu), ctx.empty(nmu)]
    for b in bufs:
        b.fill_(poison)

    def est(Q_=Q, N_=N, K_=0, nmu_=nmu, nt_=nt, dt=DT, th=tab, cf=coef, drop=None, src=(None,) * 4, drop_buf=None):
        d = [None if i == drop else t for i, t in enumerate(dev)]
        b = [None if i == drop_buf else t for i, t in enumerate(bufs)]
        return _raw(ctx, 'lrbms3_reduced_parabolic_estimate_batch_tv', Q_, N_, K_, nmu_, nt_, dt, _dblp(th), _dblp(cf), *[_vp(t) for t in d],
                    float(eng.hdiam), *[_vp(t) for t in src], *[_vp(t) for t in b], ctx._stream())

    bad = [est(Q_=0), est(Q_=9), est(N_=0), est(N_=33), est(Q_=4, N_=17), est(nmu_=0), est(nmu_=65), est(nt_=0), est(dt=0.0), est(K_=-1),
           est(K_=65, src=srcs), est(th=None), est(cf=None), est(K_=2)]
    bad += [est(drop=i) for i in range(len(dev))] + [est(drop_buf=i) for i in range(len(bufs))]
    bad += [est(K_=2, src=[None if i == j else t for i, t in enumerate(srcs)]) for j in range(4)]
    bad += [est(K_=0, src=[t if i == j else None for i, t in enumerate(srcs)]) for j in range(4)]
    assert all(rc == E_INVALID for rc in bad), bad
    assert all(bool((b == poison).all()) for b in bufs)
    tab3, coef3 = np.ascontiguousarray(tab[:nmu]), np.ascontiguousarray(coef[:nmu])
    assert est(th=tab3, cf=coef3) == 0 and est(th=tab3, cf=coef3, K_=2, src=srcs) == 0
    want = _host(_est_call(s, tab3, coef3, dev[0], nt))
    assert est(th=tab3, cf=coef3) == 0
    assert np.array_equal(bufs[5].cpu().numpy(), want['est'])


# ----------------------------------------------------------------------------------------------------------------- end to end
def _parts_err(got, want, dt):
    (e0, p0), (e1, p1) = got, want
    sq = lambda p: (p[0], p[1], p[2], np.asarray(p[3]) ** 2 * 3.0 / dt, np.asarray(p[4]) ** 2 * dt)      # noqa: E731
    return abs(e0 - e1) / abs(e1), max(c3.rel(a, b) for a, b in zip(sq(p0), sq(p1)))


def test_switched_channels_end_to_end():
    """multiscale_problem3d on 2 x 2 x 2 subdomains of one cube, the channels closing between the steps 1 and 2: solve_batch ->
    extend_basis -> reduce -> rd.solve_batch / rd.estimate_batch with 3 parameters against ``d.estimate`` of the reconstructed
    trajectories, the verification path in Python (the squared parts to 1e-10 of their largest entry, est to 1e-9, as the twins'
    tests); the single calls are one column of the same exports; the switch moves the trajectory by more than 1e-3 of max |u|.

    One part is not the same quantity on the two sides, with or without a table: the time residual of the reduced model is
    y^T M_red^-1 y with y = V^T A V du, that of ``d.estimate`` y^T M^-1 y with y = A V du -- the Galerkin projection of the residual
    against the residual itself (the 2D test of the same chain leaves it out for this reason).  So nc, r, df and time_deriv_nc are
    compared with ``d.estimate`` part by part, est with the time residual taken out on both sides (that is |eta| + |time_deriv_nc|:
    alpha and gamma per row), and the time residual with the existing single export ``lrbms3_reduced_time_residual`` run per step at
    row k + 1, all at the bounds above.  The gap between the two time residuals is printed (measured on the MI355X: 3.1e-02 of the
    squared entries, 8.7e-03 of est)."""
    from pylrbms_amd import multiscale_problem3d as mp
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D, discretize
    cfg = {'num_subdomains': [2, 2, 2], 'cubes_per_subdomain': 1}
    T, nt, mus = 0.3, 3, [0.3, 0.6, 1.0]
    d, _ = discretize(mp.init_grid_and_problem(cfg, switch_off_after=0.15), T, nt)
    d0, _ = discretize(mp.init_grid_and_problem(cfg), T, nt)
    assert d._tv and not d0._tv
    tab = d.diffusion_coefficients(1.0)
    assert tab.tolist() == [[1.0, 1.0], [1.0, 1.0], [1.0, 0.1], [1.0, 0.1]]
    trajs, trajs0 = d.solve_batch(mus), d0.solve_batch(mus)
    for m, mu in enumerate(mus):
        a, b = trajs[m].contiguous().cpu().numpy(), trajs0[m].contiguous().cpu().numpy()
        assert np.array_equal(a[:, :, 0], b[:, :, 0]) and c3.rel(a[:, :, 1], b[:, :, 1]) < 1e-6      # the same until the switch
        moved = np.abs(a - b).max() / np.abs(b).max()
        print('TV3D end to end mu={}: the switch moves the trajectory by {:.2e} of max |u|'.format(mu, moved))
        assert moved > 1e-3, (mu, moved)
    single = d.solve(mus[1]).cpu().numpy()
    assert c3.rel(single, trajs[1].contiguous().cpu().numpy()) < 1e-6
    reductor = ParabolicLRBMSReductor3D(d)
    for U in trajs:
        reductor.extend_basis(U.contiguous()[:, :, 1:].contiguous())
    rd = reductor.reduce()
    assert rd.N <= 32 and d.Q * rd.N <= 64
    us, (it, res) = rd.solve_batch(mus, return_info=True)
    assert tuple(us.shape) == (len(mus), nt + 1, d.engine.S, rd.N) and res <= 1e-12
    ests = rd.estimate_batch(us, mus, native=True)
    for m, mu in enumerate(mus):
        want = d.estimate(reductor.reconstruct(us[m]), mu)
        gap_est, gap_parts = _parts_err(ests[m], want, rd.dt)
        tab = d.diffusion_coefficients(mu)
        du = (us[m][1:] - us[m][:-1]).contiguous()
        tr2 = np.array([float(d.engine.ctx.reduced_time_residual(d.Q, tab[k + 1], rd.out['B_sys'], rd.M_red, du[k:k + 1].contiguous()).sum())
                        for k in range(nt)])
        tres = np.sqrt(tr2 * rd.dt / 3.0)
        e_parts = max([c3.rel(np.asarray(ests[m][1][i]), np.asarray(want[1][i])) for i in (0, 1, 2)] +
                      [c3.rel(np.asarray(ests[m][1][4]) ** 2, np.asarray(want[1][4]) ** 2), c3.rel(np.asarray(ests[m][1][3]) ** 2, tres ** 2)])
        rest = [e - np.linalg.norm(parts[3]) for e, parts in (ests[m], want)]
        e_est = abs(rest[0] - rest[1]) / abs(rest[1])
        print('TV3D end to end mu={}: full against projected time residual: est {:.2e}, squared parts {:.2e}'.format(mu, gap_est, gap_parts))
        u1 = rd.solve(mu)                                    # the single calls: one column of the same exports
        assert tuple(u1.shape) == tuple(us[m].shape) and c3.rel(u1.cpu().numpy(), us[m].cpu().numpy()) < 1e-9
        s_est, s_parts = _parts_err(rd.estimate(us[m], mu), ests[m], rd.dt)
        err_u = c3.rel(reductor.reconstruct(us[m]).cpu().numpy(), trajs[m].contiguous().cpu().numpy())
        print('TV3D end to end mu={}: est {:.3e}; against d.estimate est {:.2e} parts {:.2e}; single calls est {:.2e} parts {:.2e}; '
              'reduction error {:.2e}'.format(mu, ests[m][0], e_est, e_parts, s_est, s_parts, err_u))
        assert ests[m][0] > 0.0 and e_est <= 1e-9 and e_parts <= TOL, (mu, e_est, e_parts)
        assert s_est <= 1e-9 and s_parts <= TOL, (mu, s_est, s_parts)
    with pytest.raises(NotImplementedError):
        d.theta(0.5)
    with pytest.raises(NotImplementedError):
        d.solve_stationary(0.5)
