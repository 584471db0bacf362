"""The three exports for time-dependent diffusion coefficients over their panel dispatch:
lrbms_reduced_implicit_euler_batch_tv, lrbms_fom_implicit_euler_batch_tv and lrbms_reduced_parabolic_estimate_batch_tv at the
widths, basis sizes, component counts and launch forms that tests/test_parabolic_tv_gpu.py (N <= 24, nmu <= 33, Q = 2, U[0] = 0)
leaves out.

1. reduced trajectories at every (group width, k-step count) of k_bcg_matvec_panel<.., MASS>, panels of 16 past N = 32 and both
   sides of the block inverse's LDS opt-in, with sources and zero-padded bases;  2. from non-zero initial data;  3. Q = 3, 4 on
   the wide panels (the mass coefficient sits at table slot [m][Q]) and Q = 8 on panels of 16;  4. the VALU form with two, three
   and four groups under poisoned work;  5. first-step iterates against a NumPy PCG whose preconditioner sits at the mean over the
   columns and the rows 1 .. nt, and two references at other rows that the device must miss;  6. full-order trajectories over two
   to four panels, nt = 1, Q = 5, U0, coarse = 0, and the iterates that pin the coarse level;  7. estimates whose coefficient table
   needs one, one and a short, two, and exactly two uploads of 256 doubles, under poisoned work;  8. more than 64 parameters through
   the reduced model and the discretization.

Reduced cells: the system of tests/test_parabolic_batch_gpu.py (4 x 3 subdomains, k_c = 2, NMAX = 64 energy-orthonormal columns,
cut to N), tables from ``parabolic_tv_ref.switch_table`` with the switch between the steps 1 and 2, nt in (2, 3), dt = 0.05 / nt.
All tolerances are those of the twins.  tests/test_parabolic_tv_dispatch_host.py shows on the CPU that the cells reach every host
choice and that the references move by far more than the tolerances under the faults they are meant to catch."""
import numpy as np
import pytest

import parabolic_tv_ref as tv
import pcg_ref
from fom_euler_batch_ref import component_operators, p1_mass
from parabolic_batch_ref import column_errors, dense_euler, mass_operator
from parabolic_estimate_batch_ref import nc_of_differences
from test_fom_euler_batch_gpu import Call
from test_parabolic_batch_gpu import NMAX, T_END, TOL_TRAJ, _cut, _system
from test_parabolic_estimate_batch_gpu import TOL as TOL_EST
from test_parabolic_tv_gpu import _channels, _coef, _err, _estimate_reference, _host, _panel, _sources, _sys, _tables
from test_parabolic_tv_gpu import _cut as _cut_of
from test_parabolic_tv_gpu import _grams as _grams24
from test_pcg_iterates_gpu import (K_STEPS, KC, MUTANT_FLOOR, TOL_RES, TOL_X, _dev, _energy_bases, _model, _raw, check_iterates,
                                   check_mutant)
from test_work_poison_gpu import poisoned

pytestmark = pytest.mark.gpu

TAG = 'PARABOLIC-TV-DISPATCH'
# (N, nmu): the branch reached
REDUCED_CELLS = ((40, 1), (64, 16),          # panels of 16 past N = 32
                 (33, 17),                   # GW 32, ksc_n 10
                 (40, 32),                   # a full group of 32
                 (16, 64), (32, 47), (48, 33),      # GW 64, ksc_n 4 / 8 / 12
                 (63, 49), (64, 64))         # GW 64, ksc_n 16: the two sides of the block inverse's 64 KB LDS opt-in
SOURCE_CELLS = ((33, 17), (48, 33))          # ... once more with K = 3 time-dependent sources
RAGGED_CELL = (40, 32)
U0_CELLS = ((24, 16), (40, 47))
Q_CELLS = ((3, 17, 33), (4, 33, 24), (4, 64, 40), (8, 16, 33))          # Q, nmu, N on the 3 x 3 grid
Q_GRID, Q_NB = (3, 3), 40
VALU_CELLS = ((24, 17, 2), (64, 40, 3), (48, 64, 4))                    # N, nmu, groups of 16
ITERATE_CELLS = ((5, 3), (24, 17), (40, 47))
ITERATE_EXTRA = (24, 17)                     # once more from non-zero U0 and once with K = 3
ITERATE_NT = 2
FOM_GRIDS = ((2, 2), (3, 3))
FOM_PANELS = (33, 49, 64)                    # three panels with a short last one, four with a short one, four full ones
FOM_ITERATE_NMU = (3, 17, 33)
EST_CELLS = ((33, 16, 2), (40, 33, 3), (48, 49, 4), (64, 64, 3))        # N, nmu, nt: 96, 264, 490 and 512 coef doubles
EST_BOTH_LAYOUTS = ((40, 33, 3), (64, 64, 3))
EST_MAIN = (40, 33, 3)
EST_Q_CELLS = ((4, 17), (8, 16))             # Q, nmu on the 3 x 3 grid at N = 24
EST_VALU_LAYOUT = {'solve_valu': 'factored', 'estimate_valu': 'dense'}   # k_reduced_estimate_batch (VALU) takes the dense layout only
SWAP = (5, 40)                               # two columns of the 49 in different 16-column blocks

_REF = {}
_QSYS = {}
_EST = {}


def nt_of(N, nmu):
    """nt in (2, 3), fixed per cell; the largest dense references (N + nmu even) run two steps."""
    return 3 if (N + nmu) % 2 else 2


def tables(nmu, nt, Q=2, seed=0):
    """``switch_table`` with the switch at 1.4 dt: between the steps 1 and 2, so the rows 1 and 2 differ by it."""
    assert nt >= 2
    return _tables(nmu, nt, Q, seed=seed)


def start_values(B, M, rhs, nbr, theta, nmu, seed=11):
    """U0 [S, N, nmu] that differs per column and has the size of a solution (one dense step from zero at ``theta``)."""
    S, N = M.shape[:2]
    u_scale = np.abs(dense_euler(B, M, nbr, theta, T_END, 1, rhs=rhs)).max()
    return np.ascontiguousarray(np.random.default_rng(seed).standard_normal((S, N, nmu)) * u_scale)


def _part(what, worst, tol, extra=''):
    return '{}: worst error {:.2e} (tolerance {:.0e}){}'.format(what, worst, tol, extra)


def _say(*parts):
    """The one line of a test: every worst error next to its tolerance."""
    print('{} {}'.format(TAG, '; '.join(parts)))


# ------------------------------------------------------------------------------------------------- 1. reduced trajectories
def _inputs(N, nmu, nt, K=0, ragged=False, with_U0=False, const=False):
    """The host inputs of a reduced cell and its dense reference, computed once per cell and left unchanged."""
    key = (N, nmu, nt, K, ragged, with_U0, const)
    if key not in _REF:
        s = _system()
        B, M, rhs, keep = _cut_of(s, N, ragged)
        th = tables(nmu, nt, seed=N + nmu)
        if const:
            th = np.ascontiguousarray(np.repeat(th[:, 1:2], nt + 1, axis=1))
        c = dict(B=B, M=M, rhs=rhs, keep=keep, th=th, rhs_K=None, phis=None, U0=None)
        if K:
            c['rhs_K'], c['phis'] = _sources(s, N, nmu, nt, K, rhs)
            if keep is not None:
                c['rhs_K'] = c['rhs_K'] * keep
        if with_U0:
            c['U0'] = start_values(B, M, rhs, s['nbr'], th[0, 1], nmu)
        c['ref'] = tv.dense_euler_batch_tv(B, M, s['nbr'], th, T_END / nt, nt, rhs=None if K else rhs, rhs_K=c['rhs_K'],
                                           phis=c['phis'], U0=c['U0'], keep=keep)
        c['ref'].setflags(write=False)
        _REF[key] = c
    return _REF[key]


def _solve(c, nt):
    ctx = _system()['eng'].ctx
    U0 = None if c['U0'] is None else _dev(ctx, c['U0'])
    if c['rhs_K'] is not None:
        return ctx.reduced_implicit_euler_batch_tv(c['th'], T_END / nt, nt, _dev(ctx, c['B']), _dev(ctx, c['M']), _dev(ctx, c['rhs_K']),
                                                   phi=c['phis'], U0=U0)
    return ctx.reduced_implicit_euler_batch_tv(c['th'], T_END / nt, nt, _dev(ctx, c['B']), _dev(ctx, c['M']), _dev(ctx, c['rhs']), U0=U0)


def _check_trajectories(U, info, c, nt, what):
    Uh = U.cpu().numpy()
    assert Uh.shape == c['ref'].shape
    err = column_errors(Uh, c['ref'])
    part = _part(what, float(err.max()), TOL_TRAJ, ', {} iterations'.format(info['iterations']))
    assert info['relative_residual'] <= 1e-13 and info['iterations'] >= nt, part
    assert np.isfinite(Uh).all() and np.isfinite(err).all() and err.max() < TOL_TRAJ, part
    return Uh, part


def _reduced_cell(N, nmu, K=0, ragged=False, with_U0=False):
    nt = 3 if with_U0 else nt_of(N, nmu)
    c = _inputs(N, nmu, nt, K, ragged, with_U0)
    U, info = _solve(c, nt)
    Uh, part = _check_trajectories(U, info, c, nt, 'reduced N={} nmu={} nt={} K={} ragged={} U0={}'.format(N, nmu, nt, K, ragged, with_U0))
    _say(part)
    if with_U0:
        assert np.array_equal(Uh[0], c['U0'])
    return Uh, c


@pytest.mark.parametrize('N, nmu', REDUCED_CELLS)
def test_reduced_trajectories_over_the_panel_dispatch(N, nmu):
    _reduced_cell(N, nmu)


@pytest.mark.parametrize('N, nmu', SOURCE_CELLS)
def test_reduced_trajectories_with_sources_on_the_wide_panels(N, nmu):
    _reduced_cell(N, nmu, K=3)


def test_reduced_trajectories_with_zero_padded_bases_in_a_full_group():
    Uh, c = _reduced_cell(*RAGGED_CELL, ragged=True)
    keep = c['keep']
    assert (keep == 0).any() and np.all(Uh[:, keep == 0, :] == 0.0)           # the padding stays exactly 0


# ------------------------------------------------------------------------------------------- 2. non-zero initial data
@pytest.mark.parametrize('N, nmu', U0_CELLS)
def test_reduced_trajectories_from_non_zero_initial_data(N, nmu):
    _reduced_cell(N, nmu, with_U0=True)


def test_constant_table_from_non_zero_initial_data_is_the_existing_export():
    N, nmu = U0_CELLS[0]
    nt = 3
    c = _inputs(N, nmu, nt, with_U0=True, const=True)
    ctx = _system()['eng'].ctx
    U1, info = _solve(c, nt)
    _, part = _check_trajectories(U1, info, c, nt, 'reduced constant table N={} nmu={} U0'.format(N, nmu))
    U0, _ = ctx.reduced_implicit_euler_batch(np.ascontiguousarray(c['th'][:, 1]), T_END / nt, nt, _dev(ctx, c['B']), _dev(ctx, c['M']),
                                             _dev(ctx, c['rhs']), U0=_dev(ctx, c['U0']))
    err = float(column_errors(U1.cpu().numpy(), U0.cpu().numpy()).max())
    _say(part, _part('against the twin from the same U0', err, TOL_TRAJ))
    assert err < TOL_TRAJ


# ------------------------------------------------------------------------------------------------ 3. Q on the wide panels
def _qsys(Q):
    """The 3 x 3 grid of tests/test_parabolic_tv_gpu.py at Q_NB = 40 energy-orthonormal columns, per Q."""
    if Q not in _QSYS:
        m = _model(Q_GRID, 0, Q=Q, kc=KC)
        eng = m['eng']
        buf = eng.project_and_estimate(eng.ctx.from_numpy(_energy_bases(eng, Q_NB, seed=5)))
        _QSYS[Q] = dict(eng=eng, nbr=m['nbr'], Q=m['Q'], B=buf['sys'][0].cpu().numpy(), rhs=buf['sys'][1].cpu().numpy(),
                        M=buf['sys'][3].cpu().numpy())
    return _QSYS[Q]


@pytest.mark.parametrize('Q, nmu, N', Q_CELLS)
def test_reduced_trajectories_over_the_component_counts(Q, nmu, N):
    s = _qsys(Q)
    assert s['Q'] == Q
    ctx = s['eng'].ctx
    nt = nt_of(N, nmu)
    B, M, rhs, _ = _cut_of(s, N)
    th = tables(nmu, nt, Q, seed=N + nmu)
    U, info = ctx.reduced_implicit_euler_batch_tv(th, T_END / nt, nt, _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs))
    c = dict(ref=tv.dense_euler_batch_tv(B, M, s['nbr'], th, T_END / nt, nt, rhs=rhs))
    _say(_check_trajectories(U, info, c, nt, 'reduced Q={} N={} nmu={} nt={}'.format(Q, N, nmu, nt))[1])


# ------------------------------------------------------------------------------------------------------------ 4. VALU form
@pytest.mark.parametrize('N, nmu, groups', VALU_CELLS)
def test_reduced_trajectories_valu_form_under_poisoned_work(N, nmu, groups):
    """Groups of 16 with the gather / scatter path: zero- and NaN-filled work between sentinel bands, against the dense reference
    and against the matrix-core result of the same cell."""
    assert (nmu + 15) // 16 == groups
    ctx = _system()['eng'].ctx
    nt = nt_of(N, nmu)
    c = _inputs(N, nmu, nt)
    U_mfma, _ = _solve(c, nt)
    ctx.set_option('solve_valu', 1)
    try:
        U, info = poisoned(ctx, lambda: _solve(c, nt))
    finally:
        ctx.set_option('solve_valu', 0)
    Uh, part = _check_trajectories(U, info, c, nt, 'reduced VALU N={} nmu={} nt={} groups={}'.format(N, nmu, nt, groups))
    err = float(column_errors(Uh, U_mfma.cpu().numpy()).max())
    _say(part, _part('against the matrix-core form', err, TOL_TRAJ))
    assert err < TOL_TRAJ


# ------------------------------------------------------------------------- 5. first-step iterates pin the tv preconditioner
def iterate_inputs(B, M, rhs, nbr, nmu, K=0, with_U0=False, seed=0):
    """Host inputs of an iterate cell (NumPy only): the table [nmu, 3, Q], the right-hand side as the export takes it, phi, the
    columns dt b_m of the first step (row 1 of phi) and the start values [S N, nmu]."""
    S, N = M.shape[:2]
    nt, dt = ITERATE_NT, T_END / ITERATE_NT
    th = tables(nmu, nt, B.shape[0], seed=N + nmu)
    phi = None
    if K == 0:
        cols = dt * np.repeat(rhs.reshape(-1, 1), nmu, axis=1)
    else:
        rng = np.random.default_rng(seed)
        rhs = np.ascontiguousarray(rng.standard_normal((K, S, N)) * np.abs(rhs).max())
        phi = np.ascontiguousarray(rng.uniform(0.2, 1.0, (nmu, nt + 1, K)))
        cols = dt * np.einsum('mk,kn->nm', phi[:, 1], rhs.reshape(K, -1))
    U0 = start_values(B, M, rhs if K == 0 else rhs[0], nbr, th[0, 1], nmu) if with_U0 else None
    return dict(th=th, rhs=rhs, phi=phi, cols=cols, U0=U0, dt=dt, nt=nt)


def iterate_reference(B, M, nbr, inp, pc_theta=None, coarse=1):
    """reference(k) of ``check_iterates`` for the first step: per column the PCG on the step operator of row 1 with ONE
    preconditioner, ``ReducedPrecond`` of the step blocks at ``pc_theta`` (default: the mean over the columns and the rows
    1 .. nt).  With start values the right-hand side is the start residual and the ratio refers to |M u_0 + dt b|."""
    S, N = M.shape[:2]
    th, dt, cols = inp['th'], inp['dt'], inp['cols']
    nmu = th.shape[0]
    As = [pcg_ref.reduced_operator(tv.row_step_blocks(B, M, th[m, 1], dt), nbr) for m in range(nmu)]
    P = pcg_ref.ReducedPrecond(tv.row_step_blocks(B, M, tv.step_mean(th) if pc_theta is None else pc_theta, dt), nbr, coarse)
    scale = np.ones(nmu)
    if inp['U0'] is not None:
        u0 = inp['U0'].reshape(S * N, nmu)
        full = mass_operator(M) @ u0 + cols
        cols = np.stack([full[:, j] - As[j] @ u0[:, j] for j in range(nmu)], axis=1)
        scale = np.linalg.norm(cols, axis=0) / np.linalg.norm(full, axis=0)

    def reference(k):
        out = [pcg_ref.pcg_iterate(lambda p, A=A: A @ p, P.apply, cols[:, j], k) for j, A in enumerate(As)]
        return np.stack([x for x, _ in out], axis=1), np.array([r for _, r in out]) * scale
    return reference, P


def _iterate_cell(N, nmu, K=0, with_U0=False):
    """(run, inputs) of the raw export with nt = 2 and max_iter = k: the driver stops after the capped first step, U[1] - U[0] is
    the k-th iterate and U[2] stays as it was."""
    from pylrbms_amd._native import _dblp, c_vp
    s = _system()
    ctx, S = s['eng'].ctx, s['eng'].S
    B, M, rhs = _cut(N)
    inp = iterate_inputs(B, M, rhs, s['nbr'], nmu, K, with_U0)
    nt = inp['nt']
    Bd, Md, rd = _dev(ctx, B), _dev(ctx, M), _dev(ctx, inp['rhs'])
    phid = None if inp['phi'] is None else _dev(ctx, inp['phi'])
    work = ctx.empty(int(ctx.lib.lrbms_reduced_implicit_euler_batch_tv_work_size(ctx.handle, N, nmu, nt)))

    def run(k, rtol=1e-14):
        U = ctx.zeros(nt + 1, S, N, nmu)
        if inp['U0'] is not None:
            U[0] = _dev(ctx, inp['U0'])
        info = np.zeros(2)
        rc = _raw(ctx, 'lrbms_reduced_implicit_euler_batch_tv', B.shape[0], N, K, nmu, _dblp(inp['th']), inp['dt'], nt, c_vp(Bd.data_ptr()),
                  c_vp(Md.data_ptr()), c_vp(rd.data_ptr()), c_vp(None) if phid is None else c_vp(phid.data_ptr()),
                  c_vp(work.data_ptr()), c_vp(U.data_ptr()), float(rtol), int(k), _dblp(info), ctx._stream())
        Uh = U.cpu().numpy().reshape(nt + 1, S * N, nmu)
        assert not Uh[2].any()                                              # no step after the one that missed
        return rc, Uh[1] - Uh[0], info
    return run, inp, (B, M, s['nbr'])


def _miss(run, reference, what):
    X_ref, _ = reference(2)
    _, X2, _ = run(2)
    err = float((np.linalg.norm(X2 - X_ref, axis=0) / np.linalg.norm(X_ref, axis=0)).max())
    assert err > MUTANT_FLOOR, (what, err)
    return 'x_2 misses {} by {:.2e} (floor {:.0e})'.format(what, err, MUTANT_FLOOR)


@pytest.mark.parametrize('N, nmu', ITERATE_CELLS)
def test_first_step_iterates_against_numpy_pcg(N, nmu):
    run, inp, (B, M, nbr) = _iterate_cell(N, nmu)
    ref, P = iterate_reference(B, M, nbr, inp)
    assert P.has_coarse
    tag = 'euler batch tv N={} nmu={}'.format(N, nmu)
    cell, res = check_iterates(run, ref, tag, tol_x=TOL_X, tol_res=TOL_RES, steps=K_STEPS)
    th = inp['th']
    _say(_part('iterates N={} nmu={}'.format(N, nmu), cell, TOL_X, ', worst ratio error {:.2e} (tolerance {:.0e})'.format(res, TOL_RES)),
         _miss(run, iterate_reference(B, M, nbr, inp, pc_theta=tv.step_mean(th, last=1))[0], 'a preconditioner at row 1'),
         _miss(run, iterate_reference(B, M, nbr, inp, pc_theta=tv.step_mean(th, first=0))[0], 'a preconditioner at the rows 0 .. nt'))
    ctx = _system()['eng'].ctx
    ctx.set_option('coarse', 0)
    try:
        check_mutant(run, ref, tag)
    finally:
        ctx.set_option('coarse', 1)


@pytest.mark.parametrize('K, with_U0', ((0, True), (3, False)))
def test_first_step_iterates_from_initial_data_and_with_sources(K, with_U0):
    N, nmu = ITERATE_EXTRA
    run, inp, (B, M, nbr) = _iterate_cell(N, nmu, K=K, with_U0=with_U0)
    ref, _ = iterate_reference(B, M, nbr, inp)
    cell, res = check_iterates(run, ref, 'euler batch tv N={} nmu={} K={} U0={}'.format(N, nmu, K, with_U0))
    _say(_part('iterates N={} nmu={} K={} U0={}'.format(N, nmu, K, with_U0), cell, TOL_X,
               ', worst ratio error {:.2e} (tolerance {:.0e})'.format(res, TOL_RES)))


# --------------------------------------------------------------------------------- 6. full-order trajectories and iterates
def _fom_check(shape, nmu, nt, Q=2, K=1, with_U0=False, coarse=1, seed=0):
    m = _model(shape, 0, Q=Q, kc=KC)
    eng = m['eng']
    assert m['Q'] == Q
    ctx, S, n = eng.ctx, eng.S, eng.t.n
    th = _tables(nmu, nt, Q, seed=seed + nmu)
    rng = np.random.default_rng(seed + 1)
    b = eng.b.reshape(1, S, n)
    if K > 1:
        b_K = ctx.from_numpy(np.concatenate([b.cpu().numpy(), rng.standard_normal((K - 1, S, n)) * float(b.abs().max())]))
        phis = np.ascontiguousarray(rng.uniform(0.2, 1.0, (nmu, nt + 1, K)))
    else:
        b_K, phis = b.contiguous(), np.ones((nmu, nt + 1, 1))
    dt = T_END / nt
    Aq = component_operators(eng.A_diag.cpu().numpy(), eng.A_cpl.cpu().numpy(), ctx.t, m['nbr'])
    mass = p1_mass(ctx.t.area, S)
    U0 = None
    if with_U0:
        u_scale = np.abs(tv.fom_euler_tv(Aq, mass, th[0], T_END, 1, phis[0][:2], b_K.cpu().numpy(), rows=th[0, 1:2])).max()
        U0 = np.ascontiguousarray(rng.standard_normal((S * n, nmu)) * u_scale)
    ctx.set_option('coarse', coarse)
    try:
        U, info = ctx.fom_implicit_euler_batch_tv(th, dt, nt, eng.A_diag, eng.A_cpl, b_K, phis,
                                                  U0=None if U0 is None else _dev(ctx, U0.reshape(S, n, nmu)))
    finally:
        ctx.set_option('coarse', 1)
    ref = tv.fom_euler_batch_tv(Aq, mass, th, dt, nt, phis, b_K.cpu().numpy(), U0=U0)
    Uh = U.cpu().numpy().reshape(nt + 1, S * n, 1, nmu)
    err = column_errors(Uh, ref.reshape(nt + 1, S * n, 1, nmu))
    _say(_part('fom {} nmu={} nt={} Q={} K={} U0={} coarse={}'.format(shape, nmu, nt, Q, K, with_U0, coarse), float(err.max()), TOL_TRAJ,
               ', panels {}'.format(info['panel_iterations'])))
    assert len(info['panel_iterations']) == (nmu + 15) // 16 and min(info['panel_iterations']) >= nt
    assert info['relative_residual'] <= 1e-12
    assert np.isfinite(Uh).all() and np.isfinite(err).all() and err.max() < TOL_TRAJ, float(err.max())
    if with_U0:
        assert np.array_equal(Uh[0, :, 0, :], U0)


@pytest.mark.parametrize('nmu', FOM_PANELS)
def test_full_order_trajectories_over_the_panels(nmu):
    _fom_check(FOM_GRIDS[nmu % 2], nmu, 2, K=3 if nmu == 33 else 1)


@pytest.mark.parametrize('kw', (dict(nmu=17, nt=1), dict(nmu=3, nt=2, Q=5), dict(nmu=17, nt=2, with_U0=True),
                                dict(nmu=17, nt=2, coarse=0)), ids=('nt1', 'Q5', 'U0', 'coarse0'))
def test_full_order_trajectories_further_cells(kw):
    _fom_check((3, 3), **kw)


class CallTv(Call):
    """``test_fom_euler_batch_gpu.Call`` on lrbms_fom_implicit_euler_batch_tv: ``thetas`` of the base class are the row-1 tables
    (the operators of the first step), the reference's coarse level sits at the mean over the columns and the rows 1 .. nt, and
    ``run`` takes nt = 2: every panel stops after its capped first step."""

    def __init__(self, shape, kc, theta_t, coarse=1):
        self.theta_t = np.ascontiguousarray(theta_t, dtype=np.float64)
        Call.__init__(self, shape, kc, self.theta_t[:, 1], nt=self.theta_t.shape[1] - 1, coarse=coarse, reference=False)
        self.ref = self.reference()

    def reference(self, **kw):
        kw.setdefault('coarse_theta', tv.step_mean(self.theta_t))
        return Call.reference(self, **kw)

    def raw(self, k, rtol=1e-14):
        from pylrbms_amd._native import _dblp, c_vp
        import test_pcg_iterates_gpu as cells
        ctx, eng = self.ctx, self.eng
        self.work.fill_(float('nan'))
        U = ctx.empty(self.nt + 1, self.S, self.t.n, self.nmu)
        U.fill_(float('nan'))
        U[0] = 0.0
        info = np.zeros(2)
        rc = cells._raw(ctx, 'lrbms_fom_implicit_euler_batch_tv', self.Q, self.K, self.nmu, _dblp(self.theta_t), float(self.dt), self.nt,
                        c_vp(eng.A_diag.data_ptr()), c_vp(eng.A_cpl.data_ptr()), c_vp(self.b_K.data_ptr()), c_vp(self.phis.data_ptr()),
                        c_vp(self.work.data_ptr()), c_vp(U.data_ptr()), float(rtol), int(k), _dblp(info), ctx._stream())
        return rc, U, info

    def run(self, k, rtol=1e-14):
        rc, U, info = self.raw(k, rtol)
        pan, npan = self.panels(), (self.nmu + 15) // 16
        assert info[0] == pan[0:2 * npan:2].sum() and info[1] == pan[1::2].max(), (info, pan)
        assert all(v == pan[0] for v in pan[0:2 * npan:2]) and not pan[2 * npan:].any(), pan
        Uh = U.cpu().numpy().reshape(self.nt + 1, -1, self.nmu)
        assert np.isnan(Uh[2:]).all()                                       # no panel went past the step it missed
        return rc, Uh[1] - Uh[0], np.array([pan[0], info[1]])


@pytest.mark.parametrize('nmu', FOM_ITERATE_NMU)
def test_full_order_first_step_iterates_pin_the_coarse_level(nmu):
    shape = (3, 3)
    th = tables(nmu, 2, seed=nmu)
    c = CallTv(shape, KC, th)
    assert c.ref.has_coarse
    tag = 'fom euler batch tv {} nmu={}'.format(shape, nmu)
    cell, res = check_iterates(c.run, c.ref.iterate, tag, tol_x=TOL_X, tol_res=TOL_RES, steps=K_STEPS)
    _say(_part('fom iterates {} nmu={}'.format(shape, nmu), cell, TOL_X,
               ', worst ratio error {:.2e} (tolerance {:.0e})'.format(res, TOL_RES)),
         _miss(c.run, c.reference(coarse_theta=tv.step_mean(th, last=1)).iterate, 'a coarse level at row 1'))
    c.ctx.set_option('coarse', 0)
    try:
        check_mutant(c.run, c.ref.iterate, tag)
    finally:
        c.ctx.set_option('coarse', 1)


# -------------------------------------------------------------------------------------------------------------- 7. estimates
def _grams(N, layout, keep=None):
    """(system dict, estimator operators) of a pass at the first N of the NMAX columns (``keep``: zero-padded), per layout."""
    key = (N, layout, keep is not None)
    if key not in _EST:
        s = _system()
        eng = s['eng']
        V = _energy_bases(eng, NMAX, seed=5)[:, :, :N].copy()
        if keep is not None:
            V *= keep[:, None, :]
        buf = eng.alloc_reduce_buffers(N, factored=(layout == 'factored'))
        eng.project_and_estimate(eng.ctx.from_numpy(V), buf)
        sv = dict(s, B=buf['sys'][0].cpu().numpy(), M=buf['sys'][3].cpu().numpy(), rhs=buf['sys'][1].cpu().numpy())
        _EST[key] = (sv, tuple(g.clone() for g in buf['grams']))
    return _EST[key]


def _estimate_cell(s, grams, N, nmu, nt, what, layout='factored', src=None, keep=None, sqrt_locals=(False, True), options=()):
    """One call per ``sqrt_local`` under poisoned work against ``_estimate_reference``; -> the host results of the last call, its
    inputs and the cell's part of the test's line."""
    eng = s['eng']
    ctx = eng.ctx
    Q = s['Q']
    th, coef = tables(nmu, nt, Q, seed=N), _coef(nmu, nt)
    assert coef.size == 2 * nmu * (nt + 1)
    Uh = _panel(s, N, nmu, nt, th)
    if keep is not None:
        Uh = np.ascontiguousarray(Uh * keep[None, :, :, None])
    B, M, _, _ = _cut_of(s, N)
    kw = {} if src is None else dict(phi=src['phi'], F2=src['F2'], r_fd_K=src['r_fd_K'])
    worst = 0.0
    for sq in sqrt_locals:
        def call(sq=sq):
            return ctx.reduced_parabolic_estimate_batch_tv(th, coef, T_END / nt, nt, _dev(ctx, Uh), _dev(ctx, B), _dev(ctx, M), grams,
                                                           eng.f2, eng.ceps, eng.hdiam, sqrt_local=sq, **kw)
        for name in options:
            ctx.set_option(name, 1)
        try:
            res = _host(poisoned(ctx, call))
        finally:
            for name in options:
                ctx.set_option(name, 0)
        ref = _estimate_reference(s, N, nt, th, coef, Uh, grams, sqrt_local=sq, src=src)
        errs = {k: _err(res[k], ref[k]) for k in ref}
        if layout == 'dense':                                               # pure NumPy: this output depends on no sibling export
            ncd = nc_of_differences(grams[0].cpu().numpy(), s['nbr'], Uh)
            errs['time_deriv_nc (NumPy)'] = _err(res['time_deriv_nc'], np.sqrt(np.maximum(ncd * (nt / T_END), 0.0)))
        assert res['est'].min() > 0.0 and res['time_residual'].min() > 0.0
        for k, v in errs.items():
            assert v <= TOL_EST, (what, sq, k, v)
        worst = max(worst, max(errs.values()))
    extra = ''
    if src is not None:                                                     # the row the source terms go into, on its own
        moved = _err(ref['eta_loc'][1], _estimate_reference(s, N, nt, th, coef, Uh, grams, sqrt_local=sq)['eta_loc'][1])
        extra = ', eta_loc[1] (the residual row, which the source terms move by {:.2e}) {:.2e}'.format(
            moved, _err(res['eta_loc'][1], ref['eta_loc'][1]))
        assert moved > 1e4 * TOL_EST, moved
    return (res, (th, coef, Uh, B, M),
            _part('estimate {} {} N={} nmu={} nt={} Q={}'.format(what, layout, N, nmu, nt, Q), worst, TOL_EST, extra))


@pytest.mark.parametrize('N, nmu, nt, layout', [c + ('factored',) for c in EST_CELLS] + [c + ('dense',) for c in EST_BOTH_LAYOUTS])
def test_estimates_over_the_coefficient_uploads(N, nmu, nt, layout):
    s, grams = _grams(N, layout)
    _say(_estimate_cell(s, grams, N, nmu, nt, 'uploads', layout=layout)[2])


def _layout_of(s, N):
    """The factored layout where the fused pass runs (Q, N); the unfused kernels write the dense one."""
    return 'factored' if s['eng'].ctx.fused_supported(s['Q'], N, factored=True) else 'dense'


@pytest.mark.parametrize('Q, nmu', EST_Q_CELLS)
def test_estimates_over_the_component_counts(Q, nmu):
    s = _sys(Q_GRID, Q)
    layout = _layout_of(s, 24)
    _say(_estimate_cell(s, _grams24(s, 24, layout), 24, nmu, 3, 'components', layout=layout)[2])


def _source(s, grams, N, nmu, nt, K=3, seed=5):
    ctx, S = s['eng'].ctx, s['eng'].S
    rng = np.random.default_rng(seed)
    return dict(phi=np.ascontiguousarray(rng.uniform(0.2, 1.0, (nmu, nt + 1, K))),
                F2=_dev(ctx, np.einsum('ski,skj->sij', *(2 * (rng.standard_normal((S, 4, K)),))) + np.eye(K)),
                r_fd_K=_dev(ctx, rng.standard_normal((K, S, 5 * s['Q'] * N)) * float(grams[1].abs().max())))


def test_estimates_with_a_source_on_the_wide_panels():
    N, nmu, nt = EST_MAIN
    s, grams = _grams(N, 'factored')
    wide = _estimate_cell(s, grams, N, nmu, nt, 'K=3 source', src=_source(s, grams, N, nmu, nt), sqrt_locals=(False,))[2]
    s = _sys(Q_GRID, 4)
    layout = _layout_of(s, 24)
    grams = _grams24(s, 24, layout)
    _say(wide, _estimate_cell(s, grams, 24, 17, 3, 'K=3 source', layout=layout, src=_source(s, grams, 24, 17, 3), sqrt_locals=(False,))[2])


def test_estimates_with_zero_padded_bases():
    N, nmu, nt = EST_MAIN
    keep = _cut_of(_system(), N, ragged=True)[3]
    assert (keep == 0).any()
    s, grams = _grams(N, 'factored', keep=keep)
    res, _, part = _estimate_cell(s, grams, N, nmu, nt, 'zero-padded', keep=keep, sqrt_locals=(False,))
    _say(part)
    assert all(np.isfinite(v).all() for v in res.values())


@pytest.mark.parametrize('option', ('solve_valu', 'estimate_valu'))
def test_estimates_in_the_valu_forms(option):
    """``solve_valu``: the time residual's matvec in groups of 16 (VALU kernels).  ``estimate_valu``: the VALU form of the elliptic
    rows, which exists for the dense layout only (the factored layout always runs the matrix-core kernel), so that cell is dense.
    The reference's elliptic rows and the default call run with the option off: the matrix-core form."""
    N, nmu, nt = EST_MAIN
    layout = EST_VALU_LAYOUT[option]
    s, grams = _grams(N, layout)
    res, (th, coef, Uh, B, M), part = _estimate_cell(s, grams, N, nmu, nt, option, layout=layout, sqrt_locals=(False,), options=(option,))
    eng = s['eng']
    ctx = eng.ctx
    plain = _host(ctx.reduced_parabolic_estimate_batch_tv(th, coef, T_END / nt, nt, _dev(ctx, Uh), _dev(ctx, B), _dev(ctx, M), grams,
                                                          eng.f2, eng.ceps, eng.hdiam))
    worst = max(_err(res[k], plain[k]) for k in plain)
    _say(part, _part('against the default form', worst, TOL_EST))
    assert worst <= TOL_EST


def test_swapping_columns_of_two_blocks_swaps_their_estimates_bit_for_bit():
    N, nmu, nt = EST_CELLS[2]
    assert nmu == 49 and SWAP[0] // 16 != SWAP[1] // 16
    s, grams = _grams(N, 'factored')
    eng = s['eng']
    ctx = eng.ctx
    th, coef = tables(nmu, nt, seed=N), _coef(nmu, nt)
    Uh = _panel(s, N, nmu, nt, th)
    B, M, _, _ = _cut_of(s, N)
    perm = np.arange(nmu)
    perm[list(SWAP)] = perm[list(SWAP[::-1])]
    args = (_dev(ctx, B), _dev(ctx, M), grams, eng.f2, eng.ceps, eng.hdiam)
    x = _host(poisoned(ctx, lambda: ctx.reduced_parabolic_estimate_batch_tv(th, coef, T_END / nt, nt, _dev(ctx, Uh), *args)))
    y = _host(poisoned(ctx, lambda: ctx.reduced_parabolic_estimate_batch_tv(
        np.ascontiguousarray(th[perm]), np.ascontiguousarray(coef[perm]), T_END / nt, nt, _dev(ctx, Uh[..., perm]), *args)))
    for k in x:
        assert np.array_equal(x[k][..., perm], y[k]), k
    assert not np.array_equal(x['est'][SWAP[0]], x['est'][SWAP[1]])
    _say(_part('estimate swap of the columns {} and {} of {}'.format(SWAP[0], SWAP[1], nmu), 0.0, TOL_EST, ', bit for bit'))


# ------------------------------------------------------------------------------ 8. more than 64 parameters through Python
def test_more_than_64_parameters_through_the_reduced_model_and_the_discretization():
    from pylrbms_amd.reductor import ParabolicLRBMSReductor
    T, nt = 0.05, 4
    p, d, data = _channels(1.5 * T / nt)
    assert d._tv
    reductor = ParabolicLRBMSReductor(d, products=[d.operators['local_energy_dg_product_{}'.format(ii)]
                                                   for ii in range(data['block_space'].num_blocks)])
    reductor.extend_basis(d.solve_batch([[0.2], [0.6], [1.0]], as_snapshots=True), method='pod', pod_modes=6)
    rd = reductor.reduce()
    mus = [[float(v)] for v in np.linspace(0.2, 1.0, 67)]                   # 64 + 3: a full chunk and a short one
    us = rd.solve_batch(mus)
    ests = rd.estimate_batch(us, mus)
    assert len(us) == len(ests) == 67
    worst_u = worst_e = 0.0
    for i in (0, 63, 64, 66):
        u1 = rd.solve(mus[i]).tensor
        worst_u = max(worst_u, float((u1 - us[i].tensor).abs().max() / u1.abs().max()))
        e1 = rd.estimate(us[i], mus[i])
        assert e1[0] > 0.0 and np.isfinite(e1[0])
        worst_e = max([worst_e, abs(e1[0] - ests[i][0]) / e1[0]] + [_err(np.asarray(a), np.asarray(b)) for a, b in zip(ests[i][1], e1[1])])
    assert worst_u <= TOL_TRAJ and worst_e <= TOL_EST, (worst_u, worst_e)
    assert float((us[63].tensor - us[64].tensor).abs().max()) > 0.0         # (neighbours in the sweep, not copies)
    fom = d.solve_batch(mus[:66])
    assert len(fom) == 66
    worst_f = 0.0
    for i in (63, 64, 65):
        one = d.solve(mus[i]).tensor
        worst_f = max(worst_f, float((one - fom[i].tensor).abs().max() / one.abs().max()))
    _say(_part('67 parameters through the reduced model: trajectories', worst_u, TOL_TRAJ), _part('estimates', worst_e, TOL_EST),
         _part('66 parameters through the discretization', worst_f, TOL_TRAJ))
    assert worst_f <= TOL_TRAJ
