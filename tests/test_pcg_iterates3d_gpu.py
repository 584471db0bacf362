"""The PCG iterates of the single and stationary 3D / P2 solver exports against the NumPy PCG of tests/pcg3d_ref.py.

A converged CG solution does not depend on the preconditioner, so the parity tests cannot see a wrong inverse block, a dropped
coarse term, a coarse level built at the wrong parameter or a partial sum that skips entries.  The k-th iterate from x_0 = 0 can:
lrbms3_reduced_solve, lrbms3_reduced_solve_batch(_src), lrbms3_fom_solve and the single implicit-Euler steppers honour
``max_iter`` exactly (``red_cg``, ``red_batch_iterate``, ``fom_cg`` in pylrbms_amd/csrc/online3d.hip and lrbms3d.hip): a call with max_iter = k
returns LRBMS_E_NOT_CONVERGED, leaves x_k in the caller's array and info = (k, |r_k| / |b|).  Every cell calls the raw export
through ``ctx.lib`` with NaN-poisoned ``work`` and output for k in K_STEPS (``check_iterates`` of tests/test_pcg_iterates_gpu.py
with its TOL_X = 1e-10 and TOL_RES = 1e-8, unchanged), closes with one converged call against a direct solve, and shows for every
mutant of tests/pcg3d_ref.py that the product's x_2 misses the mutant reference by more than MUTANT_FLOOR.

The reference operators are the product's own B_sys / rhs_red / A_diag / A_cpl / M_red copied to the host (pinned to the oracle
elsewhere): the cells test the solvers alone.  The cell lists are module constants; tests/test_pcg_iterates3d_host.py mirrors the
host dispatch of online3d.hip / lrbms3d.hip and proves on the CPU that they reach every branch and that every mutant is separable.

The Euler cells compare U[1] - U[0] with the correction's iterate.  They found that a step which missed rtol returned before u_k
was added and left the bare correction in U[k + 1]; ``fom_euler_run`` and ``red_euler_run`` add u_k first now, as the batched
exports do.

Two limits of the references.  The ``nc S > 8192 -> no coarse level`` rung of ``fom_coarse`` needs 8 193 subdomains; its reference
is too slow for a GPU test, the host module checks its dispatch only.  On the 13 x 13 x 13 grid (131 820 unknowns) a sparse LU
takes a minute, so that one full-order cell closes its converged call with the true residual of the reference operator."""
import numpy as np
import pytest

import common3d as c3
import fom_batch3d_ref as ref3
import pcg3d_ref as r3
from test_pcg_iterates_gpu import K_STEPS, MIN_RATIO, MUTANT_FLOOR, TOL_RES, TOL_X, _dev, _raw, check_iterates

pytestmark = pytest.mark.gpu

E_NOT_CONVERGED = -4
MUTANT_K = 2
NAN = float('nan')
SWEEP = 'interior_3x3x3'
NMAX = 32
DT = 0.05

# A. lrbms3_reduced_solve
SINGLE_N = (1, 2, 5, 17, 32)                                       # on SWEEP
SINGLE_OTHER = (('q3_2x1x2', 6),)                                  # Q = 3
RAGGED_CELL = (SWEEP, 5, 1, 2)                                     # problem, N, subdomain, zero-padded columns
LDS_CELLS = (('q1_strip', 63), ('q1_strip', 64))                   # both sides of 64 KB of k3_block_inverse's dynamic LDS
PARTIAL_GRIDS = ((8, 8, 7), (9, 8, 7), (8, 8, 8), (10, 10, 6))     # S = 448, 504, 512, 600 at N = 2: the loops of sum_partials
REDUCE_GRID = (13, 13, 13)                                         # S = 2 197 at N = 2: the unrolled body of k3_reduce1
GRID_N = 2
# B. lrbms3_reduced_solve_batch on SWEEP: (N, nmu), each with and without an installed preconditioner built at BUILD_MU
BATCH_CELLS = ((5, 1), (16, 16), (17, 17), (32, 33), (5, 64))
BUILD_MU = 2.5
VALU_CELL = (17, 17)
SRC_CELL = (5, 20, 3, 7)                                           # N, nmu, K, the all-zero column
BIG_INSTALLED = ((10, 10, 6), GRID_N, 5)                           # S = 600: the last workgroup of k3b_coarse_apply has 8 rows
# C. lrbms3_fom_solve: (problem, coarse space)
FOM_CELLS = ((SWEEP, 'p1'), (SWEEP, 'constants'), (SWEEP, 'off'), (SWEEP, 'deficient'), ('kc_3x1x2', 'p1'), ('q3_2x1x2', 'p1'))
KEPT_CELL = (SWEEP, 0.2)                                           # the kept inverse is built at theta(0.2)
CAP_GRID = (13, 13, 13)                                            # 4 S > 8192: constants instead of P1
# D. first Euler step
EULER_PROBLEMS = ('aniso_2x2x1', SWEEP)

_ENGINES, _SYSTEMS, _FOM = {}, {}, {}
WORST = {}


def grid_spec(shape):
    """A problem of ``common3d.make_problem(spec=...)`` on ``shape`` subdomains of one cube each (k_c = 1: 60 DoFs)."""
    return (list(shape), 1, [c3._one, c3._lam1], [lambda mu: 1.0, lambda mu: mu], np.eye(3), GRID_N, 0.5)


def _engine(name):
    """(problem, assembled engine) of a named problem of ``common3d.PROBLEMS`` or of a grid shape, kept per name."""
    if name not in _ENGINES:
        p = c3.make_problem(name) if isinstance(name, str) else c3.make_problem('grid_' + 'x'.join(map(str, name)), spec=grid_spec(name))
        _ENGINES[name] = (p, c3.engine_of(p).assemble())
    return _ENGINES[name]


def _system(name, N, pad=None, mass=False):
    """Host copies of the product's reduced system at N columns of ``make_bases3d``: B [Q, S, 7, N, N], rhs [S, N], keep [S, N]
    (0 on the zero-padded columns of ``pad`` = (subdomain, count)) and, with ``mass``, M [S, N, N] of lrbms3_project_mass."""
    key = (name, N, pad, mass)
    if key not in _SYSTEMS:
        p, eng = _engine(name)
        V = c3.make_bases3d(eng.S, eng.t.n, N, seed=3)
        keep = np.ones((eng.S, N))
        if pad is not None:
            V[pad[0], :, N - pad[1]:] = 0.0
            keep[pad[0], N - pad[1]:] = 0.0
        Vd = eng.ctx.from_numpy(V)
        out = eng.project_and_estimate(Vd)
        s = dict(p=p, eng=eng, nbr=np.asarray(eng.nbr).reshape(eng.S, 7), Q=len(p['lambdas']), keep=keep,
                 B=out['B_sys'].cpu().numpy().copy(), rhs=out['rhs_red'].cpu().numpy().copy())
        if mass:
            s['M'] = eng.ctx.project_mass(Vd).cpu().numpy().copy()
        _SYSTEMS[key] = s
    return _SYSTEMS[key]


def _cut(s, N):
    return np.ascontiguousarray(s['B'][..., :N, :N]), np.ascontiguousarray(s['rhs'][:, :N])


def _poisoned(ctx, *shape):
    t = ctx.empty(*shape)
    t.fill_(NAN)
    return t


def _note(family, cell, res):
    a, b = WORST.get(family, (0.0, 0.0))
    WORST[family] = (max(a, cell), max(b, res))
    print('PCG-ITERATES-3D family {}: worst x_k error so far {:.2e}, worst ratio error {:.2e}'.format(family, *WORST[family]))


def _check(family, run, cell, tag, every_k=False):
    if every_k:                                       # decided by the reference alone: no k of K_STEPS is skipped
        for k in K_STEPS:
            assert cell.iterate(k)[1].min() >= MIN_RATIO, (tag, k)
    _note(family, *check_iterates(run, cell.iterate, tag, tol_x=TOL_X, tol_res=TOL_RES, steps=K_STEPS))


def _mutant(X, mutant, tag, what):
    """The product's x_2 against a mutant reference: must miss."""
    X_ref, ratios = mutant.iterate(MUTANT_K)
    err = r3.miss(X, X_ref)
    print('PCG-ITERATES-3D {}: misses {} by {:.2e} ({:.1e} x the tolerance)'.format(tag, what, err, err / TOL_X))
    assert err > MUTANT_FLOOR, (tag, what, err)


def _x2(run, cell, tag):
    """The product's x_2, checked to be a k the cell keeps."""
    X_ref, ratios = cell.iterate(MUTANT_K)
    assert ratios[np.linalg.norm(X_ref, axis=0) > 0.0].min() >= MIN_RATIO, tag          # (a zero column has no ratio)
    rc, X, info = run(MUTANT_K)
    assert rc == E_NOT_CONVERGED and int(info[0]) == MUTANT_K, (tag, rc, info)
    return X


# ------------------------------------------------------------------------------------------------- A. lrbms3_reduced_solve
def _single(s, N, theta, B=None, rhs=None, keep=None):
    from pylrbms_amd._native import _dblp, c_vp
    eng = s['eng']
    ctx, S, Q = eng.ctx, eng.S, s['Q']
    if B is None:
        B, rhs = _cut(s, N)
    th = np.ascontiguousarray(theta, dtype=np.float64)
    cell = r3.reduced_single(B, s['nbr'], th, rhs, keep=keep)
    Bd, rd = _dev(ctx, B), _dev(ctx, rhs)
    work = ctx.empty(int(ctx.lib.lrbms3_reduced_solve_work_size(ctx.handle, N)))

    def run(k, rtol=1e-14):
        work.fill_(NAN)
        u = _poisoned(ctx, S, N)
        info = np.zeros(2)
        rc = _raw(ctx, 'lrbms3_reduced_solve', Q, N, _dblp(th), c_vp(Bd.data_ptr()), c_vp(rd.data_ptr()), c_vp(work.data_ptr()),
                  c_vp(u.data_ptr()), float(rtol), int(k), _dblp(info), ctx._stream())
        return rc, u.cpu().numpy().reshape(-1, 1), info

    def converged():
        rc, u, info = run(20000, rtol=1e-13)
        assert rc == 0 and info[1] <= 1e-13, (rc, info)
        ref = cell.solve()
        assert np.linalg.norm(u[:, 0] - ref) < 1e-10 * np.linalg.norm(ref)
        return u
    return run, cell, converged


def _single_cell(name, N, sysN=None, theta=None, family='single reduced'):
    s = _system(name, sysN or N)
    th = c3.theta_of(s['p'], s['p']['mu']) if theta is None else theta
    tag = 'single 3D {} S={} N={}'.format(name, s['eng'].S, N)
    run, cell, converged = _single(s, N, th)
    _check(family, run, cell, tag)
    converged()
    return s, run, cell, tag


@pytest.mark.parametrize('N', SINGLE_N)
def test_single_solve_iterates_over_basis_sizes(N):
    s, run, cell, tag = _single_cell(SWEEP, N, sysN=NMAX)
    if s['Q'] > 1:                                    # the inverse blocks are those of the solve's own theta
        B, rhs = _cut(s, N)
        other = r3.reduced_single(B, s['nbr'], c3.theta_of(s['p'], s['p']['mu']), rhs, block_theta=c3.theta_of(s['p'], BUILD_MU))
        _mutant(_x2(run, cell, tag), other, tag, 'inverse blocks at another theta')


@pytest.mark.parametrize('name, N', SINGLE_OTHER + LDS_CELLS)
def test_single_solve_iterates_on_other_problems(name, N):
    _single_cell(name, N, sysN=64 if (name, N) in LDS_CELLS else None)


def test_single_solve_iterates_with_a_zero_padded_ragged_basis():
    name, N, sub, count = RAGGED_CELL
    s = _system(name, N, pad=(sub, count))
    keep = s['keep']
    assert (keep == 0).sum() == count and not s['B'][:, sub, 3, N - 1].any() and not s['rhs'][sub, N - count:].any()
    run, cell, converged = _single(s, N, c3.theta_of(s['p'], s['p']['mu']), B=s['B'], rhs=s['rhs'], keep=keep)
    _check('single reduced', run, cell, 'single 3D ragged')
    for k in K_STEPS:
        _, u, _ = run(k)
        assert np.all(u.reshape(keep.shape)[keep == 0] == 0.0), k      # the padded unknowns stay exactly 0 in every iterate
    u = converged()
    assert np.all(u.reshape(keep.shape)[keep == 0] == 0.0)


@pytest.mark.parametrize('shape', PARTIAL_GRIDS + (REDUCE_GRID,))
def test_single_solve_iterates_over_the_partial_sum_loops(shape):
    """sum_partials (64 threads, 8 x 64 unrolled) at S = 448 (tail alone), 504 (56 threads in the body, 8 in the tail), 512 (body
    alone) and 600 (body then tail); k3_reduce1 (256 threads, 8 x 256 unrolled) at S = 2 197 (body then tail).  A skipped or
    doubled partial moves alpha or beta, hence x_k."""
    s, _, _, _ = _single_cell(shape, GRID_N, family='single reduced, large S')
    assert s['eng'].S == int(np.prod(shape))


# ------------------------------------------------------------------------------------------- B. lrbms3_reduced_solve_batch
def _mus(nmu):
    return np.linspace(0.1, 1.0, nmu) if nmu > 1 else np.array([0.1])


def _batch(s, N, nmu, build_theta=None, K=0, zero_col=None, seed=0):
    from pylrbms_amd._native import _dblp, c_vp
    eng = s['eng']
    ctx, S, Q = eng.ctx, eng.S, s['Q']
    B, rhs = _cut(s, N)
    thetas = np.ascontiguousarray(np.stack([c3.theta_of(s['p'], mu) for mu in _mus(nmu)]))
    if K == 0:
        cols = np.repeat(rhs.reshape(-1, 1), nmu, axis=1)
    else:
        rng = np.random.default_rng(seed)
        rhs = np.ascontiguousarray(rng.standard_normal((K, S, N)) * np.abs(rhs).max())
        phi = rng.uniform(0.2, 1.0, (nmu, K))
        if zero_col is not None:
            phi[zero_col] = 0.0
        phi = np.ascontiguousarray(phi)
        cols = np.einsum('mk,kn->nm', phi, rhs.reshape(K, -1))
    cell = r3.reduced_batch(B, s['nbr'], thetas, cols, build_theta=build_theta)
    Bd, rd = _dev(ctx, B), _dev(ctx, rhs)
    work = ctx.empty(int(ctx.lib.lrbms3_reduced_solve_batch_work_size(ctx.handle, N, nmu)))

    def run(k, rtol=1e-14):
        work.fill_(NAN)
        u = _poisoned(ctx, S, N, nmu)
        info = np.zeros(2)
        if K == 0:
            rc = _raw(ctx, 'lrbms3_reduced_solve_batch', Q, N, nmu, _dblp(thetas), c_vp(Bd.data_ptr()), c_vp(rd.data_ptr()),
                      c_vp(work.data_ptr()), c_vp(u.data_ptr()), float(rtol), int(k), _dblp(info), ctx._stream())
        else:
            rc = _raw(ctx, 'lrbms3_reduced_solve_batch_src', Q, N, K, nmu, _dblp(thetas), _dblp(phi), c_vp(Bd.data_ptr()),
                      c_vp(rd.data_ptr()), c_vp(work.data_ptr()), c_vp(u.data_ptr()), float(rtol), int(k), _dblp(info),
                      ctx._stream())
        return rc, u.cpu().numpy().reshape(-1, nmu), info

    def converged():
        rc, u, info = run(20000, rtol=1e-13)
        assert rc == 0 and info[1] <= 1e-13, (rc, info)
        for j in sorted({0, nmu // 2, nmu - 1}):
            if cols[:, j].any():
                ref = cell.solve(j)
                assert np.linalg.norm(u[:, j] - ref) < 1e-10 * np.linalg.norm(ref), j
        return u

    def mutant(**kw):
        return r3.reduced_batch(B, s['nbr'], thetas, cols, build_theta=build_theta, **kw)
    return run, cell, converged, mutant, (Bd, thetas)


class _Installed:
    """lrbms3_reduced_precond_build at ``theta`` + _use for the block; _use(NULL) behind it."""

    def __init__(self, s, N, theta):
        self.ctx, self.args = s['eng'].ctx, (s['Q'], np.ascontiguousarray(theta, dtype=np.float64), _dev(s['eng'].ctx, _cut(s, N)[0]))

    def __enter__(self):
        self.ctx.reduced_precond_use(self.ctx.reduced_precond_build(*self.args))

    def __exit__(self, *exc):
        self.ctx.reduced_precond_use(None)


def _batch_mutants(run, cell, mutant, nmu, installed, tag):
    X = _x2(run, cell, tag)
    if installed:
        _mutant(X, mutant(coarse=None), tag, 'no coarse level')
        _mutant(X, mutant(coarse='own'), tag, 'the coarse level at the column\'s own theta')
        _mutant(X, mutant(blocks='group'), tag, 'inverse blocks at the group mean instead of the build parameter')
    else:
        if nmu > 1:
            _mutant(X, mutant(blocks='own'), tag, 'inverse blocks at the column\'s own theta')
        if nmu > r3.GROUP:
            _mutant(X, mutant(blocks='call'), tag, 'inverse blocks at the call mean instead of the group mean')


@pytest.mark.parametrize('installed', (False, True))
@pytest.mark.parametrize('N, nmu', BATCH_CELLS)
def test_batched_solve_iterates(N, nmu, installed):
    s = _system(SWEEP, NMAX)
    th_b = c3.theta_of(s['p'], BUILD_MU)
    tag = 'batch 3D N={} nmu={} {}'.format(N, nmu, 'installed' if installed else 'group mean')
    if installed:
        with _Installed(s, N, th_b):
            run, cell, converged, mutant, _ = _batch(s, N, nmu, build_theta=th_b)
            _check('batch reduced, installed', run, cell, tag)
            converged()
            _batch_mutants(run, cell, mutant, nmu, True, tag)
    else:
        run, cell, converged, mutant, _ = _batch(s, N, nmu)
        _check('batch reduced, group mean', run, cell, tag)
        converged()
        _batch_mutants(run, cell, mutant, nmu, False, tag)


@pytest.mark.parametrize('installed', (False, True))
def test_batched_solve_iterates_valu_form(installed):
    N, nmu = VALU_CELL
    s = _system(SWEEP, NMAX)
    ctx = s['eng'].ctx
    th_b = c3.theta_of(s['p'], BUILD_MU)
    tag = 'batch 3D VALU N={} nmu={} {}'.format(N, nmu, 'installed' if installed else 'group mean')
    ctx.set_option('solve_valu', 1)
    try:
        if installed:
            with _Installed(s, N, th_b):
                run, cell, converged, mutant, _ = _batch(s, N, nmu, build_theta=th_b)
                _check('batch reduced, VALU', run, cell, tag)
                converged()
                _batch_mutants(run, cell, mutant, nmu, True, tag)
        else:
            run, cell, converged, mutant, _ = _batch(s, N, nmu)
            _check('batch reduced, VALU', run, cell, tag)
            converged()
            _batch_mutants(run, cell, mutant, nmu, False, tag)
    finally:
        ctx.set_option('solve_valu', 0)


def test_batched_source_solve_iterates_and_the_zero_column():
    N, nmu, K, zero = SRC_CELL
    s = _system(SWEEP, NMAX)
    run, cell, converged, mutant, _ = _batch(s, N, nmu, K=K, zero_col=zero)
    assert not cell.cols[:, zero].any() and cell.cols[:, zero + 1].any()
    tag = 'batch 3D src N={} nmu={} K={}'.format(N, nmu, K)
    _check('batch reduced, group mean', run, cell, tag)
    for k in K_STEPS:
        _, u, _ = run(k)
        assert not u[:, zero].any(), k                                 # exact zeros in every iterate
    u = converged()
    assert not u[:, zero].any()
    _batch_mutants(run, cell, mutant, nmu, False, tag)


def test_batched_solve_iterates_with_an_installed_preconditioner_on_600_subdomains():
    shape, N, nmu = BIG_INSTALLED
    s = _system(shape, N)
    assert s['eng'].S == 600 and s['eng'].S % 16 == 8
    th_b = c3.theta_of(s['p'], BUILD_MU)
    tag = 'batch 3D S=600 N={} nmu={} installed'.format(N, nmu)
    with _Installed(s, N, th_b):
        run, cell, converged, mutant, _ = _batch(s, N, nmu, build_theta=th_b)
        _check('batch reduced, installed', run, cell, tag)
        converged()
        _batch_mutants(run, cell, mutant, nmu, True, tag)


def test_removing_the_installed_preconditioner_restores_the_bits():
    N, nmu = 17, 17
    s = _system(SWEEP, NMAX)
    run, cell, _, _, _ = _batch(s, N, nmu)
    _, before, info_b = run(3)
    with _Installed(s, N, c3.theta_of(s['p'], BUILD_MU)):
        _, during, _ = run(3)
    _, after, info_a = run(3)
    assert np.isfinite(before).all() and np.array_equal(before, after) and np.array_equal(info_b, info_a)
    assert r3.miss(during, before) > MUTANT_FLOOR                      # the installed one was in use in between


# ----------------------------------------------------------------------------------------------------- C. lrbms3_fom_solve
def _phi_of(t, space):
    return {'p1': ref3.default_phi(t), 'constants': np.ones((t.n, 1)), 'off': ref3.default_phi(t), 'deficient': np.zeros((t.n, 2))}[space]


class _Space:
    """The coarse space of a cell in the context; the default of mesh upload behind the block."""

    def __init__(self, eng, space):
        self.ctx, self.t, self.space = eng.ctx, eng.t, space

    def __enter__(self):
        if self.space == 'off':
            self.ctx.set_option('fom_coarse', 0)
        elif self.space != 'p1':
            self.ctx.fom_coarse_space(_phi_of(self.t, self.space))

    def __exit__(self, *exc):
        self.ctx.set_option('fom_coarse', 1)
        self.ctx.fom_coarse_space(ref3.default_phi(self.t))


def _fom(name):
    """(problem, engine, host operators) of a full-order cell; the component operators are kept with the engine."""
    p, eng = _engine(name)
    if name not in _FOM:
        _FOM[name] = (ref3.component_operators(eng.ops['A_diag'].cpu().numpy(), eng.ops['A_cpl'].cpu().numpy(), eng.t, eng.nbr),
                      eng.ops['b'].cpu().numpy().copy())
    return (p, eng) + _FOM[name]


def _fom_run(eng, theta):
    from pylrbms_amd._native import _dblp, c_vp
    ctx, ops = eng.ctx, eng.ops
    th = np.ascontiguousarray(theta, dtype=np.float64)
    work = ctx.empty(int(ctx.lib.lrbms3_fom_solve_work_size(ctx.handle)))

    def run(k, rtol=1e-14):
        work.fill_(NAN)
        x = _poisoned(ctx, eng.S, eng.t.n)
        info = np.zeros(2)
        rc = _raw(ctx, 'lrbms3_fom_solve', th.size, _dblp(th), c_vp(ops['A_diag'].data_ptr()), c_vp(ops['A_cpl'].data_ptr()),
                  c_vp(ops['b'].data_ptr()), c_vp(work.data_ptr()), c_vp(x.data_ptr()), float(rtol), int(k), _dblp(info), ctx._stream())
        return rc, x.cpu().numpy().reshape(-1, 1), info
    return run


def _fom_converged(run, cell, direct=True):
    rc, x, info = run(100000, rtol=1e-12)
    assert rc == 0 and info[1] <= 1e-12, (rc, info)
    if direct:
        ref = cell.solve()
        assert np.abs(x[:, 0] - ref).max() < 1e-8 * np.abs(ref).max()
    else:
        b = cell.cols[:, 0]
        assert np.linalg.norm(cell.As[0] @ x[:, 0] - b) < 1e-10 * np.linalg.norm(b)


@pytest.mark.parametrize('name, space', FOM_CELLS)
def test_fom_solve_iterates(name, space):
    p, eng, Aq, b = _fom(name)
    S, n = eng.S, eng.t.n
    th = c3.theta_of(p, p['mu'])
    tag = 'fom 3D {} space={}'.format(name, space)
    two_level = space in ('p1', 'constants')
    cell = r3.fom_single(Aq, S, n, _phi_of(eng.t, space), th, b, coarse=0 if space == 'off' else 1)
    assert cell.precond.has_coarse == two_level, tag
    run = _fom_run(eng, th)
    with _Space(eng, space):
        _check('single full order', run, cell, tag, every_k=True)
        _fom_converged(run, cell)
        X = _x2(run, cell, tag)
    if two_level:
        _mutant(X, r3.fom_single(Aq, S, n, None, th, b), tag, 'no coarse level')
        _mutant(X, r3.fom_single(Aq, S, n, _phi_of(eng.t, space), th, b, coarse_theta=c3.theta_of(p, BUILD_MU)), tag,
                'the coarse level at another theta')
        other = {'p1': 'constants', 'constants': 'p1'}[space]
        _mutant(X, r3.fom_single(Aq, S, n, _phi_of(eng.t, other), th, b), tag, 'the coarse space ' + other)
    else:                                             # 'off' and the rank-deficient space: the element blocks alone
        blocks = r3.fom_single(Aq, S, n, None, th, b)
        assert r3.miss(X, blocks.iterate(MUTANT_K)[0]) < TOL_X, tag
        _mutant(X, r3.fom_single(Aq, S, n, ref3.default_phi(eng.t), th, b), tag, 'the P1 coarse level')


def test_fom_solve_iterates_with_the_kept_coarse_inverse():
    name, mu_keep = KEPT_CELL
    p, eng, Aq, b = _fom(name)
    S, n, ctx = eng.S, eng.t.n, eng.ctx
    th, th_keep = c3.theta_of(p, p['mu']), c3.theta_of(p, mu_keep)
    Phi = ref3.default_phi(eng.t)
    cell = r3.fom_single(Aq, S, n, Phi, th, b, coarse_theta=th_keep)
    run, build = _fom_run(eng, th), _fom_run(eng, th_keep)
    tag = 'fom 3D {} kept inverse of theta({})'.format(name, mu_keep)
    ctx.fom_precond_keep(True)
    try:
        rc, _, info = build(1)                                         # builds and keeps the coarse inverse at theta(mu_keep)
        assert rc == E_NOT_CONVERGED and info[0] == 1
        _check('single full order', run, cell, tag, every_k=True)
        _fom_converged(run, cell)
        X = _x2(run, cell, tag)
    finally:
        ctx.fom_precond_keep(False)
    _mutant(X, r3.fom_single(Aq, S, n, Phi, th, b), tag, 'the coarse level at the solve\'s own theta')
    own = r3.fom_single(Aq, S, n, Phi, th, b)                          # and after keep = 0 every solve builds its own again
    assert r3.miss(_x2(run, own, tag), own.iterate(MUTANT_K)[0]) < TOL_X


def test_fom_solve_iterates_beyond_the_coarse_cap():
    """13 x 13 x 13 subdomains: 4 S = 8 788 > 8 192, ``fom_coarse`` falls back to the constants; the reference takes the same ladder
    (``BatchFomPrecond3D``), the P1 mutant (its coarse problem solved sparse) must miss.  lrbms3_fom_solve_batch shares
    ``fom_coarse``.  The partial sums of ``fom_cg`` (k3_reduce1 over 2 197 and 4 394 entries) go through body and tail."""
    p, eng, Aq, b = _fom(CAP_GRID)
    S, n = eng.S, eng.t.n
    assert 4 * S > ref3.COARSE_MAX >= S
    th = c3.theta_of(p, p['mu'])
    Phi = ref3.default_phi(eng.t)
    cell = r3.fom_single(Aq, S, n, Phi, th, b)
    assert cell.precond.has_coarse and cell.precond.A1.shape == (S, S)
    run = _fom_run(eng, th)
    tag = 'fom 3D S={} capped'.format(S)
    _check('single full order, capped', run, cell, tag, every_k=True)
    _fom_converged(run, cell, direct=False)
    X = _x2(run, cell, tag)
    _mutant(X, r3.fom_single(Aq, S, n, Phi, th, b, capped=False), tag, 'the P1 coarse level')
    _mutant(X, r3.fom_single(Aq, S, n, None, th, b), tag, 'no coarse level')


# ------------------------------------------------------------------------------------------------- D. the first Euler step
def _u0(scale, shape, seed=11):
    return np.ascontiguousarray(np.random.default_rng(seed).standard_normal(shape) * scale)


def _euler_run(ctx, export, head, tail, S, width, u0):
    """run(k) of one step (nt = 1) from u0: -> (rc, U[1] - U[0] as a column, info); ``head`` / ``tail``: the arguments around dt, nt."""
    from pylrbms_amd._native import _dblp, c_vp
    work = ctx.empty(int(getattr(ctx.lib, export + '_work_size')(ctx.handle, *([width] if 'reduced' in export else []))))
    u0d = _dev(ctx, u0)

    def run(k, rtol=1e-14):
        work.fill_(NAN)
        U = _poisoned(ctx, 2, S, width)
        U[0] = u0d
        info = np.zeros(2)
        rc = _raw(ctx, export, *head, DT, 1, *tail, c_vp(work.data_ptr()), c_vp(U.data_ptr()), float(rtol), int(k), _dblp(info),
                  ctx._stream())
        Uh = U.cpu().numpy().reshape(2, -1)
        assert np.array_equal(Uh[0], u0.ravel())
        return rc, (Uh[1] - Uh[0]).reshape(-1, 1), info
    return run


@pytest.mark.parametrize('name', EULER_PROBLEMS)
def test_first_reduced_euler_step_iterates(name):
    from pylrbms_amd._native import _dblp, c_vp
    N = c3.PROBLEMS[name][5]
    s = _system(name, N, mass=True)
    eng = s['eng']
    ctx, S, Q = eng.ctx, eng.S, s['Q']
    th = np.ascontiguousarray(c3.theta_of(s['p'], s['p']['mu']))
    B, rhs, M = s['B'], s['rhs'], s['M']
    u0 = _u0(np.abs(r3.reduced_single(B, s['nbr'], th, rhs).solve()).max(), (S, N))
    cell = r3.reduced_euler_step(B, M, s['nbr'], th, DT, rhs, u0)
    Bd, Md, rd = _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs)
    run = _euler_run(ctx, 'lrbms3_reduced_implicit_euler', (Q, N, _dblp(th)),
                     (c_vp(Bd.data_ptr()), c_vp(Md.data_ptr()), c_vp(rd.data_ptr())), S, N, u0)
    tag = 'euler 3D reduced {} N={}'.format(name, N)
    _check('first Euler step', run, cell, tag)
    rc, d, info = run(20000, rtol=1e-13)
    assert rc == 0 and info[1] <= 1e-13, (rc, info)
    ref = cell.solve()
    assert np.linalg.norm(d[:, 0] - ref) < 1e-10 * np.linalg.norm(u0.ravel() + ref)
    _mutant(_x2(run, cell, tag), r3.reduced_euler_step(B, M, s['nbr'], th, DT, rhs, u0, mass_in_blocks=False), tag,
            'inverse blocks without the mass')


@pytest.mark.parametrize('name', EULER_PROBLEMS)
def test_first_fom_euler_step_iterates(name):
    from pylrbms_amd._native import _dblp, c_vp
    p, eng, Aq, b = _fom(name)
    ctx, S, n, ops = eng.ctx, eng.S, eng.t.n, eng.ops
    th = np.ascontiguousarray(c3.theta_of(p, p['mu']))
    mass = r3.oracle_mass(c3.oracle_of(p))
    Phi = ref3.default_phi(eng.t)
    u0 = _u0(np.abs(r3.fom_single(Aq, S, n, None, th, b).solve()).max(), (S, n))
    cell = r3.fom_euler_step(Aq, mass, S, n, Phi, th, DT, b, u0)
    assert cell.precond.has_coarse
    run = _euler_run(ctx, 'lrbms3_fom_implicit_euler', (th.size, _dblp(th)),
                     (c_vp(ops['A_diag'].data_ptr()), c_vp(ops['A_cpl'].data_ptr()), c_vp(ops['b'].data_ptr())), S, n, u0)
    tag = 'euler 3D full order {}'.format(name)
    _check('first Euler step', run, cell, tag)
    rc, d, info = run(100000, rtol=1e-12)
    assert rc == 0 and info[1] <= 1e-12, (rc, info)
    ref = cell.solve()
    assert np.abs(d[:, 0] - ref).max() < 1e-8 * np.abs(u0.ravel() + ref).max()
    X = _x2(run, cell, tag)
    _mutant(X, r3.fom_euler_step(Aq, mass, S, n, Phi, th, DT, b, u0, mass_in_blocks=False), tag, 'element blocks without the mass')
    _mutant(X, r3.fom_euler_step(Aq, mass, S, n, Phi, th, DT, b, u0, coarse=0), tag, 'no coarse level')
