"""Time-dependent diffusion coefficients on the GPU: lrbms_fom_implicit_euler_batch_tv,
lrbms_reduced_implicit_euler_batch_tv and lrbms_reduced_parabolic_estimate_batch_tv against the dense stepping and the estimator
restatement of tests/parabolic_tv_ref.py (pinned on the CPU in tests/test_parabolic_tv_host.py), against the existing exports for
tables that are constant in time, under poisoned work, and end to end through the discretization.

Shapes: 2 x 2 and 3 x 3 subdomains at k_c = 2 (n = 96; the 3 x 3 grid has one subdomain with all five slots), N <= 24, nt <= 3."""
import numpy as np
import pytest

import parabolic_tv_ref as tv
from fom_euler_batch_ref import component_operators, p1_mass
from parabolic_batch_ref import column_errors
from test_parabolic_batch_gpu import TOL_TRAJ
from test_parabolic_estimate_batch_gpu import TOL as TOL_EST
from test_pcg_iterates_gpu import KC, _dev, _energy_bases, _model, _raw
from test_work_poison_gpu import poisoned

pytestmark = pytest.mark.gpu

NB = 24                     # widest basis of the cells
T_END = 0.05
GRIDS = ((2, 2), (3, 3))
_SYS = {}


def _sys(shape, Q=2):
    """Engine, neighbour table and the reduced system (host) of one pass at NB energy-orthonormal columns, per (grid, Q)."""
    key = (shape, Q)
    if key not in _SYS:
        m = _model(shape, 0, Q=Q, kc=KC)
        eng = m['eng']
        buf = eng.project_and_estimate(eng.ctx.from_numpy(_energy_bases(eng, NB, seed=5)))
        _SYS[key] = dict(eng=eng, nbr=m['nbr'], Q=m['Q'], B=buf['sys'][0].cpu().numpy(), rhs=buf['sys'][1].cpu().numpy(),
                         M=buf['sys'][3].cpu().numpy(), grams=tuple(g.clone() for g in buf['grams']))
    return _SYS[key]


def _cut(s, N, ragged=False):
    """B, M, rhs of the first N columns; ragged: zero rows and columns behind sizes[s] (zero-padded bases) and the 0 / 1 mask."""
    B, M, rhs = s['B'][..., :N, :N].copy(), s['M'][:, :N, :N].copy(), s['rhs'][:, :N].copy()
    keep = None
    if ragged:
        S = s['eng'].S
        sizes = np.random.default_rng(3).integers(max(1, N - 5), N + 1, size=S)
        sizes[0], sizes[-1] = N, max(1, N - 3)
        keep = (np.arange(N)[None, :] < sizes[:, None]).astype(np.float64)
        nb = np.where(s['nbr'] >= 0, s['nbr'], 0)
        B *= keep[None, :, None, :, None] * keep[nb][None, :, :, None, :]
        M *= keep[:, :, None] * keep[:, None, :]
        rhs *= keep
    return np.ascontiguousarray(B), np.ascontiguousarray(M), np.ascontiguousarray(rhs), keep


def _tables(nmu, nt, Q, seed=0):
    """nt >= 2: the smooth factor times the switch; nt = 1: raw random positive tables (a table that is periodic in T cannot see an
    off-by-one row there)."""
    if nt == 1:
        th = np.random.default_rng(seed).uniform(0.15, 1.0, (nmu, 2, Q))
        if Q == 2:
            th[:, :, 0] = 1.0
        return np.ascontiguousarray(th)
    return tv.switch_table(nmu, nt, Q, T_END, t_star=1.4 * T_END / nt, seed=seed)


def _sources(s, N, nmu, nt, K, rhs, seed=1):
    rng = np.random.default_rng(seed)
    rhs_K = np.ascontiguousarray(rng.standard_normal((K, s['eng'].S, N)) * np.abs(rhs).max())
    rhs_K[0] = rhs
    return rhs_K, np.ascontiguousarray(rng.uniform(0.2, 1.0, (nmu, nt + 1, K)))


# ------------------------------------------------------------------------------------------------- 1. reduced trajectories
def _reduced_cell(shape, N, nmu, nt, Q=2, K=0, ragged=False):
    s = _sys(shape, Q)
    ctx = s['eng'].ctx
    B, M, rhs, keep = _cut(s, N, ragged)
    th = _tables(nmu, nt, s['Q'], seed=N + nmu)
    dt = T_END / nt
    if K:
        rhs_K, phis = _sources(s, N, nmu, nt, K, rhs)
        if keep is not None:
            rhs_K *= keep
        U, info = ctx.reduced_implicit_euler_batch_tv(th, dt, nt, _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs_K), phi=phis)
        ref = tv.dense_euler_batch_tv(B, M, s['nbr'], th, dt, nt, rhs_K=rhs_K, phis=phis, keep=keep)
    else:
        U, info = ctx.reduced_implicit_euler_batch_tv(th, dt, nt, _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs))
        ref = tv.dense_euler_batch_tv(B, M, s['nbr'], th, dt, nt, rhs=rhs, keep=keep)
    Uh = U.cpu().numpy()
    assert Uh.shape == (nt + 1, s['eng'].S, N, nmu)
    err = column_errors(Uh, ref)
    print('PARABOLIC-TV reduced {} N={} nmu={} nt={} Q={} K={} ragged={}: {} iterations, worst column error {:.2e} (tolerance {:.0e})'
          .format(shape, N, nmu, nt, s['Q'], K, ragged, info['iterations'], float(err.max()), TOL_TRAJ))
    assert info['relative_residual'] <= 1e-13 and info['iterations'] >= nt
    assert np.isfinite(err).all() and err.max() < TOL_TRAJ, float(err.max())
    if keep is not None:
        assert (keep == 0).any() and np.all(Uh[:, keep == 0, :] == 0.0)       # the padding stays exactly 0
    return Uh, ref


@pytest.mark.parametrize('nt', (1, 3))
@pytest.mark.parametrize('nmu', (1, 3, 17, 33))
@pytest.mark.parametrize('N', (5, 17, 24))
def test_reduced_trajectories_against_dense_stepping(N, nmu, nt):
    """Group widths 16 / 32 / 64 with partial groups; K = 3 sources on the cells with 3 and 33 columns, ragged zero-padded bases
    at N = 17; the grids alternate."""
    _reduced_cell(GRIDS[(N + nmu + nt) % 2 if N != 24 else 1], N, nmu, nt, K=3 if nmu in (3, 33) else 0, ragged=(N == 17))


@pytest.mark.parametrize('nt', (1, 3))
@pytest.mark.parametrize('nmu', (1, 3, 16))
@pytest.mark.parametrize('N', (5, 17, 24))
def test_reduced_trajectories_with_five_components(N, nmu, nt):
    _reduced_cell((3, 3), N, nmu, nt, Q=5, K=3 if nmu == 3 else 0)


def test_a_wrong_row_is_seen_by_the_trajectory_check():
    """The check above has teeth on the device too: the same call with the table shifted by one row (row k for the step k -> k + 1)
    misses the reference by far more than TOL_TRAJ."""
    shape, N, nmu, nt = (3, 3), 17, 17, 3
    s = _sys(shape)
    ctx = s['eng'].ctx
    B, M, rhs, _ = _cut(s, N)
    th = _tables(nmu, nt, 2, seed=4)
    shifted = np.ascontiguousarray(np.concatenate([th[:, :1], th[:, :-1]], axis=1))
    U, _ = ctx.reduced_implicit_euler_batch_tv(shifted, T_END / nt, nt, _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs))
    ref = tv.dense_euler_batch_tv(B, M, s['nbr'], th, T_END / nt, nt, rhs=rhs)
    assert column_errors(U.cpu().numpy(), ref).max() > 1e3 * TOL_TRAJ


# ---------------------------------------------------------------------------------------------- 2. full-order trajectories
def _fom_cell(shape, nmu, nt, K=1, const=False, seed=0):
    s = _sys(shape)
    eng = s['eng']
    ctx, S, n = eng.ctx, eng.S, eng.t.n
    th = _tables(nmu, nt, 2, seed=seed + nmu)
    if const:
        th = np.ascontiguousarray(np.repeat(th[:, 1:2], nt + 1, axis=1))
    rng = np.random.default_rng(seed)
    b = eng.b.reshape(1, S, n)
    if K > 1:
        b_K = ctx.from_numpy(np.concatenate([b.cpu().numpy(), rng.standard_normal((K - 1, S, n)) * float(b.abs().max())]))
        phis = np.ascontiguousarray(rng.uniform(0.2, 1.0, (nmu, nt + 1, K)))
    else:
        b_K, phis = b.contiguous(), np.ones((nmu, nt + 1, 1))
    return s, th, b_K, phis


@pytest.mark.parametrize('nt', (2, 3))
@pytest.mark.parametrize('nmu', (1, 3, 17))
def test_full_order_trajectories_against_dense_stepping(nmu, nt):
    shape = GRIDS[(nmu + nt) % 2]
    s, th, b_K, phis = _fom_cell(shape, nmu, nt, K=2 if nmu == 3 else 1)
    eng = s['eng']
    ctx, S, n = eng.ctx, eng.S, eng.t.n
    dt = T_END / nt
    U, info = ctx.fom_implicit_euler_batch_tv(th, dt, nt, eng.A_diag, eng.A_cpl, b_K, phis)
    Aq = component_operators(eng.A_diag.cpu().numpy(), eng.A_cpl.cpu().numpy(), ctx.t, s['nbr'])
    ref = tv.fom_euler_batch_tv(Aq, p1_mass(ctx.t.area, S), th, dt, nt, phis, b_K.cpu().numpy())
    err = column_errors(U.cpu().numpy().reshape(nt + 1, S * n, 1, nmu), ref.reshape(nt + 1, S * n, 1, nmu))
    print('PARABOLIC-TV fom {} nmu={} nt={}: {} iterations, panels {}, worst column error {:.2e}'.format(
        shape, nmu, nt, info['iterations'], info['panel_iterations'], float(err.max())))
    assert len(info['panel_iterations']) == (nmu + 15) // 16 and info['relative_residual'] <= 1e-12
    assert np.isfinite(err).all() and err.max() < TOL_TRAJ, float(err.max())


# ---------------------------------------------------------------------------------------------------------- 3. estimates
def _coef(nmu, nt, seed=0):
    """Any positive numbers per (column, step): the export takes the coefficients, not mu."""
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(0.5, 1.5, (nmu, nt + 1, 2)))


def _grams(s, N, layout):
    """The estimator operators of the first N columns in the given layout, from a pass at N columns (device)."""
    key = ('grams', N, layout)
    if key not in s:
        eng = s['eng']
        buf = eng.alloc_reduce_buffers(N, factored=(layout == 'factored'))
        eng.project_and_estimate(eng.ctx.from_numpy(_energy_bases(eng, NB, seed=5)[:, :, :N].copy()), buf)
        s[key] = tuple(g.clone() for g in buf['grams'])
    return s[key]


def _panel(s, N, nmu, nt, th):
    """A solved panel plus a seeded random one of 0.3 times its size [nt + 1, S, N, nmu] (host)."""
    ctx = s['eng'].ctx
    B, M, rhs, _ = _cut(s, N)
    U, _ = ctx.reduced_implicit_euler_batch_tv(th, T_END / nt, nt, _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs))
    U = U.cpu().numpy()
    rng = np.random.default_rng(100 * N + nmu)
    return np.ascontiguousarray(U + 0.3 * np.abs(U).max() * rng.standard_normal(U.shape))


def _host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _err(a, b):
    assert a.shape == b.shape and np.isfinite(a).all(), (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _estimate_reference(s, N, nt, th, coef, Uh, grams, sqrt_local=False, src=None):
    """The NumPy restatement: the elliptic rows of U_k from the batched estimate export at row k (with a source: f2 = 0, r_fd = 0
    plus lrbms_reduced_source_terms per column), nc of the host-formed differences, the time residual of tests/parabolic_tv_ref.py
    with row k + 1, and its combine."""
    import torch
    eng = s['eng']
    ctx = eng.ctx
    B, M, _, _ = _cut(s, N)
    nmu = th.shape[0]
    Ud = _dev(ctx, Uh)
    f2, g = eng.f2, grams
    if src is not None:
        f2 = ctx.zeros(eng.S)
        g = list(grams)
        g[1] = torch.zeros_like(g[1])
        g = tuple(g)
    raw = np.stack([ctx.reduced_estimate_batch(np.ascontiguousarray(th[:, k]), Ud[k].contiguous(), g, f2, eng.ceps, eng.hdiam)
                    .cpu().numpy() for k in range(nt + 1)], axis=1)
    if src is not None:
        for k in range(nt + 1):
            for m in range(nmu):
                raw[1, k, :, m] += ctx.reduced_source_terms(th[m, k], _dev(ctx, src['phi'][m, k:k + 1]), src['F2'], src['r_fd_K'],
                                                            Ud[k, :, :, m:m + 1].contiguous(), eng.ceps, eng.hdiam).cpu().numpy()[:, 0]
    dUh = np.ascontiguousarray(Uh[1:] - Uh[:-1])
    ncd = np.stack([ctx.reduced_estimate_batch(np.ascontiguousarray(th[:, 0]), _dev(ctx, dUh[k]), grams, eng.f2, eng.ceps, eng.hdiam)[0]
                    .cpu().numpy() for k in range(nt)])
    tr2 = tv.time_residual_panel_tv(Uh, B, M, s['nbr'], th)
    return tv.combine_tv(raw, tr2, ncd, coef, T_END / nt, sqrt_local=sqrt_local)


@pytest.mark.parametrize('layout', ('factored', 'dense'))
@pytest.mark.parametrize('shape, N, nmu, nt', (((2, 2), 5, 1, 1), ((3, 3), 17, 3, 3), ((3, 3), 24, 17, 3), ((2, 2), 17, 33, 2),
                                               ((3, 3), 5, 33, 1)))
def test_estimates_against_the_numpy_restatement(shape, N, nmu, nt, layout):
    s = _sys(shape)
    eng = s['eng']
    ctx = eng.ctx
    th, coef = _tables(nmu, nt, 2, seed=N), _coef(nmu, nt)
    Uh = _panel(s, N, nmu, nt, th)
    grams = _grams(s, N, layout)
    B, M, _, _ = _cut(s, N)
    for sq in (False, True):
        res = _host(ctx.reduced_parabolic_estimate_batch_tv(th, coef, T_END / nt, nt, _dev(ctx, Uh), _dev(ctx, B), _dev(ctx, M), grams,
                                                            eng.f2, eng.ceps, eng.hdiam, sqrt_local=sq))
        ref = _estimate_reference(s, N, nt, th, coef, Uh, grams, sqrt_local=sq)
        errs = {k: _err(res[k], ref[k]) for k in ref}
        print('PARABOLIC-TV estimate {} {} N={} nmu={} nt={} sqrt_local={}: '.format(layout, shape, N, nmu, nt, sq)
              + ', '.join('{} {:.2e}'.format(k, v) for k, v in errs.items()))
        assert res['est'].min() > 0.0 and res['time_residual'].min() > 0.0
        for k, v in errs.items():
            assert v <= TOL_EST, (k, v)


def test_estimates_with_the_vertex_patch_and_with_a_source():
    """The vertex-patch convention of the Oswald interpolation (factored layout) and a K = 3 time-dependent source."""
    from pylrbms_amd.engine import Engine
    from common import theta_bar_of
    from test_pcg_iterates_gpu import _problem
    shape, N, nmu, nt, K = (3, 3), 17, 17, 3, 3
    s = _sys(shape)
    p = _problem(shape, KC)
    lam = p['lambda']
    eng = Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar_of(p),
                 conventions={'oswald_vertex_patch': True}).assemble()
    ctx = eng.ctx
    buf = eng.alloc_reduce_buffers(N, factored=True)
    eng.project_and_estimate(ctx.from_numpy(_energy_bases(eng, N, seed=5)), buf)
    Bh, Mh = buf['sys'][0].cpu().numpy(), buf['sys'][3].cpu().numpy()
    sv = dict(s, eng=eng, B=Bh, M=Mh, rhs=buf['sys'][1].cpu().numpy())
    th, coef = _tables(nmu, nt, 2, seed=9), _coef(nmu, nt, seed=2)
    Uh = _panel(sv, N, nmu, nt, th)
    grams = tuple(g.clone() for g in buf['grams'])
    res = _host(ctx.reduced_parabolic_estimate_batch_tv(th, coef, T_END / nt, nt, _dev(ctx, Uh), buf['sys'][0], buf['sys'][3], grams,
                                                        eng.f2, eng.ceps, eng.hdiam))
    ref = _estimate_reference(sv, N, nt, th, coef, Uh, grams)
    for k in ref:
        assert _err(res[k], ref[k]) <= TOL_EST, ('vertex patch', k, _err(res[k], ref[k]))
    # a time-dependent source on the plain engine
    eng, ctx = s['eng'], s['eng'].ctx
    rng = np.random.default_rng(5)
    grams = _grams(s, N, 'factored')
    B, M, _, _ = _cut(s, N)
    src = dict(phi=np.ascontiguousarray(rng.uniform(0.2, 1.0, (nmu, nt + 1, K))),
               F2=_dev(ctx, np.einsum('ski,skj->sij', *(2 * (rng.standard_normal((eng.S, 4, K)),))) + np.eye(K)),
               r_fd_K=_dev(ctx, rng.standard_normal((K, eng.S, 5 * 2 * N)) * float(grams[1].abs().max())))
    Uh = _panel(s, N, nmu, nt, th)
    res = _host(ctx.reduced_parabolic_estimate_batch_tv(th, coef, T_END / nt, nt, _dev(ctx, Uh), _dev(ctx, B), _dev(ctx, M), grams,
                                                        eng.f2, eng.ceps, eng.hdiam, phi=src['phi'], F2=src['F2'], r_fd_K=src['r_fd_K']))
    ref = _estimate_reference(s, N, nt, th, coef, Uh, grams, src=src)
    for k in ref:
        assert _err(res[k], ref[k]) <= TOL_EST, ('source', k, _err(res[k], ref[k]))


# ------------------------------------------------------------------------------------------- 4. a table constant in time
@pytest.mark.parametrize('shape, N, nmu, nt', (((2, 2), 17, 3, 3), ((3, 3), 24, 33, 3), ((3, 3), 5, 17, 1)))
def test_constant_tables_are_the_existing_exports(shape, N, nmu, nt):
    s = _sys(shape)
    eng = s['eng']
    ctx = eng.ctx
    dt = T_END / nt
    B, M, rhs, _ = _cut(s, N)
    Bd, Md, rd = _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs)
    thetas = np.ascontiguousarray(_tables(nmu, 2, 2, seed=1)[:, 1])
    th = np.ascontiguousarray(np.repeat(thetas[:, None, :], nt + 1, axis=1))
    U0, _ = ctx.reduced_implicit_euler_batch(thetas, dt, nt, Bd, Md, rd)
    U1, _ = ctx.reduced_implicit_euler_batch_tv(th, dt, nt, Bd, Md, rd)
    assert column_errors(U1.cpu().numpy(), U0.cpu().numpy()).max() < TOL_TRAJ
    rhs_K, phis = _sources(s, N, nmu, nt, 3, rhs)
    V0, _ = ctx.reduced_implicit_euler_batch_src(thetas, dt, nt, Bd, Md, _dev(ctx, rhs_K), phis)
    V1, _ = ctx.reduced_implicit_euler_batch_tv(th, dt, nt, Bd, Md, _dev(ctx, rhs_K), phi=phis)
    assert column_errors(V1.cpu().numpy(), V0.cpu().numpy()).max() < TOL_TRAJ
    # estimates
    grams = _grams(s, N, 'factored')
    c2 = _coef(nmu, 1)[:, 0]
    args = (U0, Bd, Md, grams, eng.f2, eng.ceps, eng.hdiam)
    e0 = _host(ctx.reduced_parabolic_estimate_batch(thetas, c2, dt, nt, *args))
    e1 = _host(ctx.reduced_parabolic_estimate_batch_tv(th, np.ascontiguousarray(np.repeat(c2[:, None, :], nt + 1, axis=1)), dt, nt, *args))
    for k in e0:
        assert _err(e1[k], e0[k]) <= TOL_EST, k
    # full order
    if nmu <= 17:
        b_K, ones = eng.b.reshape(1, eng.S, eng.t.n).contiguous(), np.ones((nmu, nt + 1, 1))
        F0, _ = ctx.fom_implicit_euler_batch(thetas, dt, nt, eng.A_diag, eng.A_cpl, b_K, ones)
        F1, _ = ctx.fom_implicit_euler_batch_tv(th, dt, nt, eng.A_diag, eng.A_cpl, b_K, ones)
        F0, F1 = (x.cpu().numpy().reshape(nt + 1, -1, 1, nmu) for x in (F0, F1))
        assert column_errors(F1, F0).max() < TOL_TRAJ


def test_swapping_the_rows_of_two_columns_swaps_their_results_bit_for_bit():
    import torch
    shape, N, nmu, nt = (3, 3), 17, 17, 3
    s = _sys(shape)
    eng = s['eng']
    ctx = eng.ctx
    dt = T_END / nt
    B, M, rhs, _ = _cut(s, N)
    Bd, Md, rd = _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs)
    th, coef = _tables(nmu, nt, 2, seed=6), _coef(nmu, nt)
    perm = np.arange(nmu)
    perm[[2, 11]] = perm[[11, 2]]
    U, _ = ctx.reduced_implicit_euler_batch_tv(th, dt, nt, Bd, Md, rd)
    Up, _ = ctx.reduced_implicit_euler_batch_tv(np.ascontiguousarray(th[perm]), dt, nt, Bd, Md, rd)
    assert torch.equal(U[..., perm], Up) and not torch.equal(U[..., 2], U[..., 11])
    grams = _grams(s, N, 'factored')
    Uh = _panel(s, N, nmu, nt, th)
    args = (Bd, Md, grams, eng.f2, eng.ceps, eng.hdiam)
    x = _host(ctx.reduced_parabolic_estimate_batch_tv(th, coef, dt, nt, _dev(ctx, Uh), *args))
    y = _host(ctx.reduced_parabolic_estimate_batch_tv(np.ascontiguousarray(th[perm]), np.ascontiguousarray(coef[perm]), dt, nt,
                                                      _dev(ctx, Uh[..., perm]), *args))
    for k in x:
        assert np.array_equal(x[k][..., perm], y[k]), k
    assert not np.array_equal(x['est'][2], x['est'][11])
    b_K, ones = eng.b.reshape(1, eng.S, eng.t.n).contiguous(), np.ones((nmu, nt + 1, 1))
    F, _ = ctx.fom_implicit_euler_batch_tv(th, dt, nt, eng.A_diag, eng.A_cpl, b_K, ones, rtol=1e-10)
    Fp, _ = ctx.fom_implicit_euler_batch_tv(np.ascontiguousarray(th[perm]), dt, nt, eng.A_diag, eng.A_cpl, b_K, ones, rtol=1e-10)
    # (the columns 2 and 11 share the first panel: the panel's iteration count, hence the bits, do not depend on their order)
    assert torch.equal(F[..., perm], Fp)


# ------------------------------------------------------------------------------------- 5. poisoned work, repeats, refusals
@pytest.mark.parametrize('nmu', (3, 33))
def test_poisoned_work_and_repeat_calls(nmu):
    import torch
    shape, N, nt = (3, 3), 17, 3
    s = _sys(shape)
    eng = s['eng']
    ctx = eng.ctx
    dt = T_END / nt
    B, M, rhs, _ = _cut(s, N)
    Bd, Md, rd = _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs)
    th, coef = _tables(nmu, nt, 2, seed=8), _coef(nmu, nt)
    th0, coef0 = th.copy(), coef.copy()
    U = poisoned(ctx, lambda: ctx.reduced_implicit_euler_batch_tv(th, dt, nt, Bd, Md, rd)[0])
    assert torch.equal(U, ctx.reduced_implicit_euler_batch_tv(th, dt, nt, Bd, Md, rd)[0])
    grams = _grams(s, N, 'factored')
    Uc = U.clone()
    est = lambda: ctx.reduced_parabolic_estimate_batch_tv(th, coef, dt, nt, U, Bd, Md, grams, eng.f2, eng.ceps, eng.hdiam)      # noqa: E731
    a = poisoned(ctx, lambda: torch.cat([v.reshape(-1) for v in est().values()]))
    assert torch.equal(a, torch.cat([v.reshape(-1) for v in est().values()]))
    if nmu <= 16:
        b_K, ones = eng.b.reshape(1, eng.S, eng.t.n).contiguous(), np.ones((nmu, nt + 1, 1))
        fom = lambda: ctx.fom_implicit_euler_batch_tv(th, dt, nt, eng.A_diag, eng.A_cpl, b_K, ones, rtol=1e-10)[0]      # noqa: E731
        assert torch.equal(poisoned(ctx, fom), fom())
    assert torch.equal(U, Uc) and np.array_equal(th, th0) and np.array_equal(coef, coef0)
    assert torch.equal(Bd, _dev(ctx, B)) and torch.equal(Md, _dev(ctx, M)) and torch.equal(rd, _dev(ctx, rhs))


def test_refusals_leave_everything_untouched():
    import torch
    from pylrbms_amd._native import _dblp, c_vp
    LRBMS_E_INVALID = -1                                                   # include/lrbms_hip.h
    shape, N, nt = (2, 2), 5, 2
    s = _sys(shape)
    eng = s['eng']
    ctx, S, n = eng.ctx, eng.S, eng.t.n
    B, M, rhs, _ = _cut(s, N)
    Bd, Md, rd = _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs)
    th = _tables(64, nt, 2)
    big = np.ascontiguousarray(np.tile(th, (2, 1, 1))[:65])
    th5 = np.ascontiguousarray(np.random.default_rng(0).uniform(0.2, 1.0, (17, nt + 1, 5)))
    mark = 7.25
    vp = lambda t: c_vp(t.data_ptr())                                                                                  # noqa: E731
    assert ctx.lib.lrbms_reduced_implicit_euler_batch_tv_work_size(ctx.handle, N, 0, nt) == -1
    assert ctx.lib.lrbms_reduced_implicit_euler_batch_tv_work_size(ctx.handle, N, 3, 0) == -1
    assert ctx.lib.lrbms_reduced_parabolic_estimate_batch_tv_work_size(ctx.handle, N, 3, 0) == -1
    need = int(ctx.lib.lrbms_reduced_implicit_euler_batch_tv_work_size(ctx.handle, N, 64, nt))
    assert need > int(ctx.lib.lrbms_reduced_implicit_euler_batch_work_size(ctx.handle, N, 64))
    work = torch.full((need,), mark, dtype=torch.float64, device=Bd.device)
    U = torch.full((nt + 1, S, N, 65), mark, dtype=torch.float64, device=Bd.device)
    info = np.zeros(2)

    def red(nmu, table, nt_=nt, dt=0.01, rtol=1e-13, Q=2, K=0, phi=None):
        return _raw(ctx, 'lrbms_reduced_implicit_euler_batch_tv', Q, N, K, nmu, _dblp(table), dt, nt_, vp(Bd), vp(Md), vp(rd),
                    c_vp(None) if phi is None else vp(phi), vp(work), vp(U), rtol, 100, _dblp(info), ctx._stream())
    for rc in (red(0, th), red(65, big), red(3, th, nt_=0), red(3, th, dt=0.0), red(3, th, rtol=0.0), red(17, th5, Q=5),
               red(3, th, K=65), red(3, th, K=2)):
        assert rc == LRBMS_E_INVALID
    # full order: nmu, nt, K out of range
    fwork = torch.full((int(ctx.lib.lrbms_fom_implicit_euler_batch_work_size(ctx.handle, 3)),), mark, dtype=torch.float64, device=Bd.device)
    FU = torch.full((nt + 1, S, n, 65), mark, dtype=torch.float64, device=Bd.device)
    b_K, ones = eng.b.reshape(1, S, n).contiguous(), _dev(ctx, np.ones((65, nt + 1, 1)))

    def fom(nmu, table, nt_=nt, K=1):
        return _raw(ctx, 'lrbms_fom_implicit_euler_batch_tv', 2, K, nmu, _dblp(table), 0.01, nt_, vp(eng.A_diag), vp(eng.A_cpl), vp(b_K),
                    vp(ones), vp(fwork), vp(FU), 1e-10, 100, _dblp(info), ctx._stream())
    for rc in (fom(0, th), fom(65, big), fom(3, th, nt_=0), fom(3, th, K=0)):
        assert rc == LRBMS_E_INVALID
    # estimate: nmu, nt, dt, Q for wide calls, F_side without F_nc
    grams = _grams(s, N, 'factored')
    gp, _ = ctx._gram_ptrs(grams, 2, N)
    ework = torch.full((int(ctx.lib.lrbms_reduced_parabolic_estimate_batch_tv_work_size(ctx.handle, N, 64, nt)),), mark,
                       dtype=torch.float64, device=Bd.device)
    outs = [torch.full(shp, mark, dtype=torch.float64, device=Bd.device)
            for shp in ((3, nt + 1, S, 65), (nt, S, 65), (nt, 65), (nt + 1, 65), (65,))]
    coef = _coef(65, nt)

    def est(nmu, table, nt_=nt, dt=0.01, Q=2, g=gp):
        return _raw(ctx, 'lrbms_reduced_parabolic_estimate_batch_tv', Q, N, 0, nmu, nt_, dt, _dblp(table), _dblp(coef), 0, vp(U), vp(Bd),
                    vp(Md), *g, vp(eng.f2), vp(eng.ceps), float(eng.hdiam), c_vp(None), c_vp(None), c_vp(None), vp(ework),
                    *[vp(o) for o in outs], ctx._stream())
    for rc in (est(0, th), est(65, big), est(3, th, nt_=0), est(3, th, dt=0.0), est(17, th5, Q=5), est(3, th, g=gp[:7] + [c_vp(None)])):
        assert rc == LRBMS_E_INVALID
    for t in [work, U, fwork, FU, ework] + outs:
        assert bool((t == mark).all())


# ------------------------------------------------------------------------------------------------------------ 6. end to end
_E2E = {}


def _channels(switch_off_after):
    """The artificial-channels problem on 4 x 4 subdomains, nt = 4, with and without the switch (kept per variant)."""
    if switch_off_after not in _E2E:
        from pylrbms_amd import artificial_channels_problem as acp
        from pylrbms_amd.discretize_parabolic_block_swipdg import discretize
        p = acp.init_grid_and_problem({'num_subdomains': [4, 4], 'half_num_fine_elements_per_subdomain_and_dim': 4},
                                      switch_off_after=switch_off_after)
        d, data = discretize(p, 0.05, 4)
        _E2E[switch_off_after] = (p, d, data)
    return _E2E[switch_off_after]


def test_switched_channels_end_to_end():
    from pylrbms_amd.reductor import ParabolicLRBMSReductor
    T, nt = 0.05, 4
    t_star = 1.5 * T / nt                                                   # between the steps 1 and 2
    p, d, data = _channels(t_star)
    _, d0, _ = _channels(None)
    assert d._tv and not d0._tv and '_t' not in d.parameter_type
    mus = [[0.2], [0.6], [1.0]]
    th = d.diffusion_coefficients(mus[1])
    assert th.shape == (nt + 1, 4) and np.all(th[:2, 3] == 0.6) and np.all(th[2:, 3] == p['mu_min'][0])
    # refusals of the time-dependent discretization
    for call in (lambda: d.solve_stationary(mus[0]), lambda: d.solve_stationary_batch(mus), lambda: d.theta(mus[0])):
        with pytest.raises(NotImplementedError):
            call()
    # the trajectory differs from the unswitched one only after t*
    trajs = d.solve_batch(mus)
    plain = d0.solve_batch(mus)
    for U, U0 in zip(trajs, plain):
        a, b = U.tensor.cpu().numpy(), U0.tensor.cpu().numpy()              # [S, n, nt + 1]
        scale = np.abs(b).max()
        assert np.abs(a[..., :2] - b[..., :2]).max() <= TOL_TRAJ * scale
        assert np.abs(a[..., 2:] - b[..., 2:]).max() > 1e3 * TOL_TRAJ * scale
    one = d.solve(mus[1]).tensor
    assert float((one - trajs[1].tensor).abs().max()) <= TOL_TRAJ * float(one.abs().max())
    # POD -> reduce -> reduced sweep
    reductor = ParabolicLRBMSReductor(d, products=[d.operators['local_energy_dg_product_{}'.format(ii)]
                                                   for ii in range(data['block_space'].num_blocks)])
    reductor.extend_basis(d.solve_batch(mus, as_snapshots=True), method='pod', pod_modes=6)
    rd = reductor.reduce()
    us = rd.solve_batch(mus)
    ests = rd.estimate_batch(us, mus)
    assert len(us) == len(ests) == len(mus)
    u1 = rd.solve(mus[1]).tensor
    assert float((u1 - us[1].tensor).abs().max()) <= TOL_TRAJ * float(u1.abs().max())
    e1 = rd.estimate(us[1], mus[1])
    assert abs(e1[0] - ests[1][0]) <= TOL_EST * ests[1][0] and ests[1][0] > 0.0
    # the reduced trajectory reproduces the snapshots it was built from, and the full-order estimate of the reconstruction (the
    # verification path in Python) agrees with the native export on every part that does not invert a mass matrix -- the time
    # residual uses M^-1 there and M_red^-1 here; 1e-6 is the bound of the same comparison in tests/test_parabolic_source_gpu.py
    Ur = reductor.reconstruct(us[1])
    err = float((Ur.tensor - trajs[1].tensor).abs().max() / trajs[1].tensor.abs().max())
    print('PARABOLIC-TV end to end: N = {}, reconstruction error {:.2e}, est {}'.format(rd.N, err, [e[0] for e in ests]))
    assert err < 1e-3
    ef = d.estimate(Ur, mus[1])
    for i in (0, 1, 2, 4):
        assert _err(np.asarray(ef[1][i]), np.asarray(ests[1][1][i])) < 1e-6, i
    assert ef[0] > 0.0 and np.isfinite(ef[0])


def test_a_time_independent_discretization_calls_none_of_the_tv_exports():
    from pylrbms_amd.reductor import ParabolicLRBMSReductor
    _, d0, data = _channels(None)
    ctx = d0.engine.ctx
    calls = []
    names = ('fom_implicit_euler_batch_tv', 'reduced_implicit_euler_batch_tv', 'reduced_parabolic_estimate_batch_tv')
    for name in names:
        def spy(*a, _name=name, **kw):
            calls.append(_name)
            raise AssertionError(_name)
        setattr(ctx, name, spy)
    try:
        mus = [[0.3], [0.9]]
        U = d0.solve(mus[0])
        reductor = ParabolicLRBMSReductor(d0, products=[d0.operators['local_energy_dg_product_{}'.format(ii)]
                                                        for ii in range(data['block_space'].num_blocks)])
        reductor.extend_basis(d0.solve_batch(mus, as_snapshots=True), method='pod', pod_modes=4)
        rd = reductor.reduce()
        us = rd.solve_batch(mus)
        rd.estimate_batch(us, mus)
        rd.estimate(rd.solve(mus[0]), mus[0])
        d0.estimate(U, mus[0])
    finally:
        for name in names:
            delattr(ctx, name)
    assert calls == []
