"""Batched parabolic estimates on the GPU: lrbms_reduced_parabolic_estimate_batch -- the estimator of all trajectories of a batched
reduced solve in one native call -- against the existing estimate exports slab by slab, the NumPy restatement of
tests/parabolic_estimate_batch_ref.py (pinned to the oracle in tests/test_parabolic_estimate_batch_host.py), and through
``InstationaryReducedDiscretization.estimate_batch`` against ``rd.estimate`` and the oracle.

Shapes: the grid of the iterate tests (4 x 3 subdomains, k_c = 2), operators cut from ONE pass at 64 energy-orthonormal columns
per layout, nt <= 3, dt = 0.05 / nt.  Input panels are a solved panel plus a seeded random one, so that no term vanishes.
Tolerance of the native comparisons: 1e-10 relative to the largest entry of the part (the project's bound for
estimate columns)."""
import numpy as np
import pytest

from parabolic_estimate_batch_ref import combine, time_residual_panel
from test_parabolic_batch_gpu import NMAX, T_END, _cut, _system, _thetas
from test_pcg_iterates_gpu import KC, SWEEP_GRID, _dev, _energy_bases
from test_work_poison_gpu import poisoned

pytestmark = pytest.mark.gpu

TOL = 1e-10
Q = 2
PARTS = ('local_eta_nc', 'local_eta_r', 'local_eta_df', 'time_residual', 'time_deriv_nc')
CELLS = ((3, 1, 2), (5, 17, 2), (24, 16, 2), (40, 33, 2), (64, 64, 2), (24, 17, 1), (24, 17, 3))      # N, nmu, nt
LAYOUTS = ('factored', 'dense')

_PASS = {}


def _err(a, b):
    a = a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().numpy() if hasattr(b, 'detach') else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _pass(layout):
    """The projected estimator operators of ONE pass at NMAX columns in the given layout (device, left unchanged)."""
    if layout not in _PASS:
        eng = _system()['eng']
        assert eng.ctx.fused_supported(Q, NMAX, factored=True)
        buf = eng.alloc_reduce_buffers(NMAX, factored=(layout == 'factored'))
        eng.project_and_estimate(eng.ctx.from_numpy(_energy_bases(eng, NMAX, seed=5)), buf)
        _PASS[layout] = tuple(g.clone() for g in buf['grams'])
    return _PASS[layout]


def _grams(layout, N):
    """The operators of the first N basis columns, cut out of the pass at NMAX (every entry belongs to one pair of columns)."""
    import torch
    eng = _system()['eng']
    S, F, ncf = eng.S, NMAX, eng.t.ncf
    g = _pass(layout)
    QN = Q * N
    if layout == 'factored':
        G_nc, r_fd, G_rdd, G_bb, G_ab, G_aa, Fs, Fn = g
        self_cut = lambda G: G.reshape(S, Q, F, Q, F)[:, :, :N, :, :N].reshape(S, QN, QN)        # noqa: E731
        out = (G_nc[:, :N, :N], r_fd.reshape(S, 5, Q, F)[..., :N].reshape(S, 5 * QN), self_cut(G_rdd), self_cut(G_bb),
               G_ab.reshape(Q, S, F, Q, F)[:, :, :N, :, :N].reshape(Q, S, N, QN), G_aa[..., :N, :N],
               torch.cat([Fs[..., :4 * Q * F].reshape(S, 4, ncf, 4 * Q, F)[..., :N].reshape(S, 4, ncf, 4 * QN), Fs[..., 4 * Q * F:]],
                         dim=3),
               torch.cat([Fn[..., :N], Fn[..., F:F + N], Fn[..., 2 * F:]], dim=3))
    else:
        G_nc, r_fd, G_rdd, G_bb, G_ab, G_aa = g
        side_cut = lambda G: G.reshape(S, 9, Q, F, Q, F)[:, :, :, :N, :, :N].reshape(S, 9, QN, QN)      # noqa: E731
        out = (G_nc.reshape(S, 5, F, 5, F)[:, :, :N, :, :N].reshape(S, 5 * N, 5 * N),
               r_fd.reshape(S, 5, Q, F)[..., :N].reshape(S, 5 * QN), side_cut(G_rdd), side_cut(G_bb),
               G_ab.reshape(Q, S, F, 5, Q, F)[:, :, :N, :, :, :N].reshape(Q, S, N, 5 * QN), G_aa[..., :N, :N])
    return tuple(t.contiguous() for t in out)


def _panel(N, nmu, nt, seed=0):
    """A solved panel plus a seeded random one of 0.3 times its size [nt + 1, S, N, nmu] (host)."""
    s = _system()
    ctx = s['eng'].ctx
    B, M, rhs = _cut(N)
    U, _ = ctx.reduced_implicit_euler_batch(_thetas(nmu), T_END / nt, nt, _dev(ctx, B), _dev(ctx, M), _dev(ctx, rhs))
    U = U.cpu().numpy()
    rng = np.random.default_rng(100 * N + nmu + seed)
    return np.ascontiguousarray(U + 0.3 * np.abs(U).max() * rng.standard_normal(U.shape))


def _abh(nmu):
    """alpha_bar, gamma_bar, alpha_hat per column (any positive numbers: the export takes the coefficients, not mu)."""
    return np.linspace(0.5, 1.5, nmu), np.linspace(1.0, 2.0, nmu), np.linspace(0.7, 1.2, nmu)


def _coef(nmu):
    a_bar, g_bar, a_hat = _abh(nmu)
    return np.ascontiguousarray(np.stack([np.sqrt(g_bar) / np.sqrt(a_bar), (1.0 / np.sqrt(a_hat)) / np.sqrt(a_bar)], axis=1))


def _call(N, Ud, thetas, nt, layout='factored', grams=None, f2=None, **kw):
    s = _system()
    eng = s['eng']
    ctx = eng.ctx
    B, M, _ = _cut(N)
    nmu = thetas.shape[0]
    return ctx.reduced_parabolic_estimate_batch(thetas, _coef(nmu), T_END / nt, nt, Ud, _dev(ctx, B), _dev(ctx, M),
                                                grams if grams is not None else _grams(layout, N),
                                                f2 if f2 is not None else eng.f2, eng.ceps, eng.hdiam, **kw)


def _host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _combine_of(res, nmu, dt, sqrt_local=False):
    """The NumPy combine on the device's own local parts (eta_loc unscaled again; the sums of tr2 / nc_diff as one 'subdomain')."""
    s = 2 * np.sqrt(dt / 3)
    a_bar, g_bar, a_hat = _abh(nmu)
    return combine(res['eta_loc'] / s, (res['time_residual'] ** 2 / (dt / 3))[:, None, :], res['time_deriv_nc'] ** 2 * dt,
                   a_bar, g_bar, a_hat, dt, sqrt_local=sqrt_local)


# ------------------------------------------------------------------------------- 2. the native call against the existing exports
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('N, nmu, nt', CELLS)
def test_native_call_against_the_existing_exports(N, nmu, nt, layout):
    s = _system()
    eng = s['eng']
    ctx, S = eng.ctx, eng.S
    dt = T_END / nt
    sc = 2 * np.sqrt(dt / 3)
    B, M, _ = _cut(N)
    Bd, Md = _dev(ctx, B), _dev(ctx, M)
    thetas = _thetas(nmu)
    grams = _grams(layout, N)
    Uh = _panel(N, nmu, nt)
    Ud = _dev(ctx, Uh)
    res = _host(_call(N, Ud, thetas, nt, layout))
    assert res['eta_loc'].shape == (3, nt + 1, S, nmu) and res['time_deriv_nc'].shape == (nt, S, nmu)
    assert res['time_residual'].shape == (nt, nmu) and res['eta'].shape == (nt + 1, nmu) and res['est'].shape == (nmu,)
    # per slab: the batched estimate export on U[k], its nc row on the host-formed differences
    raw = np.stack([ctx.reduced_estimate_batch(thetas, Ud[k].contiguous(), grams, eng.f2, eng.ceps, eng.hdiam).cpu().numpy()
                    for k in range(nt + 1)], axis=1)
    dUh = np.ascontiguousarray(Uh[1:] - Uh[:-1])
    ncd = np.stack([ctx.reduced_estimate_batch(thetas, _dev(ctx, dUh[k]), grams, eng.f2, eng.ceps, eng.hdiam)[0].cpu().numpy()
                    for k in range(nt)])
    assert ncd.min() > 0.0
    tr_dev = np.empty((nt, nmu))
    for m in range(nmu):
        out = ctx.reduced_time_residual(thetas[m], Bd, Md, _dev(ctx, dUh[..., m]))
        tr_dev[:, m] = np.sqrt(out.sum(dim=1).cpu().numpy() * (dt / 3))
    tr_np = np.sqrt(time_residual_panel(Uh, B, M, s['nbr'], thetas).sum(axis=1) * (dt / 3))
    ref = _combine_of(res, nmu, dt)
    errs = {'nc': _err(res['eta_loc'][0], raw[0] * sc), 'r': _err(res['eta_loc'][1], raw[1] * sc),
            'df': _err(res['eta_loc'][2], raw[2] * sc), 'time_deriv_nc': _err(res['time_deriv_nc'], np.sqrt(ncd / dt)),
            'time_residual/export': _err(res['time_residual'], tr_dev), 'time_residual/numpy': _err(res['time_residual'], tr_np),
            'eta': _err(res['eta'], ref['eta']), 'est': _err(res['est'], ref['est'])}
    print('PARABOLIC-ESTIMATE-BATCH {} N={} nmu={} nt={}: '.format(layout, N, nmu, nt)
          + ', '.join('{} {:.2e}'.format(k, v) for k, v in errs.items()))
    assert res['est'].min() > 0.0 and res['time_residual'].min() > 0.0
    for k, v in errs.items():
        assert v <= TOL, (k, v)


def test_the_two_layouts_agree():
    N, nmu, nt = 24, 17, 2
    ctx = _system()['eng'].ctx
    Ud = _dev(ctx, _panel(N, nmu, nt))
    a, b = (_host(_call(N, Ud, _thetas(nmu), nt, layout)) for layout in LAYOUTS)
    for k in a:
        assert _err(a[k], b[k]) <= TOL, k


def test_sqrt_local_switch():
    N, nmu, nt = 24, 17, 2
    ctx = _system()['eng'].ctx
    dt = T_END / nt
    Ud = _dev(ctx, _panel(N, nmu, nt))
    plain, sq = (_host(_call(N, Ud, _thetas(nmu), nt, sqrt_local=flag)) for flag in (False, True))
    sc = 2 * np.sqrt(dt / 3)
    assert _err(sq['eta_loc'], np.sqrt(np.abs(plain['eta_loc'] / sc)) * sc) <= TOL
    ref = _combine_of(plain, nmu, dt, sqrt_local=True)                      # the NumPy combine of the unrooted parts
    for k in ('eta_loc', 'eta', 'est'):
        assert _err(sq[k], ref[k]) <= TOL, k
    assert _err(sq['est'], plain['est']) > 1e-3                             # the switch is seen
    for k in ('time_residual', 'time_deriv_nc'):
        assert np.array_equal(sq[k], plain[k]), k


# -------------------------------------------------------------------------------------------- 3. theta really is per column
def test_theta_is_per_column():
    """Two columns hold the same trajectory at different theta: every theta-dependent output differs (r, df, time residual, eta,
    est; the nonconformity rows do not involve theta and agree bitwise); swapping the columns swaps the outputs bitwise; a column
    of zeros gives exact zeros in every part, est = 0 when f = 0, and with f its r row is the zero-solution value."""
    import torch
    N, nt = 24, 2
    s = _system()
    eng = s['eng']
    ctx = eng.ctx
    dt = T_END / nt
    one = _panel(N, 1, nt)
    Uh = np.ascontiguousarray(np.concatenate([one, one, np.zeros_like(one)], axis=3))
    thetas = np.ascontiguousarray(np.array([[1.0, 0.2], [1.0, 0.9], [1.0, 0.5]]))
    a = _host(_call(N, _dev(ctx, Uh), thetas, nt))
    for k in ('time_residual', 'eta', 'est'):
        assert np.all(a[k][..., 0] != a[k][..., 1]), k
    assert np.all(a['eta_loc'][1:, ..., 0] != a['eta_loc'][1:, ..., 1])
    assert np.array_equal(a['eta_loc'][0, ..., 0], a['eta_loc'][0, ..., 1])
    assert np.array_equal(a['time_deriv_nc'][..., 0], a['time_deriv_nc'][..., 1])
    # the columns of a call with swapped (theta, coef) pairs: the same bits at the swapped places (coef is per column too)
    perm = [1, 0, 2]
    coef = _coef(3)
    B, M, _ = _cut(N)
    args = (_dev(ctx, B), _dev(ctx, M), _grams('factored', N), eng.f2, eng.ceps, eng.hdiam)
    x = _host(ctx.reduced_parabolic_estimate_batch(thetas, coef, dt, nt, _dev(ctx, Uh), *args))
    y = _host(ctx.reduced_parabolic_estimate_batch(thetas[perm], coef[perm], dt, nt, _dev(ctx, Uh[..., perm]), *args))
    for k in x:
        assert np.array_equal(x[k][..., perm], y[k]), k
    # the zero column: with f its r row is the zero-solution value of the estimate export, everything else exact zeros
    zero_u = ctx.zeros(eng.S, N, 1)
    r0 = ctx.reduced_estimate_batch(thetas[2:], zero_u, _grams('factored', N), eng.f2, eng.ceps, eng.hdiam).cpu().numpy()
    assert np.abs(r0[1]).max() > 0.0
    for k in range(nt + 1):
        assert _err(a['eta_loc'][1, k, :, 2], r0[1, :, 0] * 2 * np.sqrt(dt / 3)) <= 1e-14
    assert np.all(a['eta_loc'][[0, 2], ..., 2] == 0.0) and np.all(a['time_deriv_nc'][..., 2] == 0.0)
    assert np.all(a['time_residual'][..., 2] == 0.0)
    grams0 = list(_grams('factored', N))
    grams0[1] = torch.zeros_like(grams0[1])
    z = _host(_call(N, _dev(ctx, Uh), thetas, nt, grams=tuple(grams0), f2=ctx.zeros(eng.S)))
    for k in z:
        assert np.all(z[k][..., 2] == 0.0), k
    assert z['est'][0] > 0.0


# ----------------------------------------------------------------------------------------------------------- 4. source terms
def _source(N, K, seed=7):
    eng = _system()['eng']
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((eng.S, K, K))
    F2 = np.ascontiguousarray(np.einsum('sij,skj->sik', X, X))
    r_fd_K = np.ascontiguousarray(rng.standard_normal((K, eng.S, 5 * Q * N)))
    return F2, r_fd_K


def test_time_dependent_source_rows():
    """K = 3, phi switching sign per column and step, against the batched estimate with zero f2 / r_fd plus the single-theta
    lrbms_reduced_source_terms per parameter."""
    import torch
    N, nmu, nt, K = 24, 17, 3, 3
    eng = _system()['eng']
    ctx = eng.ctx
    dt = T_END / nt
    sc = 2 * np.sqrt(dt / 3)
    thetas = _thetas(nmu)
    Uh = _panel(N, nmu, nt)
    Ud = _dev(ctx, Uh)
    F2, r_fd_K = _source(N, K)
    phi = np.empty((nmu, nt + 1, K))
    for m in range(nmu):
        for k in range(nt + 1):
            phi[m, k] = (-1.0) ** (m + k) * (1.0 + 0.1 * np.arange(K) + 0.01 * m)
    grams = _grams('factored', N)
    res = _host(_call(N, Ud, thetas, nt, phi=phi, F2=_dev(ctx, F2), r_fd_K=_dev(ctx, r_fd_K)))
    grams0 = list(grams)
    grams0[1] = torch.zeros_like(grams0[1])
    zero_f2 = ctx.zeros(eng.S)
    want = np.stack([ctx.reduced_estimate_batch(thetas, Ud[k].contiguous(), tuple(grams0), zero_f2, eng.ceps, eng.hdiam).cpu().numpy()
                     for k in range(nt + 1)], axis=1)                       # [3, nt + 1, S, nmu]
    for m in range(nmu):
        u = _dev(ctx, np.ascontiguousarray(Uh[..., m].transpose(1, 2, 0)))  # [S, N, nt + 1]
        add = ctx.reduced_source_terms(thetas[m], phi[m], _dev(ctx, F2), _dev(ctx, r_fd_K), u, eng.ceps, eng.hdiam).cpu().numpy()
        want[1, :, :, m] += add.T
    plain = _host(_call(N, Ud, thetas, nt))
    assert _err(res['eta_loc'][1], plain['eta_loc'][1]) > 1e-3              # the source is seen
    for i, nm in enumerate(PARTS[:3]):
        e = _err(res['eta_loc'][i], want[i] * sc)
        print('PARABOLIC-ESTIMATE-BATCH source K=3 {}: {:.2e}'.format(nm, e))
        assert e <= TOL, nm
    ref = _combine_of(res, nmu, dt)
    assert _err(res['eta'], ref['eta']) <= TOL and _err(res['est'], ref['est']) <= TOL


def test_one_unit_source_component_is_the_call_without_a_source():
    N, nmu, nt = 24, 17, 2
    eng = _system()['eng']
    ctx = eng.ctx
    Ud = _dev(ctx, _panel(N, nmu, nt))
    grams = _grams('factored', N)
    plain = _host(_call(N, Ud, _thetas(nmu), nt))
    one = _host(_call(N, Ud, _thetas(nmu), nt, phi=np.ones((nmu, nt + 1, 1)), F2=eng.f2.reshape(-1, 1, 1).contiguous(),
                      r_fd_K=grams[1][None].contiguous()))
    for k in plain:
        assert _err(one[k], plain[k]) <= 1e-12, k


# ------------------------------------------------------------------------------------------------------------ 6. ragged bases
def test_zero_padded_basis_columns():
    """Zero-padded basis columns contribute exactly 0 and M_red counts as the identity there: garbage in the padded rows of the
    panel does not change the time residual (bitwise), which is that of lrbms_reduced_time_residual (the same rule)."""
    from common import oracle_from_problem, ragged_padded_bases
    from test_pcg_iterates_gpu import _problem
    s = _system()
    eng = s['eng']
    ctx = eng.ctx
    N, nmu, nt = 12, 20, 2
    dt = T_END / nt
    V, sizes = ragged_padded_bases(oracle_from_problem(_problem(SWEEP_GRID, KC)), N, seed=2)
    assert min(sizes) < N
    keep = (np.arange(N)[None, :] < np.asarray(sizes)[:, None]).astype(np.float64)
    buf = eng.project_and_estimate(ctx.from_numpy(V))
    Bd, Md, grams = buf['sys'][0], buf['sys'][3], tuple(buf['grams'])
    thetas = _thetas(nmu)
    rng = np.random.default_rng(9)
    clean = rng.standard_normal((nt + 1, eng.S, N, nmu)) * keep[None, :, :, None]
    dirty = clean + 1e3 * rng.standard_normal(clean.shape) * (1.0 - keep)[None, :, :, None]

    def run(Uh):
        return _host(ctx.reduced_parabolic_estimate_batch(thetas, _coef(nmu), dt, nt, _dev(ctx, Uh), Bd, Md, grams, eng.f2, eng.ceps,
                                                          eng.hdiam))
    a, b = run(clean), run(dirty)
    assert np.array_equal(a['time_residual'], b['time_residual'])
    for k in ('eta_loc', 'time_deriv_nc', 'eta', 'est'):                    # the other forms have zero rows and columns there too
        assert _err(b[k], a[k]) <= TOL, k
    dU = np.ascontiguousarray(dirty[1:] - dirty[:-1])
    want = np.empty((nt, nmu))
    for m in range(nmu):
        want[:, m] = np.sqrt(ctx.reduced_time_residual(thetas[m], Bd, Md, _dev(ctx, dU[..., m])).sum(dim=1).cpu().numpy() * (dt / 3))
    assert _err(a['time_residual'], want) <= TOL
    ref = np.sqrt(time_residual_panel(clean, Bd.cpu().numpy(), Md.cpu().numpy(), s['nbr'], thetas).sum(axis=1) * (dt / 3))
    assert _err(a['time_residual'], ref) <= TOL


# ---------------------------------------------------------------------------------------------------------------- 7. hygiene
@pytest.mark.parametrize('N, nmu, layout, K', ((24, 17, 'factored', 0), (16, 40, 'dense', 2)))
def test_result_does_not_depend_on_the_work_buffer_and_repeats(N, nmu, layout, K):
    import torch
    eng = _system()['eng']
    ctx = eng.ctx
    nt = 2
    B, M, _ = _cut(N)
    Bd, Md = _dev(ctx, B), _dev(ctx, M)
    Ud = _dev(ctx, _panel(N, nmu, nt))
    grams = _grams(layout, N)
    kw = {}
    if K:
        F2, r_fd_K = _source(N, K)
        kw = dict(phi=_dev(ctx, np.random.default_rng(1).uniform(-1.0, 1.0, (nmu, nt + 1, K))), F2=_dev(ctx, F2),
                  r_fd_K=_dev(ctx, r_fd_K))
    inputs = [Ud, Bd, Md, eng.f2, eng.ceps] + list(grams) + list(kw.values())
    before = [t.clone() for t in inputs]

    def run():
        return ctx.reduced_parabolic_estimate_batch(_thetas(nmu), _coef(nmu), T_END / nt, nt, Ud, Bd, Md, grams, eng.f2, eng.ceps,
                                                    eng.hdiam, **kw)
    a = poisoned(ctx, run)
    b = run()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for t, t0 in zip(inputs, before):
        assert torch.equal(t, t0)


def test_installed_preconditioner_and_the_next_stationary_batch_are_untouched():
    import torch
    N, nmu, nt = 16, 17, 2
    eng = _system()['eng']
    ctx = eng.ctx
    B, M, rhs = _cut(N)
    Bd, rd = _dev(ctx, B), _dev(ctx, rhs)
    thetas = _thetas(nmu)
    Ud = _dev(ctx, _panel(N, nmu, nt))
    pc = ctx.reduced_precond_build(np.array([1.0, 0.6]), Bd)
    pc0 = pc.clone()
    free = _call(N, Ud, thetas, nt)
    ctx.reduced_precond_use(pc)
    try:
        u0, i0 = ctx.reduced_solve_batch(thetas, Bd, rd)
        used = _call(N, Ud, thetas, nt)
        u1, i1 = ctx.reduced_solve_batch(thetas, Bd, rd)
    finally:
        ctx.reduced_precond_use(None)
    assert torch.equal(pc, pc0)
    assert torch.equal(u0, u1) and i0 == i1
    for k in free:
        assert torch.equal(free[k], used[k]), k


@pytest.mark.parametrize('N, nmu', ((48, 17), (64, 40)))
def test_valu_form_of_the_matvec(N, nmu):
    ctx = _system()['eng'].ctx
    nt = 2
    Ud = _dev(ctx, _panel(N, nmu, nt))
    base = _host(_call(N, Ud, _thetas(nmu), nt))
    ctx.set_option('solve_valu', 1)
    try:
        valu = _host(_call(N, Ud, _thetas(nmu), nt))
    finally:
        ctx.set_option('solve_valu', 0)
    for k in base:
        e = _err(valu[k], base[k])
        print('PARABOLIC-ESTIMATE-BATCH VALU N={} nmu={} {}: {:.2e}'.format(N, nmu, k, e))
        assert e <= TOL, k


def test_refusals_before_any_launch():
    from common import theta_bar_of
    from pylrbms_amd import multiscale_problem
    from pylrbms_amd._native import NativeError
    from pylrbms_amd.engine import Engine
    eng = _system()['eng']
    ctx, S = eng.ctx, eng.S
    N = 8
    B, M, _ = _cut(N)
    Bd, Md = _dev(ctx, B), _dev(ctx, M)
    gf, gd = _grams('factored', N), _grams('dense', N)

    def call(c, nmu, dt, nt, Bx=Bd, Mx=Md, grams=gf, n=N, thetas=None):
        th = _thetas(nmu) if thetas is None else thetas
        out = c.reduced_parabolic_estimate_batch(th, np.ones((th.shape[0], 2)), dt, nt, c.zeros(max(nt, 0) + 1, c.S, n, th.shape[0]),
                                                 Bx, Mx, grams, c.zeros(c.S), c.zeros(c.S) + 1.0, 1.0)
        c.torch.cuda.synchronize()
        return out

    call(ctx, 3, 0.01, 1)                                                   # the arguments below are otherwise fine
    call(ctx, 3, 0.01, 1, grams=gd)
    with pytest.raises(NativeError):
        call(ctx, 65, 0.01, 1)
    with pytest.raises(NativeError):
        call(ctx, 3, 0.0, 1)
    with pytest.raises(NativeError):
        call(ctx, 3, 0.01, 0)
    with pytest.raises(NativeError):                                        # N = 65
        g65 = (ctx.zeros(S, 5 * 65, 5 * 65), ctx.zeros(S, 5 * Q * 65), ctx.zeros(S, 9, Q * 65, Q * 65), ctx.zeros(S, 9, Q * 65, Q * 65),
               ctx.zeros(Q, S, 65, 5 * Q * 65), ctx.zeros(Q, Q, S, 65, 65))
        call(ctx, 3, 0.01, 1, ctx.zeros(Q, S, 5, 65, 65), ctx.zeros(S, 65, 65), g65, n=65)
    with pytest.raises(NativeError):                                        # Q = 5 with more than 16 columns
        g5 = (ctx.zeros(S, 5 * N, 5 * N), ctx.zeros(S, 25 * N), ctx.zeros(S, 9, 5 * N, 5 * N), ctx.zeros(S, 9, 5 * N, 5 * N),
              ctx.zeros(5, S, N, 25 * N), ctx.zeros(5, 5, S, N, N))
        call(ctx, 17, 0.01, 1, ctx.zeros(5, S, 5, N, N), grams=g5, thetas=np.ones((17, 5)))
    # F_side and F_nc go together (below the wrapper, which always passes both or neither)
    from pylrbms_amd._native import _dblp, c_vp
    th, cf = _thetas(3), np.ones((3, 2))
    U = ctx.zeros(2, S, N, 3)
    work = ctx.empty(int(ctx.lib.lrbms_reduced_parabolic_estimate_batch_work_size(ctx.handle, N, 3, 1)))
    outs = [ctx.zeros(3, 2, S, 3), ctx.zeros(1, S, 3), ctx.zeros(1, 3), ctx.zeros(2, 3), ctx.zeros(3)]
    ptrs = [c_vp(t.data_ptr()) for t in gf]
    ptrs[7] = c_vp(None)
    rc = ctx.lib.lrbms_reduced_parabolic_estimate_batch(
        ctx.handle, Q, N, 0, 3, 1, 0.01, _dblp(th), _dblp(cf), 0, c_vp(U.data_ptr()), c_vp(Bd.data_ptr()), c_vp(Md.data_ptr()), *ptrs,
        c_vp(eng.f2.data_ptr()), c_vp(eng.ceps.data_ptr()), float(eng.hdiam), c_vp(None), c_vp(None), c_vp(None),
        c_vp(work.data_ptr()), *[c_vp(t.data_ptr()) for t in outs], ctx._stream())
    ctx.torch.cuda.synchronize()
    assert rc != 0 and all(float(t.abs().max()) == 0.0 for t in outs)       # refused, nothing was written

    class TwoRanks:
        rank, size = 0, 2

    p = multiscale_problem.init_grid_and_problem({'num_subdomains': list(SWEEP_GRID), 'coarse_per_subdomain': KC}, mpi_comm=TwoRanks())
    lam = p['lambda']
    sharded = Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar_of(p))
    c2, S2 = sharded.ctx, sharded.S
    assert sharded.S_ext > S2
    g2 = (c2.zeros(S2, 5 * N, 5 * N), c2.zeros(S2, 5 * Q * N), c2.zeros(S2, 9, Q * N, Q * N), c2.zeros(S2, 9, Q * N, Q * N),
          c2.zeros(Q, S2, N, 5 * Q * N), c2.zeros(Q, Q, S2, N, N))
    with pytest.raises(NativeError, match='one rank'):
        call(c2, 3, 0.01, 1, c2.zeros(Q, S2, 5, N, N), c2.zeros(S2, N, N), g2)


def test_vertex_patch_needs_the_factored_layout():
    from common import theta_bar_of
    from pylrbms_amd import multiscale_problem
    from pylrbms_amd._native import NativeError
    from pylrbms_amd.engine import Engine
    p = multiscale_problem.init_grid_and_problem({'num_subdomains': [3, 3], 'coarse_per_subdomain': KC})
    lam = p['lambda']
    eng = Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar_of(p),
                 conventions={'oswald_vertex_patch': True})
    c, S, N = eng.ctx, eng.S, 4
    dense = (c.zeros(S, 5 * N, 5 * N), c.zeros(S, 5 * Q * N), c.zeros(S, 9, Q * N, Q * N), c.zeros(S, 9, Q * N, Q * N),
             c.zeros(Q, S, N, 5 * Q * N), c.zeros(Q, Q, S, N, N))
    with pytest.raises(NativeError, match='factored'):
        c.reduced_parabolic_estimate_batch(_thetas(3), np.ones((3, 2)), 0.01, 1, c.zeros(2, S, N, 3), c.zeros(Q, S, 5, N, N),
                                           c.zeros(S, N, N), dense, c.zeros(S), c.zeros(S) + 1.0, 1.0)


# ------------------------------------------------------------------------------------------------------- 1. / 5. Python surface
def _reduced_model(name, **kw):
    from pylrbms_amd import OS2015_academic_problem, artificial_channels_problem, multiscale_problem
    from pylrbms_amd.discretize_parabolic_block_swipdg import discretize
    from pylrbms_amd.reductor import ParabolicLRBMSReductor
    if name == 'os2015':
        p = OS2015_academic_problem.init_grid_and_problem({'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 4})
        T, nt, mu_values = 0.5, 4, (0.2, 0.5, 0.9)
    elif name == 'channels':
        p = artificial_channels_problem.init_grid_and_problem({'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 8})
        T, nt, mu_values = 1.0, 4, (0.1, 0.5, 0.9)
    else:
        p = multiscale_problem.init_grid_and_problem({'num_subdomains': [3, 3], 'coarse_per_subdomain': 2})
        T, nt, mu_values = 0.05, 3, (0.2, 0.5, 0.9)
    d, d_data = discretize(p, T, nt, **kw)
    reductor = ParabolicLRBMSReductor(
        d, products=[d.operators['local_energy_dg_product_{}'.format(ii)] for ii in range(d_data['block_space'].num_blocks)])
    snap_idx = [1, nt // 2, nt]
    U = d.solve(d.parse_parameter(mu_values[1]))
    reductor.extend_basis(U[snap_idx])
    return p, d, reductor, reductor.reduce(), T, nt, mu_values, snap_idx, U


def _compare(got, want, tol, tag):
    (est, parts), (est_w, parts_w) = got, want
    assert len(parts) == len(parts_w) == 5
    worst = 0.0
    for nm, a, b in zip(PARTS, parts, parts_w):
        assert isinstance(a, np.ndarray)
        e = _err(a, b)
        worst = max(worst, e)
        assert e < tol, (tag, nm, e)
    assert abs(est - est_w) < tol * est_w, (tag, est, est_w)
    return worst


@pytest.mark.parametrize('name', ('os2015', 'channels'))
def test_estimate_batch_of_the_parabolic_reduced_model(name):
    """``rd.estimate_batch(rd.solve_batch(mus), mus)`` for three parameters: against ``OracleParabolicReduced.estimate`` where the
    oracle has the model (os2015; the setup and the 1e-6 of tests/test_parabolic_gpu.py) and against ``rd.estimate`` per
    trajectory (both problems; the two run the same forms in different kernels and orders: 1e-10)."""
    from common import oracle_from_problem
    from oracle.lrbms import OracleReductor
    from oracle.parabolic import OracleParabolic, OracleParabolicReduced
    p, d, reductor, rd, T, nt, mu_values, snap_idx, U = _reduced_model(name)
    assert (rd.rhs_red_K is not None) == (name == 'channels')
    mus = [d.parse_parameter(v) for v in mu_values]
    Us = rd.solve_batch(mus)
    assert Us[0].tensor._base is Us[1].tensor._base                         # views of ONE panel ...
    assert rd._panel_of(Us).data_ptr() == Us[0].tensor._base.data_ptr()     # ... which estimate_batch takes without a copy
    out = rd.estimate_batch(Us, mus)
    assert isinstance(out, list) and len(out) == len(mus)
    N = reductor.basis_size()
    S = d.engine.S
    for (est, parts), U_m, mu in zip(out, Us, mus):
        assert parts[0].shape == (S, nt + 1) and parts[3].shape == (nt,) and parts[4].shape == (S, nt) and est > 0.0
        worst = _compare((est, parts), rd.estimate(U_m, mu), TOL, (name, 'rd.estimate'))
        print('PARABOLIC-ESTIMATE-BATCH estimate_batch {} mu={}: worst part vs rd.estimate {:.2e}'.format(name, mu, worst))
    # a panel tensor and a list of copies (stacked) give the same result
    panel = Us[0].tensor._base
    again = rd.estimate_batch(panel, mus)
    copies = rd.estimate_batch([type(U_m)(U_m.tensor.clone()) for U_m in Us], mus)
    for a, b, c in zip(out, again, copies):
        assert a[0] == b[0] == c[0] and all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a[1], b[1], c[1]))
    if name == 'os2015':
        o = oracle_from_problem(p)
        U_ref = OracleParabolic(o, T, nt).solve(mu_values[1])
        bases = [np.stack([np.ones(o.n)] + [U_ref[k, ii] for k in snap_idx], axis=1) for ii in range(o.S)]
        ored = OracleReductor(o, bases)
        opr = OracleParabolicReduced(ored, ored.reduce(), T, nt)
        for got, mu_v in zip(out, mu_values):
            worst = _compare(got, opr.estimate(opr.solve(mu_v), mu_v), 1e-6, (name, 'oracle'))
            print('PARABOLIC-ESTIMATE-BATCH estimate_batch {} mu={}: worst part vs the oracle {:.2e}'.format(name, mu_v, worst))


def test_estimate_batch_falls_back_and_refuses():
    p, d, reductor, rd, T, nt, mu_values, _, _ = _reduced_model('os2015')
    mus = [d.parse_parameter(v) for v in mu_values]
    Us = rd.solve_batch(mus)
    d.estimator.elliptic_reconstruction = True
    try:
        out = rd.estimate_batch(Us, mus)
        for got, U_m, mu in zip(out, Us, mus):
            _compare(got, rd.estimate(U_m, mu), 1e-14, 'elliptic_reconstruction')
    finally:
        d.estimator.elliptic_reconstruction = False
    eng = d.engine
    S_ext = eng.S_ext
    eng.S_ext = eng.S + 1                                                   # what a sharded discretization looks like to the method
    try:
        with pytest.raises(NotImplementedError, match='S_ext == S'):
            rd.estimate_batch(Us, mus)
    finally:
        eng.S_ext = S_ext


def test_estimate_batch_with_the_oswald_vertex_patch():
    p, d, reductor, rd, T, nt, mu_values, _, _ = _reduced_model('multiscale', conventions={'oswald_vertex_patch': True})
    assert len(rd.grams) == 8
    mus = [d.parse_parameter(v) for v in mu_values]
    rng = np.random.default_rng(4)
    Us = rd.solve_batch(mus)
    panel = Us[0].tensor._base
    panel += 0.3 * float(panel.abs().max()) * d.engine.ctx.from_numpy(rng.standard_normal(tuple(panel.shape)))
    out = rd.estimate_batch(Us, mus)
    for got, U_m, mu in zip(out, Us, mus):
        worst = _compare(got, rd.estimate(U_m, mu), TOL, 'vertex patch')
        print('PARABOLIC-ESTIMATE-BATCH vertex patch mu={}: worst part vs rd.estimate {:.2e}'.format(mu, worst))
    # the corner terms are seen: without the patch the nonconformity parts differ
    _, _, _, rd0, _, _, _, _, _ = _reduced_model('multiscale')
    plain = rd0.estimate_batch(panel, mus)
    assert _err(plain[0][1][0], out[0][1][0]) > 1e-6


# ------------------------------------------------------------------------------------------------------ 8. small API pieces
@pytest.mark.parametrize('affine', (False, True))
def test_stationary_estimate_batch_is_the_loop_of_estimate(affine):
    from pylrbms_amd import OS2015_academic_problem
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    from pylrbms_amd.reductor import LRBMSReductor, ReducedVectorArray
    if affine:
        from affine_source_ref import make_problem
        p = make_problem({'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 4})
    else:
        p = OS2015_academic_problem.init_grid_and_problem({'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 4})
    d, data = discretize(p)
    reductor = LRBMSReductor(d, products=[d.operators['local_energy_dg_product_{}'.format(ii)]
                                          for ii in range(data['block_space'].num_blocks)])
    for v in ([0.2], [0.7], [1.0]):
        reductor.extend_basis(d.solve(d.parse_parameter(v)))
    rd = reductor.reduce()
    assert rd._affine() == affine
    mus = [d.parse_parameter(v) for v in ([0.15], [0.4], [0.8], [0.95])]
    U = rd.solve_batch(mus)
    cols = [ReducedVectorArray(U.tensor[:, :, m:m + 1].contiguous()) for m in range(len(mus))]
    for decompose in (False, True):
        out = rd.estimate_batch(U, mus, decompose=decompose)
        as_list = rd.estimate_batch(cols, mus, decompose=decompose)
        as_tensor = rd.estimate_batch(U.tensor.permute(2, 0, 1).contiguous(), mus, decompose=decompose)
        assert len(out) == len(mus)
        for m, mu in enumerate(mus):
            want = rd.estimate(cols[m], mu, decompose=decompose)
            for got in (out[m], as_list[m], as_tensor[m]):
                if not decompose:
                    assert abs(got - want) <= TOL * want and want > 0.0
                    continue
                assert abs(got[0] - want[0]) <= TOL * want[0]
                for a, b in zip(got[1], want[1]):
                    assert _err(a, b) <= TOL
                assert _err(got[2], want[2]) <= TOL


def test_instationary_3d_estimate_batch_is_the_loop_of_estimate():
    import common3d as c3
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D, discretize
    from test_parabolic3d_gpu import _pd
    p = c3.make_problem('aniso_2x2x1')
    T, nt = 0.75, 3
    d, _ = discretize(_pd(p), T, nt)
    reductor = ParabolicLRBMSReductor3D(d)
    reductor.extend_basis(d.solve(p['mu'])[:, :, [1, 2, nt]])
    rd = reductor.reduce()
    mus = [0.2, p['mu'], 0.9]
    U = rd.solve_batch(mus)
    out = rd.estimate_batch(U, mus)
    assert len(out) == len(mus)
    for m, mu in enumerate(mus):
        est, parts = rd.estimate(U[m], mu)
        assert out[m][0] == est and est > 0.0
        for a, b in zip(out[m][1], parts):
            assert np.array_equal(np.asarray(a), np.asarray(b))
