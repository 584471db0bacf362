"""Batched parabolic estimates of the 3D / P2 path on the GPU: lrbms3_reduced_parabolic_estimate_batch -- the
parabolic estimate of nmu <= 64 reduced trajectories of one panel U [nt + 1, S, N, nmu] per call -- against the existing exports
slab by slab (lrbms3_reduced_estimate_batch on U[k] and on U[k+1] - U[k], lrbms3_reduced_time_residual per column,
lrbms3_reduced_source_terms), against the NumPy restatement tests/parabolic_estimate_batch3d_ref.py (pinned to the 3D references in
tests/test_parabolic_estimate_batch3d_host.py) on the dense operators ``expand_factored`` makes of the pass's arrays, and through
``InstationaryReducedDiscretization3D.estimate_batch(native=True)``.

Squared quantities are compared (time_deriv_nc^2 dt, time_residual^2 3 / dt: the square roots amplify round-off near zero), each
to TOL = 1e-10 of the largest entry of its output -- the bound of the 2D twin's tests.  Cells and inputs: ``ref.CELLS``, ``ref.panel``,
``ref.coefficients``, ``ref.cell_thetas`` (the host test runs its mutants on the same inputs)."""
import ctypes

import numpy as np
import pytest

import common3d as c3
import parabolic_estimate_batch3d_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-10
DT = ref.DT
E_INVALID = -1
OUTS = ('eta_loc', 'time_deriv_nc', 'time_residual', 'eta', 'est')

_ENG = {}
_SYS = {}


def _engine(name):
    if name not in _ENG:
        from pylrbms_amd.engine3d import Engine3D
        p = c3.make_problem(name)
        _ENG[name] = (p, Engine3D(p['grid'], p['lambdas'], p['f'], p['lambda_bar'], p['lambda_hat'],
                                  theta_bar=c3.theta_of(p, p['mu_bar'])).assemble())
    return _ENG[name]


def _system(name, N, pad=0):
    """Engine, the factored arrays of a pass on ``make_bases3d`` bases with N columns, M_red and the host model of the restatement.
    pad > 0: the last ``pad`` basis columns of subdomain 1 are zero (a ragged basis, zero-padded)."""
    key = (name, N, pad)
    if key not in _SYS:
        from pylrbms_amd.engine3d import expand_factored
        p, eng = _engine(name)
        V = c3.make_bases3d(eng.S, eng.ctx.n, N, seed=ref.BASIS_SEED)
        keep = np.ones((eng.S, N), dtype=bool)
        if pad:
            V[1, :, N - pad:] = 0.0
            keep[1, N - pad:] = False
        Vd = eng.ctx.from_numpy(V)
        out = eng.project_and_estimate(Vd)
        M = eng.ctx.project_mass(Vd)
        Q = len(p['lambdas'])
        dense = {k: v.cpu().numpy() for k, v in expand_factored(eng, out, Q, N).items()}
        model = dict(dense, nbr=np.asarray(eng.nbr).reshape(eng.S, 7), M_red=M.cpu().numpy(), f2=eng.ops['f2'].cpu().numpy(),
                     ceps=eng.ops['ceps'].cpu().numpy(), hdiam=float(eng.hdiam))
        _SYS[key] = dict(p=p, eng=eng, ctx=eng.ctx, Q=Q, N=N, S=eng.S, out=out, M=M, model=model, keep=keep)
    return _SYS[key]


def _call(s, thetas, coef, U, nt, out=None, ops=None, **kw):
    """The export through its wrapper on the host panel U -> dict of host arrays."""
    ctx = s['ctx']
    Ud = U if hasattr(U, 'data_ptr') else ctx.from_numpy(np.ascontiguousarray(U))
    r = ctx.reduced_parabolic_estimate_batch(s['Q'], thetas, coef, DT, nt, Ud, s['out']['B_sys'], s['M'], s['out'] if out is None else out,
                                             s['eng'].ops if ops is None else ops, s['eng'].hdiam, **kw)
    ctx.torch.cuda.synchronize()
    return r


def _host(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _check(got, want, tag):
    miss = ref.worst(got, want, DT)
    print('PEB3D {}: '.format(tag) + ', '.join('{} {:.2e}'.format(k, v) for k, v in miss.items()))
    for k, v in miss.items():
        assert np.isfinite(v) and v <= TOL, (tag, k, v)
    return miss


# ----------------------------------------------------------------------------------- against the existing exports and NumPy
@pytest.mark.parametrize('name, N, nmu, nt', ref.CELLS)
def test_outputs_against_the_slab_exports_and_the_restatement(name, N, nmu, nt):
    s = _system(name, N)
    ctx, Q, S, eng = s['ctx'], s['Q'], s['S'], s['eng']
    U = ref.panel(S, N, nmu, nt)
    thetas, coef = ref.cell_thetas(s['p'], nmu), ref.coefficients(nmu)
    got = _host(_call(s, thetas, coef, U, nt))
    assert got['eta_loc'].shape == (3, nt + 1, S, nmu) and got['time_deriv_nc'].shape == (nt, S, nmu)
    assert got['time_residual'].shape == (nt, nmu) and got['eta'].shape == (nt + 1, nmu) and got['est'].shape == (nmu,)
    assert all(np.isfinite(got[k]).all() for k in OUTS) and got['est'].min() > 0.0
    # ---- the NumPy restatement on the expanded operators; its nc(dU) is not near the clamp
    want = ref.estimate_outputs(s['model'], thetas, coef, DT, U)
    assert want['nc_dU'].min() >= -1e-12 * want['nc_dU'].max() and want['nc_dU'].max() > 0.0
    _check(got, want, '{} N={} nmu={} nt={} numpy'.format(name, N, nmu, nt))
    # ---- slab by slab: the batched estimate on U[k] and on dU[k], the time residual per column
    sc = 2.0 * np.sqrt(DT / 3.0)
    Ud = ctx.from_numpy(U)
    dUd = (Ud[1:] - Ud[:-1]).contiguous()
    rows = np.stack([ctx.reduced_estimate_batch(Q, thetas, Ud[k].contiguous(), s['out'], eng.ops, eng.hdiam).cpu().numpy()
                     for k in range(nt + 1)], axis=1)                                     # [3, nt + 1, S, nmu]
    ncd = np.stack([ctx.reduced_estimate_batch(Q, thetas, dUd[k], s['out'], eng.ops, eng.hdiam)[0].cpu().numpy() for k in range(nt)])
    tr2 = np.stack([ctx.reduced_time_residual(Q, thetas[m], s['out']['B_sys'], s['M'], dUd[:, :, :, m].contiguous()).sum(dim=1).cpu().numpy()
                    for m in range(nmu)], axis=1)                                         # [nt, nmu]
    e = {'eta_loc': c3.rel(got['eta_loc'], rows * sc), 'tdnc2': c3.rel(got['time_deriv_nc'] ** 2 * DT, np.maximum(ncd, 0.0)),
         'tr2': c3.rel(got['time_residual'] ** 2 * 3.0 / DT, tr2)}
    print('PEB3D {} N={} nmu={} nt={} exports: '.format(name, N, nmu, nt) + ', '.join('{} {:.2e}'.format(k, v) for k, v in e.items()))
    assert all(v <= TOL for v in e.values()), e


# --------------------------------------------------------------------------------------------------------- theta per column
def test_swapped_columns_swap_the_bits_and_a_zero_column_gives_zeros():
    """Columns 2 and 20 (two different passes) exchanged in theta, coef and U: the output columns exchange their bits.  A zero
    column of U: exact zeros in time_deriv_nc, time_residual and the nc and df rows of eta_loc; its r row is the f2 term of the
    estimate, bit for bit what lrbms3_reduced_estimate_batch gives for a zero column -- and exactly zero with zeroed f terms."""
    name, N, nmu, nt = 'interior_3x3x3', 17, 33, 3
    s = _system(name, N)
    ctx, eng, S = s['ctx'], s['eng'], s['S']
    U = ref.panel(S, N, nmu, nt)
    U[..., 7] = 0.0
    thetas, coef = ref.cell_thetas(s['p'], nmu), ref.coefficients(nmu)
    a = _host(_call(s, thetas, coef, U, nt))
    perm = np.arange(nmu)
    perm[[2, 20]] = [20, 2]
    b = _host(_call(s, thetas[perm], coef[perm], np.ascontiguousarray(U[..., perm]), nt))
    for k in OUTS:
        assert np.array_equal(a[k][..., perm], b[k]), k
    assert not np.array_equal(a['est'][2], a['est'][20])
    assert np.all(a['time_deriv_nc'][..., 7] == 0.0) and np.all(a['time_residual'][:, 7] == 0.0)
    assert np.all(a['eta_loc'][0, ..., 7] == 0.0) and np.all(a['eta_loc'][2, ..., 7] == 0.0)
    zero = ctx.reduced_estimate_batch(s['Q'], thetas, ctx.zeros(S, N, nmu), s['out'], eng.ops, eng.hdiam).cpu().numpy()
    sc = 2.0 * np.sqrt(DT / 3.0)
    assert np.array_equal(a['eta_loc'][1, 0, :, 7], zero[1, :, 7] * sc) and np.abs(zero[1, :, 7]).min() > 0.0
    from pylrbms_amd.sources3d import zeroed
    out0, ops0 = zeroed(eng, s['out'])
    z = _host(_call(s, thetas, coef, U, nt, out=out0, ops=ops0))
    assert np.all(z['eta_loc'][..., 7] == 0.0) and np.all(z['eta'][:, 7] == 0.0) and z['est'][7] == 0.0


# ---------------------------------------------------------------------------------------------------------------------- source
def _source(s, K, nmu, nt, seed=5):
    """Synthetic source data of K components on the system s: F2 [S, K, K] (SPD per subdomain), r_fd_K [K, S, QN], bdiv_K [K, S, n_T]
    and phi [nmu, nt + 1, K] whose first component switches between 0 and 1 from row to row."""
    rng = np.random.default_rng(seed)
    S, QN, nT = s['S'], s['Q'] * s['N'], s['ctx'].n_T
    G = rng.standard_normal((S, K, K))
    F2 = np.einsum('sij,skj->sik', G, G) + K * np.eye(K)[None]
    phi = rng.uniform(0.5, 1.5, size=(nmu, nt + 1, K))
    phi[:, :, 0] = (np.arange(nt + 1)[None, :] + np.arange(nmu)[:, None]) % 2
    return F2, rng.standard_normal((K, S, QN)), rng.standard_normal((K, S, nT)), np.ascontiguousarray(phi)


def test_source_terms_against_the_column_loop_of_the_source_export():
    """K = 3 with a switching coefficient: the r rows are those of the estimate without f terms plus lrbms3_reduced_source_terms
    of U[k] with row k of the table, column by column."""
    from pylrbms_amd.sources3d import zeroed
    name, N, nmu, nt, K = 'interior_3x3x3', 5, 17, 3, 3
    s = _system(name, N)
    ctx, eng, Q, S = s['ctx'], s['eng'], s['Q'], s['S']
    F2, r_fd_K, bdiv_K, phi = _source(s, K, nmu, nt)
    F2d, rKd, bKd = (ctx.from_numpy(np.ascontiguousarray(x)) for x in (F2, r_fd_K, bdiv_K))
    U = ref.panel(S, N, nmu, nt)
    thetas, coef = ref.cell_thetas(s['p'], nmu), ref.coefficients(nmu)
    out0, ops0 = zeroed(eng, s['out'])
    got = _host(_call(s, thetas, coef, U, nt, out=out0, ops=ops0, phi=phi, F2=F2d, r_fd_K=rKd, bdiv_K=bKd))
    base = _host(_call(s, thetas, coef, U, nt, out=out0, ops=ops0))
    Ud = ctx.from_numpy(U)
    add = np.zeros((nt + 1, S, nmu))
    for k in range(nt + 1):
        for m in range(nmu):
            add[k, :, m] = ctx.reduced_source_terms(Q, thetas[m:m + 1], phi[m, k:k + 1], F2d, rKd, bKd, s['out']['Rb'],
                                                    Ud[k, :, :, m:m + 1].contiguous(), eng.ops['ceps'], eng.hdiam).cpu().numpy()[:, 0]
    sc = 2.0 * np.sqrt(DT / 3.0)
    want_r = base['eta_loc'][1] + add * sc
    e_r = c3.rel(got['eta_loc'][1], want_r)
    # eta from the rows: the norms of the raw rows over the subdomains
    raw = got['eta_loc'] / sc
    eta = sc * (coef[None, :, 0] * np.linalg.norm(raw[0], axis=1) + coef[None, :, 1] * np.linalg.norm(raw[1] + raw[2], axis=1))
    e_eta = c3.rel(got['eta'], eta)
    print('PEB3D source K=3: r rows {:.2e}, eta {:.2e}'.format(e_r, e_eta))
    assert np.abs(add).max() > 0.0 and e_r <= TOL and e_eta <= TOL
    for k in ('time_deriv_nc', 'time_residual'):
        assert np.array_equal(got[k], base[k]), k
    assert np.array_equal(got['eta_loc'][[0, 2]], base['eta_loc'][[0, 2]])


def test_one_source_component_with_unit_coefficient_is_the_plain_call():
    """K = 1, phi = 1 with the discretization's own f2 / r_fd / bdiv as the component: the call with K = 0, to 1e-10."""
    from pylrbms_amd.sources3d import zeroed
    name, N, nmu, nt = 'aniso_2x2x1', 4, 16, 3
    s = _system(name, N)
    ctx, eng, S = s['ctx'], s['eng'], s['S']
    U = ref.panel(S, N, nmu, nt)
    thetas, coef = ref.cell_thetas(s['p'], nmu), ref.coefficients(nmu)
    plain = _host(_call(s, thetas, coef, U, nt))
    out0, ops0 = zeroed(eng, s['out'])
    got = _host(_call(s, thetas, coef, U, nt, out=out0, ops=ops0, phi=np.ones((nmu, nt + 1, 1)), F2=eng.ops['f2'].reshape(S, 1, 1).contiguous(),
                      r_fd_K=s['out']['r_fd'][None].contiguous(), bdiv_K=eng.ops['bdiv'][None].contiguous()))
    _check(got, plain, 'K=1 phi=1 against K=0')


# -------------------------------------------------------------------------------------------------------------- ragged bases
def test_zero_padded_basis_columns_give_the_outputs_of_the_unpadded_model():
    """Subdomain 1 keeps N - 2 vectors, zero-padded: the restatement on the kept unknowns (M_red inverted there only) to 1e-10,
    with arbitrary coefficients on the padded unknowns -- they do not contribute."""
    name, N, nmu, nt = 'interior_3x3x3', 16, 15, 3
    s = _system(name, N, pad=2)
    U = ref.panel(s['S'], N, nmu, nt)
    thetas, coef = ref.cell_thetas(s['p'], nmu), ref.coefficients(nmu)
    got = _host(_call(s, thetas, coef, U, nt))
    U0 = U.copy()
    U0[:, 1, N - 2:, :] = 0.0
    want = ref.estimate_outputs(s['model'], thetas, coef, DT, U0, keep=s['keep'])
    _check(got, want, 'ragged (padded coefficients arbitrary)')
    _check(_host(_call(s, thetas, coef, U0, nt)), want, 'ragged (padded coefficients zero)')


# ------------------------------------------------------------------------------------------------------- buffers and repeats
def _banded(ctx, a):
    """A device copy of ``a`` between two NaN bands -> (view, whole buffer)."""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64)
    big = torch.full((a.size + 128,), float('nan'), dtype=torch.float64, device=ctx.device)
    big[64:64 + a.size] = ctx.from_numpy(a.reshape(-1))
    return big[64:64 + a.size].view(a.shape), big


def test_poisoned_work_guard_bands_repeats_and_untouched_inputs():
    """work and outputs NaN-filled between sentinel bands (tests/test_work_poison_gpu.py), the device inputs between NaN bands: the
    NaN-filled run gives the bits of the zero-filled one, two calls give the same bits, the bands are intact and the inputs
    unchanged.  With a source, so that every stage writes."""
    import torch
    from test_work_poison_gpu import poisoned
    from pylrbms_amd.sources3d import zeroed
    name, N, nmu, nt, K = 'interior_3x3x3', 17, 33, 3, 2
    s = _system(name, N)
    ctx, eng = s['ctx'], s['eng']
    F2, r_fd_K, bdiv_K, phi = _source(s, K, nmu, nt)
    thetas, coef = ref.cell_thetas(s['p'], nmu), ref.coefficients(nmu)
    out0, ops0 = zeroed(eng, s['out'])
    ins = {k: _banded(ctx, v) for k, v in dict(U=ref.panel(s['S'], N, nmu, nt), phi=phi, F2=F2, r_fd_K=r_fd_K, bdiv_K=bdiv_K,
                                               B_sys=s['out']['B_sys'].cpu().numpy(), M=s['M'].cpu().numpy()).items()}
    before = {k: big.clone() for k, (_, big) in ins.items()}
    facts = {k: out0[k].clone() for k in ('G_nc', 'As', 'Cn', 'Rb', 'G_bb')}

    def run():
        r = ctx.reduced_parabolic_estimate_batch(s['Q'], thetas, coef, DT, nt, ins['U'][0], ins['B_sys'][0], ins['M'][0], out0, ops0,
                                                 eng.hdiam, phi=ins['phi'][0], F2=ins['F2'][0], r_fd_K=ins['r_fd_K'][0],
                                                 bdiv_K=ins['bdiv_K'][0])
        torch.cuda.synchronize()
        return r

    first = poisoned(ctx, run)
    second = run()
    for k in OUTS:
        assert torch.equal(first[k], second[k]), k
        assert bool(torch.isfinite(first[k]).all()), k
    for k, (_, big) in ins.items():
        assert torch.equal(big.view(torch.int64), before[k].view(torch.int64)), k
    for k, v in facts.items():
        assert torch.equal(out0[k], v), k


def test_installed_preconditioner_and_the_next_stationary_batch_are_untouched():
    import torch
    name, N, nmu, nt = 'interior_3x3x3', 17, 17, 1
    s = _system(name, N)
    ctx, Q = s['ctx'], s['Q']
    thetas, coef = ref.cell_thetas(s['p'], nmu), ref.coefficients(nmu)
    U = ref.panel(s['S'], N, nmu, nt)
    B, rhs = s['out']['B_sys'], s['out']['rhs_red']
    pc = ctx.reduced_precond_build(Q, c3.theta_of(s['p'], 0.6), B)
    pc0 = pc.clone()
    free = _call(s, thetas, coef, U, nt)
    ctx.reduced_precond_use(pc)
    try:
        u0, i0 = ctx.reduced_solve_batch(Q, thetas, B, rhs, rtol=1e-12)
        got = _call(s, thetas, coef, U, nt)
        u1, i1 = ctx.reduced_solve_batch(Q, thetas, B, rhs, rtol=1e-12)
    finally:
        ctx.reduced_precond_use(None)
    assert torch.equal(pc, pc0) and torch.equal(u0, u1) and i0 == i1
    for k in OUTS:
        assert torch.equal(got[k], free[k]), k


# ------------------------------------------------------------------------------------------------------------------ VALU forms
@pytest.mark.parametrize('option', ('estimate_valu', 'solve_valu'))
@pytest.mark.parametrize('name, N, nmu, nt', (('interior_3x3x3', 17, 33, 1), ('q3_2x1x2', 6, 33, 3)))
def test_valu_forms_agree_with_the_matrix_core_forms(option, name, N, nmu, nt):
    """LRBMS3_OPT_ESTIMATE_VALU = 1 (the VALU estimate on every slab and row 0 of it for the differences) and
    LRBMS3_OPT_SOLVE_VALU = 1 (the VALU panel matvec of the time residual), each against the default to 1e-10."""
    s = _system(name, N)
    ctx = s['ctx']
    U = ref.panel(s['S'], N, nmu, nt)
    thetas, coef = ref.cell_thetas(s['p'], nmu), ref.coefficients(nmu)
    mfma = _host(_call(s, thetas, coef, U, nt))
    ctx.set_option(option, 1)
    try:
        valu = _host(_call(s, thetas, coef, U, nt))
    finally:
        ctx.set_option(option, 0)
    _check(valu, mfma, '{} {} N={}'.format(option, name, N))
    assert any(not np.array_equal(valu[k], mfma[k]) for k in OUTS)          # the option reached a kernel of the call


# -------------------------------------------------------------------------------------------------------------------- refusals
def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(None)


def _dblp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if a is not None else ctypes.POINTER(ctypes.c_double)()


def test_refusals_before_any_launch():
    """Every limit and every null pointer: LRBMS_E_INVALID, outputs and work untouched; a valid call succeeds afterwards."""
    name, N, nmu, nt, K = 'interior_3x3x3', 5, 3, 2, 2
    s = _system(name, N)
    ctx, eng, Q, S = s['ctx'], s['eng'], s['Q'], s['S']
    F2, r_fd_K, bdiv_K, phi = _source(s, K, 65, nt + 1)
    thetas, coef = ref.cell_thetas(s['p'], 65), ref.coefficients(65)
    names = ('G_nc', 'G_bb', 'G_rdd', 'G_ab', 'G_aa', 'r_fd', 'Rb', 'Yb', 'Dp', 'Xab', 'As', 'Cn')
    dev = [ctx.from_numpy(ref.panel(S, 33, 65, nt + 1)), s['out']['B_sys'], s['M']] + [s['out'][k] for k in names]
    dev += [eng.ops[k] for k in ('ebar', 'Bbb', 'bdiv', 'f2', 'ceps')]
    srcs = [ctx.from_numpy(x) for x in (phi, np.ascontiguousarray(F2), r_fd_K, bdiv_K)]
    poison = float(np.pi)
    size = int(ctx.lib.lrbms3_reduced_parabolic_estimate_batch_work_size(ctx.handle, 32, 64, nt + 1))
    bufs = [ctx.empty(size), ctx.empty(3, nt + 2, S, 65), ctx.empty(nt + 1, S, 65), ctx.empty(nt + 1, 65), ctx.empty(nt + 2, 65),
            ctx.empty(65)]
    for b in bufs:
        b.fill_(poison)

    def call(Q_=Q, N_=N, K_=0, nmu_=nmu, nt_=nt, dt=DT, th=thetas, cf=coef, drop=None, src=(None,) * 4, drop_buf=None):
        d = [None if i == drop else t for i, t in enumerate(dev)]
        b = [None if i == drop_buf else t for i, t in enumerate(bufs)]
        rc = ctx.lib.lrbms3_reduced_parabolic_estimate_batch(ctx.handle, Q_, N_, K_, nmu_, nt_, dt, _dblp(th), _dblp(cf), *[_vp(t) for t in d],
                                                             float(eng.hdiam), *[_vp(t) for t in src], *[_vp(t) for t in b],
                                                             ctx._stream())
        ctx.torch.cuda.synchronize()
        return rc

    bad = [call(Q_=0), call(Q_=9), call(N_=0), call(N_=33), call(Q_=4, N_=17), call(nmu_=0), call(nmu_=65), call(nt_=0), call(dt=0.0),
           call(dt=-1.0), call(dt=float('nan')), call(K_=-1), call(K_=65, src=srcs), call(th=None), call(cf=None)]
    bad += [call(drop=i) for i in range(len(dev))] + [call(drop_buf=i) for i in range(len(bufs))]
    bad += [call(K_=K, src=[None if i == j else t for i, t in enumerate(srcs)]) for j in range(4)]        # K >= 1: all four set
    bad += [call(K_=0, src=[t if i == j else None for i, t in enumerate(srcs)]) for j in range(4)]        # K = 0: all four null
    bad += [call(K_=K)]
    assert all(rc == E_INVALID for rc in bad), bad
    assert all(bool((b == poison).all()) for b in bufs)
    wsz = ctx.lib.lrbms3_reduced_parabolic_estimate_batch_work_size
    assert wsz(ctx.handle, 33, 3, 2) == -1 and wsz(ctx.handle, 5, 65, 2) == -1 and wsz(ctx.handle, 5, 3, 0) == -1 and wsz(ctx.handle, 0, 3, 2) == -1
    assert 0 < wsz(ctx.handle, N, nmu, nt) <= size
    # the arguments above are otherwise fine (the buffers are larger than this call needs: it addresses them with its own sizes)
    Ud = ctx.from_numpy(ref.panel(S, N, nmu, nt))
    dev[0] = Ud
    assert call() == 0
    assert call(K_=K, src=[ctx.from_numpy(np.ascontiguousarray(phi[:nmu, :nt + 1])), srcs[1], ctx.from_numpy(r_fd_K[:, :, :Q * N].copy()), srcs[3]]) == 0
    want = _host(_call(s, thetas[:nmu], coef[:nmu], Ud, nt))
    assert call() == 0
    assert np.array_equal(bufs[5][:nmu].cpu().numpy(), want['est'])


# ---------------------------------------------------------------------------------------------------------------- Python level
def _pd(p):
    return {'grid': p['grid'], 'lambda': {'functions': p['lambdas'], 'coefficients': p['thetas']}, 'lambda_bar': p['lambda_bar'],
            'lambda_hat': p['lambda_hat'], 'f': p['f'], 'mu_bar': p['mu_bar'], 'mu_hat': p['mu_hat']}


_PY = {}


def _reduced_model(source):
    """d, rd, the bases and the trajectories of three parameters on aniso_2x2x1, T = 0.75, nt = 3 (as
    tests/test_parabolic_batch3d_gpu.py builds them), with or without the PARABOLIC source of tests/affine_source3d_ref.py."""
    if source not in _PY:
        from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D, discretize
        p = c3.make_problem('aniso_2x2x1')
        T, nt = 0.75, 3
        if source:
            from affine_source3d_ref import PARABOLIC, problem_dict
            d, _ = discretize(problem_dict(p, coeffs=PARABOLIC), T, nt)
        else:
            d, _ = discretize(_pd(p), T, nt)
        reductor = ParabolicLRBMSReductor3D(d)
        reductor.extend_basis(d.solve(p['mu'])[:, :, [1, 2, nt]])
        rd = reductor.reduce()
        mus = [0.2, p['mu'], 0.9]
        _PY[source] = dict(p=p, d=d, rd=rd, V=reductor._V.cpu().numpy()[:d.engine.S], mus=mus, U=rd.solve_batch(mus), T=T, nt=nt)
    return _PY[source]


def _parts_err(got, want, dt):
    """(|est - est'| / est', worst squared part relative to its largest entry) of two ``estimate`` tuples."""
    (e0, p0), (e1, p1) = got, want
    sq = lambda p: (p[0], p[1], p[2], np.asarray(p[3]) ** 2 * 3.0 / dt, np.asarray(p[4]) ** 2 * dt)      # noqa: E731
    return abs(e0 - e1) / abs(e1), max(c3.rel(a, b) for a, b in zip(sq(p0), sq(p1)))


@pytest.mark.parametrize('source', (False, True))
def test_estimate_batch_native_against_estimate_and_the_reference(source):
    m_ = _reduced_model(source)
    p, d, rd, mus, U, nt = m_['p'], m_['d'], m_['rd'], m_['mus'], m_['U'], m_['nt']
    assert (rd.rhs_red_K is not None) == source
    S, N = d.engine.S, rd.N
    native = rd.estimate_batch(U, mus, native=True)
    assert len(native) == len(mus)
    if source:
        from affine_source3d_ref import PARABOLIC, AffineSource3D, ParabolicSourceReduced3D
        red = ParabolicSourceReduced3D(AffineSource3D(p, coeffs=PARABOLIC), m_['V'], m_['T'], nt)
    else:
        from parabolic3d_ref import ParabolicReduced3D
        red = ParabolicReduced3D(c3.oracle_of(p), [m_['V'][ii] for ii in range(S)], m_['T'], nt)
    for m, mu in enumerate(mus):
        single = rd.estimate(U[m], mu)
        est, parts = native[m]
        assert isinstance(est, float) and [np.shape(x) for x in parts] == [np.shape(x) for x in single[1]]
        e_est, e_parts = _parts_err(native[m], single, rd.dt)
        o_est, o_parts = _parts_err(native[m], red.estimate(U[m].cpu().numpy().reshape(nt + 1, -1), mu), rd.dt)
        print('PEB3D estimate_batch source={} mu={}: est {:.2e} parts {:.2e} (single), est {:.2e} parts {:.2e} (reference)'.format(
            source, mu, e_est, e_parts, o_est, o_parts))
        assert est > 0.0 and e_est <= 1e-9 and e_parts <= TOL, (mu, e_est, e_parts)
        assert o_est <= 1e-6 and o_parts <= 1e-6, (mu, o_est, o_parts)
    if source:
        with pytest.raises(ValueError):
            rd.estimate_batch(U[:, :nt], mus, native=True)


def test_seventy_parameters_are_two_native_calls_and_the_default_is_the_loop():
    m_ = _reduced_model(False)
    rd, mus, U = m_['rd'], m_['mus'], m_['U']
    ctx = m_['d'].engine.ctx
    many = list(np.linspace(0.2, 0.9, 70))
    U70 = rd.solve_batch(many)
    calls = []
    inner = ctx.reduced_parabolic_estimate_batch
    ctx.reduced_parabolic_estimate_batch = lambda *a, **k: calls.append(a[1].shape[0]) or inner(*a, **k)
    try:
        native = rd.estimate_batch(U70, many, native=True)
        loop = rd.estimate_batch(U, mus)
        assert calls == [64, 6]
    finally:
        del ctx.reduced_parabolic_estimate_batch
    for m in (0, 63, 64, 69):
        e_est, e_parts = _parts_err(native[m], rd.estimate(U70[m], many[m]), rd.dt)
        assert e_est <= 1e-9 and e_parts <= TOL, (m, e_est, e_parts)
    for m, mu in enumerate(mus):                     # native=False: the loop's bits, nothing went to the export
        est, parts = rd.estimate(U[m], mu)
        assert loop[m][0] == est and all(np.array_equal(a, b) for a, b in zip(loop[m][1], parts))


def test_a_model_beyond_the_batch_limits_runs_the_loop_under_native():
    """N > 32: ``estimate_batch(native=True)`` returns the bits of the loop of ``estimate`` (the export is not called)."""
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D, discretize
    p = c3.make_problem('q1_strip')
    d, _ = discretize(_pd(p), 0.2, 2)
    N = 33
    rd = ParabolicLRBMSReductor3D(d, bases=c3.make_bases3d(d.engine.S, d.engine.ctx.n, N, seed=2)).reduce()
    assert rd.N == 33
    ctx = d.engine.ctx
    ctx.reduced_parabolic_estimate_batch = None      # a call would raise
    try:
        mus = [0.4, 1.1]
        U = ctx.from_numpy(ref.panel(d.engine.S, N, 2, 2).transpose(3, 0, 1, 2).copy())
        native = rd.estimate_batch(U, mus, native=True)
    finally:
        del ctx.reduced_parabolic_estimate_batch
    for m, mu in enumerate(mus):
        est, parts = rd.estimate(U[m], mu)
        assert native[m][0] == est and all(np.array_equal(a, b) for a, b in zip(native[m][1], parts))
