"""The parabolic 3D / P2 path on the GPU (lrbms3_mass_inverse_norm2, lrbms3_project_mass, lrbms3_fom_implicit_euler,
lrbms3_reduced_implicit_euler, lrbms3_reduced_time_residual and pylrbms_amd.discretize_parabolic_block_swipdg_3d) against the CPU
reference of tests/parabolic3d_ref.py (a restatement of oracle/parabolic.py on the 3D oracle) and dense NumPy."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import common3d as c3
from parabolic3d_ref import Parabolic3D, ParabolicReduced3D

pytestmark = pytest.mark.gpu

PARTS = ('local_eta_nc', 'local_eta_r', 'local_eta_df', 'time_residual', 'time_deriv_nc')


def _pd(p):
    return {'grid': p['grid'], 'lambda': {'functions': p['lambdas'], 'coefficients': p['thetas']}, 'lambda_bar': p['lambda_bar'],
            'lambda_hat': p['lambda_hat'], 'f': p['f'], 'mu_bar': p['mu_bar'], 'mu_hat': p['mu_hat']}


def _setup(name, T=1.0, nt=4):
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import discretize
    p = c3.make_problem(name)
    d, _ = discretize(_pd(p), T, nt)
    return p, c3.oracle_of(p), d


@pytest.mark.parametrize('L', [1, 7])
def test_mass_inverse_norm2_matches_the_oracle_mass(L):
    p, o, d = _setup('aniso_2x2x1')
    Y = np.random.default_rng(L).standard_normal((o.S, o.n, L))
    out = d.engine.ctx.mass_inverse_norm2(d.engine.ctx.from_numpy(Y)).cpu().numpy()
    lu = spla.splu(o.M.tocsc())
    for l in range(L):
        y = Y[:, :, l].reshape(-1)
        ref = (y * lu.solve(y)).reshape(o.S, o.n).sum(axis=1)
        assert c3.rel(out[:, l], ref) < 1e-12


@pytest.mark.parametrize('name', ['aniso_2x2x1', 'kc_3x1x2', 'cfg5_template'])
@pytest.mark.parametrize('N', [1, 4, 30])
def test_project_mass_matches_VtMV(name, N):
    p, o, d = _setup(name)
    V = c3.make_bases3d(o.S, o.n, N, seed=N)
    if N > 1:
        V[0, :, N - 1] = 0.0                     # a zero-padded column of a ragged basis
    M_red = d.engine.ctx.project_mass(d.engine.ctx.from_numpy(V)).cpu().numpy()
    Mt = o.M.tocsr()
    for ii in range(o.S):
        dofs = o.dofs_of(ii)
        ref = V[ii].T @ (Mt[dofs][:, dofs] @ V[ii])
        assert c3.rel(M_red[ii], ref) < 1e-12
    if N > 1:
        assert np.all(M_red[0, N - 1, :] == 0.0) and np.all(M_red[0, :, N - 1] == 0.0)


@pytest.mark.parametrize('name', ['aniso_2x2x1', 'q3_2x1x2', 'kc_3x1x2'])
def test_fom_implicit_euler_matches_sparse_lu_stepping(name):
    p, o, d = _setup(name, T=0.3, nt=5)
    mu = p['mu']
    U = d.solve(mu)
    assert tuple(U.shape) == (o.S, o.n, 6)
    it, res = d.last_solve_info
    assert it > 0 and res <= 1e-10
    ref = Parabolic3D(o, 0.3, 5).solve(mu)
    Uh = U.permute(2, 0, 1).cpu().numpy()
    assert np.abs(Uh[0]).max() == 0.0
    assert c3.rel(Uh, ref) < 1e-8
    # a non-zero initial value is honoured
    eng = d.engine
    U0 = np.random.default_rng(3).standard_normal((o.S, o.n))
    U2, _ = eng.ctx.fom_implicit_euler(d.Q, d.theta(mu), d.dt, 5, eng.ops['A_diag'], eng.ops['A_cpl'], eng.ops['b'],
                                       U0=eng.ctx.from_numpy(U0))
    assert c3.rel(U2.cpu().numpy(), Parabolic3D(o, 0.3, 5).solve(mu, U0=U0)) < 1e-8


def test_fom_implicit_euler_long_horizon_errors_and_the_kept_preconditioner():
    from pylrbms_amd._native import NativeError
    p, o, d = _setup('aniso_2x2x1', T=400.0, nt=16)
    mu = p['mu']
    Us = d.solve_stationary(mu)                  # keeps the elliptic coarse inverse (fom_precond_keep) in the context
    before = Us.clone()
    U = d.solve(mu)
    assert c3.rel(U[:, :, -1].cpu().numpy(), Us.cpu().numpy()) < 1e-7
    after = d.solve_stationary(mu)
    assert bool((after == before).all())         # the implicit-Euler call neither used nor replaced it
    eng = d.engine
    args = (eng.ops['A_diag'], eng.ops['A_cpl'], eng.ops['b'])
    th = d.theta(mu)
    with pytest.raises(NativeError):
        eng.ctx.fom_implicit_euler(d.Q, th, 0.0, 4, *args)
    with pytest.raises(NativeError):
        eng.ctx.fom_implicit_euler(d.Q, th, -1.0, 4, *args)
    with pytest.raises(NativeError):
        eng.ctx.fom_implicit_euler(d.Q, th, 0.1, 0, *args)
    with pytest.raises(NativeError):
        eng.ctx.fom_implicit_euler(d.Q, th, 0.1, 4, *args, rtol=1e-30, max_iter=3)


def _dense_reduced(S, N, nbr, B, th):
    A = np.zeros((S * N, S * N))
    for s in range(S):
        for slot in range(7):
            t = nbr[s, slot]
            if t >= 0:
                A[s * N:(s + 1) * N, t * N:(t + 1) * N] = np.einsum('q,qij->ij', th, B[:, s, slot])
    return A


@pytest.mark.parametrize('name,ragged', [('aniso_2x2x1', False), ('aniso_2x2x1', True), ('q3_2x1x2', True)])
def test_reduced_implicit_euler_and_time_residual_match_dense_numpy(name, ragged):
    p, o, d = _setup(name, T=0.2, nt=4)
    eng, mu = d.engine, p['mu']
    N = p['N']
    V = c3.make_bases3d(o.S, o.n, N, seed=5)
    if ragged:
        V[1, :, N - 2:] = 0.0                    # subdomain 1 has N - 2 vectors, zero-padded
    Vt = eng.ctx.from_numpy(V)
    out = eng.project_and_estimate(Vt)
    M_red = eng.ctx.project_mass(Vt)
    th = d.theta(mu)
    u, (it, res) = eng.ctx.reduced_implicit_euler(d.Q, th, 0.05, 4, out['B_sys'], M_red, out['rhs_red'])
    assert res <= 1e-12
    u = u.cpu().numpy()
    nbr = np.asarray(p['grid'].neighbor_slots).reshape(o.S, 7)
    B, Mr, rhs = out['B_sys'].cpu().numpy(), M_red.cpu().numpy(), out['rhs_red'].cpu().numpy().reshape(-1)
    A = _dense_reduced(o.S, N, nbr, B, th)
    M = np.zeros_like(A)
    for s in range(o.S):
        M[s * N:(s + 1) * N, s * N:(s + 1) * N] = Mr[s]
    keep = np.ones(o.S * N, dtype=bool)
    if ragged:
        keep[N + N - 2:2 * N] = False
        assert np.all(u[:, 1, N - 2:] == 0.0)    # padded unknowns stay exactly 0
    Ak, Mk = A[np.ix_(keep, keep)], M[np.ix_(keep, keep)]
    ref = np.zeros((5, int(keep.sum())))
    for k in range(4):
        ref[k + 1] = np.linalg.solve(Mk + 0.05 * Ak, Mk @ ref[k] + 0.05 * rhs[keep])
    assert c3.rel(u.reshape(5, -1)[:, keep], ref) < 1e-9
    # time residual on random differences (padded entries zero)
    dU = np.random.default_rng(1).standard_normal((3, o.S, N))
    if ragged:
        dU[:, 1, N - 2:] = 0.0
    tr = eng.ctx.reduced_time_residual(d.Q, th, out['B_sys'], M_red, eng.ctx.from_numpy(dU)).cpu().numpy()
    for l in range(3):
        y = (A @ dU[l].reshape(-1))
        for s in range(o.S):
            ks = keep[s * N:(s + 1) * N]
            ys = y[s * N:(s + 1) * N][ks]
            assert abs(tr[l, s] - ys @ np.linalg.solve(Mr[s][np.ix_(ks, ks)], ys)) < 1e-10 * abs(tr[l, s])


@pytest.mark.parametrize('name,T,nt', [('aniso_2x2x1', 0.5, 6), ('q3_2x1x2', 0.2, 5), ('cfg5_template', 0.5, 4)])
def test_parabolic3d_driver_sequence(name, T, nt):
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D
    p, o, d = _setup(name, T=T, nt=nt)
    mu = p['mu']
    ref = Parabolic3D(o, T, nt)

    U = d.solve(mu)
    Uh = U.permute(2, 0, 1).cpu().numpy()
    assert c3.rel(Uh, ref.solve(mu)) < 1e-8

    est, parts = d.estimate(U, mu)
    est_o, parts_o = ref.estimate(Uh, mu)
    for nm, a, b in zip(PARTS, parts, parts_o):
        assert a.shape == np.shape(b) and c3.rel(a, b) < 1e-7, nm
    assert abs(est - est_o) < 1e-7 * est_o

    reductor = ParabolicLRBMSReductor3D(d)
    snap_idx = [1, nt // 2, nt]
    reductor.extend_basis(U[:, :, snap_idx])
    N = reductor.basis_size()
    assert N == 1 + len(snap_idx) and reductor.local_sizes() == [N] * o.S
    rd = reductor.reduce()
    u = rd.solve(mu)
    assert tuple(u.shape) == (nt + 1, o.S, N)
    UU = reductor.reconstruct(u)
    assert tuple(UU.shape) == (o.S, o.n, nt + 1)

    V = reductor.bases.cpu().numpy()
    red = ParabolicReduced3D(o, [V[ii] for ii in range(o.S)], T, nt)
    u_o = red.solve(mu)
    assert c3.rel(u.cpu().numpy().reshape(nt + 1, -1), u_o) < 1e-8
    est_r, parts_r = rd.estimate(u, mu)
    est_ro, parts_ro = red.estimate(u_o, mu)
    for nm, a, b in zip(PARTS, parts_r, parts_ro):
        assert c3.rel(a, b) < 1e-6, nm
    assert abs(est_r - est_ro) < 1e-6 * est_ro
    est_f, parts_f = d.estimate(UU, mu)
    for i in (0, 1, 2, 4):
        assert c3.rel(parts_r[i], parts_f[i]) < 1e-6, PARTS[i]


def test_extend_basis_skips_vectors_in_the_span():
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import ExtensionError3D
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D
    p, o, d = _setup('aniso_2x2x1', T=0.5, nt=3)
    U = d.solve(p['mu'])
    red = ParabolicLRBMSReductor3D(d)
    red.extend_basis(U[:, :, [0, 1, 1]])      # the zero initial value and the repeated vector are skipped
    assert red.basis_size() == 2
    with pytest.raises(ExtensionError3D):
        red.extend_basis(U[:, :, [0, 1]])
    red.extend_basis(U[:, :, 2:], max_vectors=3)
    assert red.basis_size() == 3


def test_out_of_scope_cases_raise_not_implemented():
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D, discretize
    from pylrbms_amd.grid3d import make_grid3d
    p = c3.make_problem('aniso_2x2x1')
    with pytest.raises(NotImplementedError):
        discretize(_pd(p), 1.0, 2, elliptic_reconstruction=True)
    sharded = dict(_pd(p), grid=make_grid3d(num_subdomains=p['P'], cubes_per_subdomain_and_dim=p['kc'], kappa=p['kappa'], rank=0,
                                            world_size=2))
    with pytest.raises(NotImplementedError):
        discretize(sharded, 1.0, 2)
    d, _ = discretize(_pd(p), 1.0, 2)
    red = ParabolicLRBMSReductor3D(d)
    with pytest.raises(NotImplementedError):
        red.enrich_local(0, None)
