"""Parameter-dependent affine sources f(mu) = sum_j c_j(mu) f_j on the stationary 3D / P2 path, on the GPU, against the oracle
restatement of tests/affine_source3d_ref.py (every quantity at mu is that of the oracle discretization with f frozen at f(mu)).

Tolerances are those the existing 3D tests assert for the same single-source quantities: full-order solve 1e-9 and eta 1e-8
(tests/test_api3d_gpu.py), reduced solve against the oracle reduced model 1e-8, batched against single 1e-10, projected arrays
1e-12 (tests/test_parabolic3d_gpu.py)."""
import copy

import numpy as np
import pytest

import common3d as c3
from affine_source3d_ref import AffineSource3D, problem_dict, projected_self_blocks

pytestmark = pytest.mark.gpu

_CACHE = {}


def _setup(name):
    """(p, oracle restatement, d) of the two-component problem on the common3d grid ``name``."""
    if name not in _CACHE:
        from pylrbms_amd.discretize_elliptic_block_swipdg_3d import discretize
        p = c3.make_problem(name)
        d, _ = discretize(problem_dict(p))
        _CACHE[name] = (p, AffineSource3D(p), d)
    return _CACHE[name]


def _plain(name):
    """(p, oracle, d) of the plain single-source problem."""
    key = ('plain', name)
    if key not in _CACHE:
        from pylrbms_amd.discretize_elliptic_block_swipdg_3d import discretize
        p = c3.make_problem(name)
        d, _ = discretize(dict(problem_dict(p), f=p['f']))
        _CACHE[key] = (p, c3.oracle_of(p), d)
    return _CACHE[key]


def _pass(d, V):
    """(Vt, work, out) of one pass on the bases V (host)."""
    eng = d.engine
    Vt = eng.ctx.from_numpy(V)
    work = eng.alloc_work(V.shape[2])
    return Vt, work, eng.project_and_estimate(Vt, work=work)


@pytest.mark.parametrize('name', ['aniso_2x2x1', 'q3_2x1x2', 'cfg5_template'])
def test_source_setup_and_projections_match_the_oracle(name):
    p, src, d = _setup(name)
    o, eng, s = src.d, d.engine, d._src
    assert s['K'] == 2 and tuple(s['F2'].shape) == (o.S, 2, 2)
    print('F2', c3.rel(s['F2'].cpu().numpy(), src.gram()))
    assert c3.rel(s['F2'].cpu().numpy(), src.gram()) < 1e-12
    comps = [src.component(j) for j in range(2)]
    for j in range(2):
        assert c3.rel(s['b_K'][j].cpu().numpy().ravel(), comps[j].b) < 1e-12
        assert c3.rel(s['bdiv_K'][j].cpu().numpy().ravel(), comps[j].bdiv) < 1e-12
    V = c3.make_bases3d(o.S, o.n, p['N'], seed=3)
    Vt, work, out = _pass(d, V)
    rhs_K, rfd_K = eng.ctx.project_sources(d.Q, s['b_K'], s['bdiv_K'], Vt, work)
    QN = d.Q * p['N']
    assert tuple(rhs_K.shape) == (2, o.S, p['N']) and tuple(rfd_K.shape) == (2, o.S, QN)
    for j in range(2):
        rhs_o, rfd_o = projected_self_blocks(comps[j], V)
        err = c3.rel(rhs_K[j].cpu().numpy(), rhs_o), c3.rel(rfd_K[j].cpu().numpy(), rfd_o)
        print(name, 'component', j, 'rhs_red_K', err[0], 'r_fd_K', err[1])
        assert err[0] < 1e-12 and err[1] < 1e-12
    if name == 'aniso_2x2x1':      # the same blocks out of the oracle's reductor: its r_fd on the neighbourhood, slot 3 = [self]
        rd = c3.reduce_with_oracle(p, comps[1], V)
        assert c3.rel(rhs_K[1].cpu().numpy(), np.stack(rd.rhs)) < 1e-12
        want = np.stack([c3.oracle_dense_blocks(p, comps[1], rd, ii)['r_fd'][3 * QN:4 * QN] for ii in range(o.S)])
        assert c3.rel(rfd_K[1].cpu().numpy(), want) < 1e-12


@pytest.mark.parametrize('name', ['aniso_2x2x1', 'cfg5_template'])
def test_one_component_reproduces_the_pass_and_f2(name):
    """K = 1 with the discretization's own samples / b / bdiv: F2 is f2 bit for bit, the projections are the pass's rhs_red and
    r_fd (another summation order: 1e-12)."""
    import torch
    p, o, d = _plain(name)
    eng = d.engine
    F2 = eng.ctx.assemble_source_gram(eng.f_smp[None].contiguous())
    assert torch.equal(F2.reshape(-1), eng.ops['f2'])
    Vt, work, out = _pass(d, c3.make_bases3d(o.S, o.n, p['N'], seed=8))
    rhs_K, rfd_K = eng.ctx.project_sources(d.Q, eng.ops['b'][None].contiguous(), eng.ops['bdiv'][None].contiguous(), Vt, work)
    print('rhs_red', c3.rel(rhs_K[0].cpu().numpy(), out['rhs_red'].cpu().numpy()), 'r_fd',
          c3.rel(rfd_K[0].cpu().numpy(), out['r_fd'].cpu().numpy()))
    assert c3.rel(rhs_K[0].cpu().numpy(), out['rhs_red'].cpu().numpy()) < 1e-12
    assert c3.rel(rfd_K[0].cpu().numpy(), out['r_fd'].cpu().numpy()) < 1e-12


@pytest.mark.parametrize('K', [3, 17, 64])
def test_project_sources_and_gram_for_many_components(K):
    """More components than one 16-row tile of the matrix-core kernel: against float64 einsum of the same arrays."""
    import torch
    p, o, d = _plain('aniso_2x2x1')
    eng, t = d.engine, d.engine.t
    rng = np.random.default_rng(K)
    b_K = eng.ctx.from_numpy(rng.standard_normal((K, o.S, o.n)))
    bdiv_K = eng.ctx.from_numpy(rng.standard_normal((K, o.S, t.n_T)))
    Vt, work, out = _pass(d, c3.make_bases3d(o.S, o.n, 5, seed=K))
    rhs_K, rfd_K = eng.ctx.project_sources(d.Q, b_K, bdiv_K, Vt, work)
    assert c3.rel(rhs_K.cpu().numpy(), torch.einsum('ksn,snj->ksj', b_K, Vt).cpu().numpy()) < 1e-12
    # r_fd_K is linear in bdiv_K: the map is pinned by the K = 1 case against the pass (above); here every component against it
    one = torch.stack([eng.ctx.project_sources(d.Q, b_K[j:j + 1].contiguous(), bdiv_K[j:j + 1].contiguous(), Vt, work)[1][0]
                       for j in range(K)])
    assert c3.rel(rfd_K.cpu().numpy(), one.cpu().numpy()) < 1e-12
    f_smp_K = eng.ctx.from_numpy(rng.standard_normal((K, o.S, t.n_T, eng.spec.f_stride)))
    F2 = eng.ctx.assemble_source_gram(f_smp_K).cpu().numpy()
    WB = np.asarray(t.tables(eng.spec)['WB'])
    smp = f_smp_K.cpu().numpy()[..., :eng.spec.nB]
    assert c3.rel(F2, np.einsum('k,jsek,lsek->sjl', WB, smp, smp)) < 1e-12
    assert np.array_equal(F2, F2.transpose(0, 2, 1))


@pytest.mark.parametrize('name', ['aniso_2x2x1', 'q3_2x1x2'])
def test_full_order_solve_and_estimate_on_both_sides_of_the_switch(name):
    p, src, d = _setup(name)
    o = src.d
    for mu in (0.3, 0.9):                              # the second component is off / on
        assert np.array_equal(d.source_coefficients(mu), src.coefficients(mu))
        U = d.solve(mu, rtol=1e-12)
        ref = src.solve(mu)
        assert c3.rel(U.cpu().numpy(), ref) < 1e-9
        eta, (nc, r, df), _ = d.estimate(U, mu, decompose=True)
        eta_o, (nco, ro, dfo), _ = src.estimate(ref, mu)
        print(name, mu, 'eta', abs(eta - eta_o) / eta_o)
        assert abs(eta - eta_o) < 1e-8 * eta_o
        for a, b in ((nc, nco), (r, ro), (df, dfo)):
            assert c3.rel(a, b) < 1e-8
        W = np.random.default_rng(5).standard_normal((o.S, o.n))
        assert abs(d.estimate(W, mu) - src.estimate(W, mu)[0]) < 1e-8 * src.estimate(W, mu)[0]
    # mu <= 0.5: the solution of the plain problem with f_0 alone
    _, o_plain, _ = _plain(name)
    assert c3.rel(d.solve(0.3, rtol=1e-12).cpu().numpy().ravel(), o_plain.solve(0.3)) < 1e-9


@pytest.mark.parametrize('name', ['aniso_2x2x1', 'q3_2x1x2', 'cfg5_template'])
def test_reduced_model_matches_the_oracle_reduced_model_with_frozen_f(name):
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    p, src, d = _setup(name)
    o = src.d
    V = c3.make_bases3d(o.S, o.n, p['N'], seed=11)
    red = LRBMSReductor3D(d, V)
    rd = red.reduce()
    assert rd.N == p['N'] and rd.out['rhs_red'] is None and rd.out['r_fd'] is None
    assert tuple(rd.rhs_red_K.shape) == (2, o.S, p['N'])
    for mu in ((0.9,) if name == 'cfg5_template' else (0.3, 0.9)):      # (the oracle's reduction of config 5's template is slow)
        ord_ = src.reduced(V, mu)
        uo = ord_.solve(mu)
        u = rd.solve(mu, rtol=1e-13)
        assert c3.rel(u.cpu().numpy(), np.stack(uo)) < 1e-8
        eta, (nc, r, df), _ = rd.estimate(u, mu, decompose=True)
        eta_o, (nco, ro, dfo), _ = ord_.estimate(uo, mu, decompose=True)
        print(name, mu, 'reduced eta', abs(eta - eta_o) / eta_o, [c3.rel(a, b) for a, b in ((nc, nco), (r, ro), (df, dfo))])
        assert abs(eta - eta_o) < 1e-8 * eta_o
        for a, b in ((nc, nco), (r, ro), (df, dfo)):
            assert c3.rel(a, b) < 1e-8
        # the reduced estimate is the full-order estimate of the reconstruction
        assert abs(d.estimate(red.reconstruct(u), mu) - eta) < 1e-8 * eta


@pytest.mark.parametrize('nmu', [1, 17, 33, 64, 65])
def test_batched_solve_and_estimate_against_the_oracle_and_the_single_calls(nmu):
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    p, src, d = _setup('aniso_2x2x1')
    o = src.d
    key = ('rd', 'aniso_2x2x1')
    if key not in _CACHE:
        V = c3.make_bases3d(o.S, o.n, p['N'], seed=11)
        _CACHE[key] = (V, LRBMSReductor3D(d, V).reduce(), c3.reduce_with_oracle(p, o, V))
    V, rd, rd0 = _CACHE[key]
    mus = [0.1 + 0.9 * k / max(nmu - 1, 1) for k in range(nmu)]          # both sides of 0.5
    U = rd.solve_batch(mus, rtol=1e-13)
    assert tuple(U.shape) == (nmu, o.S, p['N'])
    for k in sorted({0, nmu // 2, nmu - 1}):
        uo = src.reduced_rhs_only(rd0, V, mus[k]).solve(mus[k])
        assert c3.rel(U[k].cpu().numpy(), np.stack(uo)) < 1e-8
        u = rd.solve(mus[k], rtol=1e-13)
        assert c3.rel(U[k].cpu().numpy(), u.cpu().numpy()) < 1e-10
    etas = rd.estimate_batch(U, mus)
    full = rd.estimate_batch(U, mus, decompose=True)
    for k in sorted({0, nmu // 2, nmu - 1}):
        single = rd.estimate(U[k], mus[k])
        assert abs(etas[k] - single) < 1e-10 * single and full[k][0] == etas[k]
    for k in sorted({0, nmu - 1}):                       # all three indicators of the BATCHED estimate against the oracle with frozen f
        ord_ = src.reduced(V, mus[k])
        eta_o, parts_o, _ = ord_.estimate(ord_.solve(mus[k]), mus[k], decompose=True)
        assert abs(etas[k] - eta_o) < 1e-8 * eta_o
        for a, b in zip(full[k][1], parts_o):
            assert c3.rel(a, b) < 1e-8


def test_a_column_with_a_zero_right_hand_side_comes_back_as_zeros():
    """Coefficients [mu > 0.5, 0]-style: column 1 of the batch has phi = 0 exactly and comes back as zeros beside the others."""
    import torch
    p, src, d = _setup('aniso_2x2x1')
    o, eng = src.d, d.engine
    V = c3.make_bases3d(o.S, o.n, p['N'], seed=11)
    Vt, work, out = _pass(d, V)
    rhs_K, _ = eng.ctx.project_sources(d.Q, d._src['b_K'], d._src['bdiv_K'], Vt, work)
    mus = [0.3, 0.6, 0.9]
    th = np.stack([d.theta(mu) for mu in mus])
    phi = np.array([[1.0, 0.2], [0.0, 0.0], [0.5, -1.0]])
    rd0 = c3.reduce_with_oracle(p, o, V)
    for pc in (False, True):
        if pc:
            eng.ctx.reduced_precond_use(eng.ctx.reduced_precond_build(d.Q, d.theta(0.5), out['B_sys']))
        try:
            u, (it, res) = eng.ctx.reduced_solve_batch_src(d.Q, th, phi, out['B_sys'], rhs_K)
        finally:
            eng.ctx.reduced_precond_use(None)
        assert res <= 1e-13 and not bool(torch.isnan(u).any())
        assert float(u[:, :, 1].abs().max()) == 0.0
        for m in (0, 2):
            rhs = eng.ctx.combine_sources(phi[m], rhs_K)
            ref, _ = eng.ctx.reduced_solve(d.Q, th[m], out['B_sys'], rhs)
            assert c3.rel(u[:, :, m].cpu().numpy(), ref.cpu().numpy()) < 1e-10
        for m in range(3):                               # the oracle reduced model with f frozen at sum_j phi[m][j] f_j
            om = src.frozen(phi[m])
            rdm = copy.copy(rd0)
            rdm.d, rdm.rhs = om, [V[ii].T @ om.b[om.dofs_of(ii)] for ii in range(o.S)]
            uo = np.stack(rdm.solve(mus[m]))
            if m == 1:
                assert np.abs(uo).max() == 0.0
            else:
                assert c3.rel(u[:, :, m].cpu().numpy(), uo) < 1e-8


@pytest.mark.parametrize('name,nmu', [('aniso_2x2x1', 5), ('aniso_2x2x1', 64), ('cfg5_template', 20)])
def test_one_component_batch_solve_is_bit_identical_to_the_existing_export(name, nmu):
    import torch
    p, o, d = _plain(name)
    eng = d.engine
    Vt, work, out = _pass(d, c3.make_bases3d(o.S, o.n, p['N'], seed=2))
    th = np.stack([d.theta(0.1 + 0.9 * k / nmu) for k in range(nmu)])
    rhs_K = out['rhs_red'][None].contiguous()
    for pc in (False, True):
        if pc:
            eng.ctx.reduced_precond_use(eng.ctx.reduced_precond_build(d.Q, d.theta(0.5), out['B_sys']))
        try:
            a, ia = eng.ctx.reduced_solve_batch(d.Q, th, out['B_sys'], out['rhs_red'])
            b, ib = eng.ctx.reduced_solve_batch_src(d.Q, th, np.ones((nmu, 1)), out['B_sys'], rhs_K)
        finally:
            eng.ctx.reduced_precond_use(None)
        assert torch.equal(a, b) and ia == ib, 'prebuilt preconditioner: {}'.format(pc)


def test_source_terms_reduce_to_the_existing_estimate_on_a_grid_with_interior_subdomains():
    """K = 1, phi = 1: the estimate with zero f2 / r_fd / bdiv plus lrbms3_reduced_source_terms is lrbms3_reduced_estimate_batch on
    the real f2 / r_fd / bdiv (1e-12); on 3 x 3 x 3 subdomains the bdiv term through the neighbours' flux images is not zero."""
    from pylrbms_amd import sources3d
    p, o, d = _plain('interior_3x3x3')
    eng = d.engine
    N, L = p['N'], 11
    Vt, work, out = _pass(d, c3.make_bases3d(o.S, o.n, N, seed=4))
    rng = np.random.default_rng(9)
    u = eng.ctx.from_numpy(rng.standard_normal((o.S, N, L)))
    th = np.stack([d.theta(0.2 + 0.07 * l) for l in range(L)])
    full = eng.ctx.reduced_estimate_batch(d.Q, th, u, out, eng.ops, eng.hdiam)
    out0, ops0 = sources3d.zeroed(eng, out)
    zero = eng.ctx.reduced_estimate_batch(d.Q, th, u, out0, ops0, eng.hdiam)
    f_smp_K, b_K, bdiv_K = eng.f_smp[None].contiguous(), eng.ops['b'][None].contiguous(), eng.ops['bdiv'][None].contiguous()
    F2 = eng.ctx.assemble_source_gram(f_smp_K)
    _, rfd_K = eng.ctx.project_sources(d.Q, b_K, bdiv_K, Vt, work)
    args = (F2, rfd_K, bdiv_K, out['Rb'], u, eng.ops['ceps'], eng.hdiam)
    terms = eng.ctx.reduced_source_terms(d.Q, th, np.ones((L, 1)), *args)
    assert c3.rel((zero[1] + terms).cpu().numpy(), full[1].cpu().numpy()) < 1e-12
    assert bool((zero[0] == full[0]).all()) and bool((zero[2] == full[2]).all())
    # the neighbour term: without bdiv the result changes
    no_bdiv = eng.ctx.reduced_source_terms(d.Q, th, np.ones((L, 1)), F2, rfd_K, 0.0 * bdiv_K, out['Rb'], u, eng.ops['ceps'], eng.hdiam)
    nb = (terms - no_bdiv).abs().max()
    assert float(nb) > 1e-6 * float(terms.abs().max())
    # per-column phi: the terms are (phi^2 F2 - 2 phi fd) scale, so phi = 2 against phi = 1 pins both parts
    two = eng.ctx.reduced_source_terms(d.Q, th, 2.0 * np.ones((L, 1)), *args)
    scale = (1.0 / np.pi ** 2) / eng.ops['ceps'] * eng.hdiam ** 2
    ff = (F2.reshape(-1) * scale)[:, None]
    assert c3.rel((two - 2.0 * terms).cpu().numpy(), (2.0 * ff).expand(-1, L).cpu().numpy()) < 1e-10


def test_large_basis_goes_through_combine_sources_and_the_single_solve():
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    p = c3.make_problem('q1_strip')                    # Q = 1: N = 34 > 32 fits the pass (Q N <= 64)
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import discretize
    d, _ = discretize(problem_dict(p))
    src = AffineSource3D(p)
    o = src.d
    V = c3.make_bases3d(o.S, o.n, 34, seed=6)
    rd = LRBMSReductor3D(d, V).reduce()
    rd0 = c3.reduce_with_oracle(p, o, V)
    mus = [0.7, 1.4]
    U = rd.solve_batch(mus, rtol=1e-13)
    for k, mu in enumerate(mus):
        uo = src.reduced_rhs_only(rd0, V, mu).solve(mu)
        assert c3.rel(U[k].cpu().numpy(), np.stack(uo)) < 1e-8


def test_refusals():
    from pylrbms_amd import storage
    from pylrbms_amd._native import NativeError
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D, discretize
    from pylrbms_amd.grid3d import make_grid3d
    from pylrbms_amd.parameters import ExpressionParameterFunctional
    p, src, d = _setup('aniso_2x2x1')
    switch = ExpressionParameterFunctional('(diffusion > 0.5) * (2 * diffusion - 1)', {'diffusion': (1,)})
    with pytest.raises(NotImplementedError, match='2D path only'):
        discretize(problem_dict(p, coeffs=[1, switch]))
    grid = make_grid3d(num_subdomains=p['P'], cubes_per_subdomain_and_dim=p['kc'], kappa=p['kappa'], rank=0, world_size=2)
    with pytest.raises(NotImplementedError, match='2D path only'):
        discretize(dict(problem_dict(p), grid=grid))
    rd = LRBMSReductor3D(d, c3.make_bases3d(src.d.S, src.d.n, 3, seed=1)).reduce()
    with pytest.raises(NotImplementedError, match='3D reduced model with an affine source'):
        storage.save_reduced(rd, '/dev/null')
    with pytest.raises(NotImplementedError, match='affine source'):
        rd.operators
    eng = d.engine
    with pytest.raises(NativeError):                   # K outside [1, 64]
        eng.ctx.assemble_source_gram(eng.ctx.zeros(65, eng.S, eng.t.n_T, eng.spec.f_stride))
    with pytest.raises(NativeError):
        eng.ctx.combine_sources(np.ones(65), eng.ctx.zeros(65, 8))
