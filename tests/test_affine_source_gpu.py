"""Parameter-dependent affine sources on the stationary 2D path, on the GPU: f(mu) = sum_j theta^f_j(mu) f_j on the OS2015
problem with a second, switching component (tests/affine_source_ref.py).  Every layer against the product's existing
single-source path on the frozen f(mu) and against the oracle: discretize, d.solve, reduce() (rhs_red_K, r_fd_K), rd.solve /
rd.solve_batch (lrbms_reduced_solve_batch_src), the estimates, the correctors and AdaptiveEnrichment, storage."""
import numpy as np
import pytest

from affine_source_ref import SMALL, AffineSource, coefficients, frozen_problem, make_problem
from oracle.lrbms import OracleReductor
from parabolic_source_ref import reduced_matrices

pytestmark = pytest.mark.gpu

MUS = ([0.3], [0.8])                       # the second coefficient is 0 at 0.3, 0.6 at 0.8


def _rel(a, b):
    a = a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a, dtype=np.float64)
    b = b.cpu().numpy() if hasattr(b, 'cpu') else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _discretize(p):
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    return discretize(p)


_CACHE = {}


def _setup(config=SMALL):
    """(p, d, reductor, rd) of the two-component problem, the basis from three snapshots; cached per config."""
    key = repr(config)
    if key not in _CACHE:
        from pylrbms_amd.reductor import LRBMSReductor
        p = make_problem(config)
        d, data = _discretize(p)
        reductor = LRBMSReductor(d, products=[d.operators['local_energy_dg_product_{}'.format(ii)]
                                              for ii in range(data['block_space'].num_blocks)])
        for mu in ([0.2], [0.7], [1.0]):
            reductor.extend_basis(d.solve(mu))
        _CACHE[key] = (p, d, data, reductor, reductor.reduce())
    return _CACHE[key]


def _frozen(p, mu, reductor):
    """The product's existing single-source path on f(mu): discretization, reductor on the same bases, reduced model."""
    from pylrbms_amd.reductor import LRBMSReductor
    df, _ = _discretize(frozen_problem(p, mu))
    assert df._affine_f is None
    rf = LRBMSReductor(df, bases={k: v for k, v in reductor.bases.items() if k.startswith('domain_')})
    return df, rf, rf.reduce()


def _bases_host(reductor, S):
    return [reductor.bases['domain_{}'.format(ii)].tensor[0].cpu().numpy() for ii in range(S)]


def test_discretize_accepts_a_parametric_source():
    """On the parent commit this raised NotImplementedError ('one f component with coefficient 1')."""
    p, d, _, _, rd = _setup()
    ref = AffineSource(p)
    src, eng = d._affine_f, d.engine
    assert src['K'] == 2 and tuple(src['F2'].shape) == (eng.S, 2, 2)
    assert _rel(src['b_K'], ref.b_K.reshape(2, eng.S, eng.t.n)) < 1e-12
    assert d.estimator.local_eta_rf_squared is None          # as the reference for K > 1
    assert list(d.f_coefficients([0.3])) == [1.0, 0.0] and list(d.f_coefficients([0.8])) == list(coefficients(p, [0.8]))
    assert tuple(rd.rhs_red_K.shape) == (2, eng.S, rd.N) and tuple(rd.r_fd_K.shape) == (2, eng.S, 5 * eng.Q * rd.N)


def test_plain_source_keeps_the_existing_path():
    p = make_problem()
    f = p['f']['functions'][0]
    for fp in (f, {'functions': [f], 'coefficients': [1]}):
        d, _ = _discretize(dict(p, f=fp))
        assert d._affine_f is None


@pytest.mark.parametrize('mu', MUS)
def test_full_order_solve(mu):
    p, d, _, reductor, _ = _setup()
    df, _, _ = _frozen(p, mu, reductor)
    U, Uf = d.solve(mu), df.solve(mu)
    assert d.last_solve_info['relative_residual'] <= 1e-10
    assert _rel(U.tensor, Uf.tensor) < 1e-9
    ref = AffineSource(p)
    assert _rel(U.tensor[:, :, 0], ref.solve(mu)) < 1e-8
    # lrbms_combine_sources: b(mu) against the frozen discretization's b, and in the fma order spelled out
    eng = d.engine
    th = d.f_coefficients(mu)
    b = eng.ctx.combine_sources(th, d._affine_f['b_K'])
    assert _rel(b, df.engine.b) < 1e-12
    bK = d._affine_f['b_K']
    assert _rel(b, th[0] * bK[0] + th[1] * bK[1]) < 1e-15


def test_combine_sources_shapes_and_order():
    """Odd lengths and misaligned starts take the scalar form; K up to 64; K = 1, phi = 1 copies."""
    import torch
    _, d, _, _, _ = _setup()
    c = d.engine.ctx
    rng = np.random.default_rng(4)
    for K, M in ((1, 7), (2, 1000), (3, 1001), (64, 4096)):
        x = c.from_numpy(rng.standard_normal((K, M)))
        ph = rng.standard_normal(K)
        y = c.combine_sources(ph, x)
        want = ph @ x.cpu().numpy()
        assert _rel(y, want) < 1e-13, (K, M)
        xo = c.zeros(K * M + 1)
        xo[1:] = x.reshape(-1)
        ys = c.combine_sources(ph, xo[1:].view(K, M))               # rows that start off the 16-byte grid: the scalar form
        assert _rel(ys, want) < 1e-13, (K, M)
        if M % 2 == 0:
            assert torch.equal(ys, y)                                # both forms add in the same order
    x = c.from_numpy(rng.standard_normal((1, 513)))
    assert torch.equal(c.combine_sources(np.ones(1), x), x[0])


@pytest.mark.parametrize('mu', MUS)
def test_projected_sources_against_the_frozen_pass_in_both_layouts(mu):
    p, d, _, reductor, rd = _setup()
    df, _, _ = _frozen(p, mu, reductor)
    th = d.f_coefficients(mu)
    rhs = sum(th[j] * rd.rhs_red_K[j] for j in range(2))
    rfd = sum(th[j] * rd.r_fd_K[j] for j in range(2))
    eng = df.engine
    V = reductor._V.contiguous()
    N = V.shape[2]
    for fused in (True, False):
        buf = eng.alloc_reduce_buffers(N, images=not fused, factored=fused)
        buf = eng.project_and_estimate(V, buf, fused=fused)
        assert _rel(rhs, buf['sys'][1]) < 1e-12, fused
        assert _rel(rfd, buf['grams'][1]) < 1e-12, fused


def _mus(n, seed):
    from pylrbms_amd.parameters import parse_parameter
    rng = np.random.default_rng(seed)
    vals = rng.uniform(0.1, 1.0, n)
    vals[::5] = 0.3                                              # the second coefficient is 0 there
    return [parse_parameter([v], {'diffusion': (1,)}) for v in vals]


@pytest.mark.parametrize('nmu', [1, 17, 33, 64, 65])
def test_reduced_solve_batch(nmu):
    p, d, _, _, rd = _setup()
    eng = d.engine
    mus = _mus(nmu, seed=nmu)
    ub = rd.solve_batch(mus).tensor
    assert tuple(ub.shape) == (eng.S, rd.N, nmu)
    rhs_K = rd.rhs_red_K.cpu().numpy().reshape(2, -1)
    for m, mu in enumerate(mus):
        us = rd.solve(mu).tensor[:, :, 0]
        assert _rel(ub[:, :, m], us) < 1e-10, m
        A, _ = reduced_matrices(rd.B_sys.cpu().numpy(), rd.M_red.cpu().numpy(), eng.nbr, d.theta(mu))
        keep = np.abs(np.diag(A)) > 0
        ref = np.linalg.solve(A[np.ix_(keep, keep)], (d.f_coefficients(mu) @ rhs_K)[keep])
        got = ub[:, :, m].cpu().numpy().reshape(-1)
        assert _rel(got[keep], ref) < 1e-10, m
        assert np.abs(got[~keep]).max(initial=0.0) == 0.0


@pytest.mark.parametrize('nmu', [1, 16, 17, 40, 65])
def test_zero_source_columns_come_back_as_zeros(nmu):
    """All theta^f_j(mu) = 0 for some columns of the panel: exact zeros there, the other columns as solved alone."""
    _, d, _, _, rd = _setup()
    c = d.engine.ctx
    rng = np.random.default_rng(nmu)
    thetas = np.array([d.theta([v]) for v in rng.uniform(0.1, 1.0, nmu)])
    phis = rng.uniform(0.5, 1.5, (nmu, 2))
    zero = np.arange(nmu) % 3 == 0
    phis[zero] = 0.0
    u, info = c.reduced_solve_batches_src(thetas, phis, rd.B_sys, rd.rhs_red_K)
    uh = u.cpu().numpy()
    assert np.isfinite(uh).all() and info['relative_residual'] <= 1e-13
    assert np.all(uh[:, :, zero] == 0.0)
    for m in np.where(~zero)[0][:4]:
        rhs = c.combine_sources(phis[m], rd.rhs_red_K)
        us, _ = c.reduced_solve(thetas[m], rd.B_sys, rhs)
        assert _rel(uh[:, :, m], us) < 1e-10
    u0, _ = c.reduced_solve_batch_src(thetas[:1], np.zeros((1, 2)), rd.B_sys, rd.rhs_red_K)   # a call of zeros only
    assert bool((u0 == 0).all())


@pytest.mark.parametrize('prebuilt', [False, True])
@pytest.mark.parametrize('nmu', [5, 17, 40])
def test_one_unit_component_gives_the_bits_of_the_existing_export(nmu, prebuilt):
    import torch
    _, d, _, _, rd = _setup()
    c = d.engine.ctx
    rhs = rd.rhs_red_K[0].contiguous()
    thetas = np.array([d.theta([v]) for v in np.linspace(0.1, 1.0, nmu)])
    pc = c.reduced_precond_build(d.theta([0.55]), rd.B_sys) if prebuilt else None
    c.reduced_precond_use(pc)
    try:
        u_old, i_old = c.reduced_solve_batch(thetas, rd.B_sys, rhs)
        u_new, i_new = c.reduced_solve_batch_src(thetas, np.ones((nmu, 1)), rd.B_sys, rhs[None].contiguous())
    finally:
        c.reduced_precond_use(None)
    assert torch.equal(u_new, u_old) and i_new == i_old


def _parts_rel(a, b):
    return max(_rel(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('mu', MUS)
def test_estimates_against_the_frozen_path_and_the_oracle(mu):
    import torch
    from pylrbms_amd.vectorarrays import ReducedVectorArray
    p, d, _, reductor, rd = _setup()
    df, _, rdf = _frozen(p, mu, reductor)
    ref = AffineSource(p)
    eng = d.engine
    # full order: the solution and two more vectors (one chunk, batched)
    U = d.solve(mu)
    eta, parts, loc = d.estimate(U, mu, decompose=True)
    eta_f, parts_f, loc_f = df.estimate(U, mu, decompose=True)
    assert abs(eta - eta_f) < 1e-10 * eta_f and _parts_rel(parts, parts_f) < 1e-10 and _rel(loc, loc_f) < 1e-10
    eta_o, parts_o, _ = ref.estimate(U.tensor[:, :, 0].cpu().numpy(), mu)
    assert abs(eta - eta_o) < 1e-9 * eta_o
    for a, b in zip(parts, parts_o):
        assert _rel(a[:, 0], b) < 1e-9
    rng = np.random.default_rng(1)
    W = U.tensor + torch.as_tensor(rng.standard_normal((eng.S, eng.t.n, 3)), device=U.tensor.device)
    UW = type(U)(torch.cat([U.tensor, W], dim=2).contiguous(), U.space)
    etas, parts3, _ = d.estimate(UW, mu, decompose=True)
    etas_f, parts3_f, _ = df.estimate(UW, mu, decompose=True)
    assert _rel(etas, etas_f) < 1e-10 and _parts_rel(parts3, parts3_f) < 1e-10
    assert _rel(etas[0], eta) < 1e-12
    # reduced: single and batched
    u = rd.solve(mu)
    uf = rdf.solve(mu)
    assert _rel(u.tensor, uf.tensor) < 1e-10
    eta_r, parts_r, loc_r = rd.estimate(u, mu, decompose=True)
    eta_rf, parts_rf, loc_rf = rdf.estimate(u, mu, decompose=True)
    assert abs(eta_r - eta_rf) < 1e-10 * eta_rf and _parts_rel(parts_r, parts_rf) < 1e-10 and _rel(loc_r, loc_rf) < 1e-10
    ored = OracleReductor(ref.at(mu), _bases_host(reductor, eng.S)).reduce()
    uo = [x for x in u.tensor[:, :, 0].cpu().numpy()]
    eta_ro, parts_ro, _ = ored.estimate([uo[s][:reductor.local_sizes()[s]] for s in range(eng.S)], ref.parse(mu), decompose=True)
    assert abs(eta_r - eta_ro) < 1e-9 * eta_ro
    for a, b in zip(parts_r, parts_ro):
        assert _rel(a[:, 0], b) < 1e-9
    ub = torch.as_tensor(rng.standard_normal((eng.S, rd.N, 20)), device=u.tensor.device)
    ub[:, :, 0] = u.tensor[:, :, 0]
    ub = ReducedVectorArray(ub.contiguous())
    etab, partsb, _ = rd.estimate(ub, mu, decompose=True)
    etab_f, partsb_f, _ = rdf.estimate(ub, mu, decompose=True)
    assert _rel(etab, etab_f) < 1e-10 and _parts_rel(partsb, partsb_f) < 1e-10
    assert abs(etab[0] - eta_r) < 1e-12 * eta_r


def test_correctors_and_adaptive_enrichment():
    """The correctors are those of f frozen at mu; AdaptiveEnrichment over several mu re-projects incrementally, and every
    array of its reduced model, rhs_red_K / r_fd_K included, is the one of a whole reduce() on the same bases, bit for bit."""
    import torch
    from pylrbms_amd.online_enrichment import AdaptiveEnrichment
    from pylrbms_amd.reductor import LRBMSReductor
    config = {'num_subdomains': [4, 4], 'half_num_fine_elements_per_subdomain_and_dim': 4}
    p = make_problem(config)
    d, data = _discretize(p)
    ref = AffineSource(p)
    for mu in MUS:
        df, _ = _discretize(frozen_problem(p, mu))
        marked = [0, 5, 10, 15]
        got = d.solve_for_local_corrections(marked, mu)
        want = df.solve_for_local_corrections(marked, mu)
        for a, b, ii in zip(got, want, marked):
            assert _rel(a.tensor, b.tensor) < 1e-10
            assert _rel(a.tensor[0, :, 0], ref.local_correction(ii, mu)) < 1e-8
    reductor = LRBMSReductor(d, products=[d.operators['local_energy_dg_product_{}'.format(ii)]
                                          for ii in range(data['block_space'].num_blocks)])
    loop = AdaptiveEnrichment(p, d, data['block_space'], reductor, reductor.reduce(), target_error=1e-12,
                              marking_doerfler_theta=0.8, marking_max_age=2)
    incremental = 0
    for k, mu in enumerate([[0.3], [0.8], [0.45], [1.0], [0.6]]):
        width, previous = reductor.basis_size(), loop.rd
        U, rd, _ = loop.solve(mu, enrichment_steps=1)
        assert np.isfinite(U.tensor.cpu().numpy()).all()
        assert rd.rhs_red is None and rd.operators['r_fd'] is None      # the projections of sum_j f_j belong to no parameter
        if reductor.basis_size() == width and reductor.last_reduce_info['incremental']:
            incremental += 1
            # written in place like B_sys and the Grams: the superseded model shares the new arrays and stays consistent
            assert previous.B_sys is rd.B_sys and previous.rhs_red_K is rd.rhs_red_K and previous.r_fd_K is rd.r_fd_K
        whole = LRBMSReductor(d, bases={kk: v for kk, v in reductor.bases.items() if kk.startswith('domain_')})
        whole._V = reductor._V.clone()                                # the same slab width (zero columns of the reserve)
        rw = whole.reduce()
        for a, b in zip((rd.B_sys, rd.E_red, rd.M_red, rd.rhs_red_K, rd.r_fd_K) + tuple(rd.grams),
                        (rw.B_sys, rw.E_red, rw.M_red, rw.rhs_red_K, rw.r_fd_K) + tuple(rw.grams)):
            assert torch.equal(a, b), k
    assert incremental >= 1


def test_storage_round_trip(tmp_path):
    import torch
    from pylrbms_amd.storage import load_reduced, save_reduced
    p, d, _, reductor, rd = _setup()
    path = str(tmp_path / 'rd.safetensors')
    save_reduced(rd, path)
    rd2 = load_reduced(reductor, path)
    assert torch.equal(rd2.rhs_red_K, rd.rhs_red_K) and torch.equal(rd2.r_fd_K, rd.r_fd_K)
    for mu in MUS:
        u, u2 = rd.solve(mu), rd2.solve(mu)
        assert torch.equal(u.tensor, u2.tensor)
        assert rd.estimate(u, mu) == rd2.estimate(u2, mu)
    assert torch.equal(rd.solve_batch(_mus(5, 2)).tensor, rd2.solve_batch(_mus(5, 2)).tensor)
    # a model without the source components does not load into this discretization, and the other way round
    df, rf, rdf = _frozen(p, MUS[0], reductor)
    plain = str(tmp_path / 'plain.safetensors')
    save_reduced(rdf, plain)
    with pytest.raises(ValueError, match='source'):
        load_reduced(reductor, plain)
    with pytest.raises(ValueError, match='source'):
        load_reduced(rf, path)


def test_solve_stationary_of_the_parabolic_path_refuses_a_time_dependent_source():
    from pylrbms_amd import artificial_channels_problem
    from pylrbms_amd.discretize_parabolic_block_swipdg import discretize
    p = artificial_channels_problem.init_grid_and_problem({'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 8})
    d, _ = discretize(p, 1.0, 4)
    with pytest.raises(NotImplementedError, match='depends on time'):
        d.solve_stationary({'switch': [0.5]})
