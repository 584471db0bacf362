"""Online enrichment (SURVEY.md section 8f "next" #1) on the GPU against the oracle:
``DuneDiscretization.solve_for_local_correction`` (reference discretize_elliptic_block_swipdg.py:227-316),
``LRBMSReductor.enrich_local`` (reductor.py:75-78) and the ``AdaptiveEnrichment`` loop (online_enrichment.py:25-93).

The corrector problems are solved iteratively on the GPU (block-Jacobi PCG, rtol 1e-12) and directly by the oracle
(SuperLU): the stated tolerance for the correction vectors is 1e-8 relative to the largest entry.  Reduced quantities
on the ragged bases the enrichment produces are compared at 1e-7."""
import numpy as np
import pytest

from common import energy_orthonormalize, make_bases, oracle_from_problem
from oracle.lrbms import OracleReductor

pytestmark = pytest.mark.gpu

CORR_TOL = 1e-8


def _problem(name, config):
    import importlib
    return importlib.import_module('pylrbms_amd.' + name).init_grid_and_problem(config)


@pytest.mark.parametrize('name,config,mu', [
    ('multiscale_problem', {'num_subdomains': [3, 4], 'coarse_per_subdomain': 2}, 0.37),          # n = 96, all hood shapes
    ('OS2015_academic_problem', {'num_subdomains': [4, 4], 'half_num_fine_elements_per_subdomain_and_dim': 16}, 0.1),  # n = 384
    ('thermalblock_problem', {'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 8},
     (0.4, 0.9, 0.2, 0.6)),                                                                       # Q = 4, every hood has 3 members
    ('multiscale_problem', {'num_subdomains': [3, 3], 'coarse_per_subdomain': 6}, 1.0),           # n_T = 288: 2 elements / thread
    ('multiscale_problem', {'num_subdomains': [2, 2], 'coarse_per_subdomain': 3}, 0.6),           # odd k, corner hoods only
    ('OS2015_academic_problem', {'num_subdomains': [1, 3], 'half_num_fine_elements_per_subdomain_and_dim': 6}, 0.5),  # kx != ky, strip
    # the launch forms of k_hood_pcg the grids above do not reach (n_T = 8 k^2 on k x k squares per subdomain; the dispatch mirror is
    # tests/test_corrector_iterates_host.py): <1,1024> at k = 5, <4,1024> at k = 8, <8,1024> at k = 11 (104 KB of dynamic LDS)
    ('OS2015_academic_problem', {'num_subdomains': [3, 3], 'half_num_fine_elements_per_subdomain_and_dim': 15}, 0.1),
    ('OS2015_academic_problem', {'num_subdomains': [3, 3], 'half_num_fine_elements_per_subdomain_and_dim': 24}, 0.1),
    ('OS2015_academic_problem', {'num_subdomains': [3, 3], 'half_num_fine_elements_per_subdomain_and_dim': 33}, 0.1),
])
def test_local_corrections_match_the_oracle(name, config, mu):
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    p = _problem(name, config)
    d, _ = discretize(p)
    o = oracle_from_problem(p)
    subdomains = list(range(o.S))
    got = d.solve_for_local_corrections(subdomains, mu)
    info = d.last_local_correction_info
    assert info.shape == (o.S, 2) and (info[:, 1] <= 1e-10).all() and (info[:, 0] >= 1).all()
    for ii in subdomains:
        ref = o.solve_for_local_correction(ii, mu)
        x = got[ii].data.reshape(-1)
        assert got[ii].space.subspaces[0].id == 'domain_{}'.format(ii)
        assert np.abs(x - ref).max() < CORR_TOL * np.abs(ref).max(), (ii, np.abs(x - ref).max() / np.abs(ref).max())
    # the single-subdomain entry point of the reference API gives the same vector (bit-identical: same kernel, same order)
    one = d.solve_for_local_correction(subdomains[-1], None, mu)
    assert np.array_equal(one.data, got[-1].data)


def test_whole_domain_neighbourhood_reproduces_the_global_solution():
    """3 x 1 subdomains: N(1) is the whole domain and its Dirichlet boundary is the physical one, so the corrector of
    the middle subdomain IS the full-order solution there (size-independent consistency property)."""
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    p = _problem('OS2015_academic_problem', {'num_subdomains': [3, 1], 'half_num_fine_elements_per_subdomain_and_dim': 12})
    d, _ = discretize(p)
    U = d.solve(0.3).data.reshape(3, -1)
    c = d.solve_for_local_correction(1, None, 0.3).data.reshape(-1)
    assert np.abs(c - U[1]).max() < 1e-8 * np.abs(U[1]).max()


def test_indefinite_neighbourhood_operator_is_reported():
    """1 x 3 subdomains of 3 x 3 coarse squares on the unit square have elements of aspect ratio 3, for which the SWIPDG
    penalties (8 / 14) do not make the form coercive: the oracle's neighbourhood matrix has a negative eigenvalue.  The
    PCG must say so (p.Ap <= 0 -> LRBMS_E_NOT_CONVERGED), never return numbers."""
    from pylrbms_amd._native import NativeError
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    p = _problem('multiscale_problem', {'num_subdomains': [1, 3], 'coarse_per_subdomain': 3})
    o = oracle_from_problem(p)
    A, _, _, _ = o.local_correction_system(0, 0.6)
    assert np.linalg.eigvalsh(A.toarray()).min() < 0.0
    d, _ = discretize(p)
    with pytest.raises(NativeError, match='not SPD'):
        d.solve_for_local_corrections([0], 0.6)


def test_local_correction_argument_checks():
    from pylrbms_amd._native import NativeError
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    p = _problem('multiscale_problem', {'num_subdomains': [2, 2], 'coarse_per_subdomain': 2})
    d, _ = discretize(p)
    eng = d.engine
    with pytest.raises(NativeError):
        eng.local_corrections(d.theta(0.5), [7])                 # subdomain index out of range
    with pytest.raises(NativeError):
        eng.local_corrections(d.theta(0.5), [0], max_iter=2)     # not converged is an error, not a silent result


def test_enrich_local_and_ragged_reduced_model_match_the_oracle():
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    from pylrbms_amd.reductor import ExtensionError, LRBMSReductor
    p = _problem('OS2015_academic_problem', {'num_subdomains': [3, 3], 'half_num_fine_elements_per_subdomain_and_dim': 12})
    d, data = discretize(p)
    o = oracle_from_problem(p)
    reductor = LRBMSReductor(d, order=0)
    reductor.extend_basis(d.solve(1.0))
    mu = 0.1
    rd = reductor.reduce()
    U = rd.solve(mu)
    # reference API, one subdomain (reductor.py:75-78) ...
    reductor.enrich_local(4, U, mu)
    assert reductor.local_sizes() == [2, 2, 2, 2, 3, 2, 2, 2, 2]
    with pytest.raises(ExtensionError):
        reductor.enrich_local(4, U, mu)                          # the corrector depends on (ii, mu) only: now in the span
    # ... and the batched form used by AdaptiveEnrichment
    grown = reductor.enrich_local_batch([0, 4, 8], U, mu)
    assert grown == [0, 8] and reductor.local_sizes() == [3, 2, 2, 2, 3, 2, 2, 2, 3]
    bases = reductor.bases
    V = [bases['domain_{}'.format(ii)].tensor[0].cpu().numpy() for ii in range(o.S)]
    assert [v.shape[1] for v in V] == reductor.local_sizes()
    # the new vector spans the oracle's corrector together with the old basis
    ref = o.solve_for_local_correction(4, mu)
    coef, res, *_ = np.linalg.lstsq(V[4], ref, rcond=None)
    assert np.abs(V[4] @ coef - ref).max() < 1e-7 * np.abs(ref).max()

    rd = reductor.reduce()
    assert rd.solution_space.dim == sum(reductor.local_sizes())
    u = rd.solve(mu)
    ored = OracleReductor(o, V).reduce()
    u_o = ored.solve(mu)
    N = reductor.basis_size()
    for ii in range(o.S):
        got = u.tensor[ii, :, 0].cpu().numpy()
        assert np.abs(got[:len(u_o[ii])] - u_o[ii]).max() < 1e-7 * max(np.abs(x).max() for x in u_o)
        assert (got[len(u_o[ii]):] == 0.0).all()                 # padded unknowns stay exactly zero
    eta, (nc, r, df), ind = rd.estimate(u, mu=mu, decompose=True)
    eta_o, (nc_o, r_o, df_o), ind_o = ored.estimate(u_o, mu, decompose=True)
    assert abs(eta - eta_o) < 1e-7 * eta_o
    for a, b in ((nc[:, 0], nc_o), (r[:, 0], r_o), (df[:, 0], df_o)):
        assert np.abs(a - b).max() < 1e-7 * np.abs(b).max()
    assert N == 3


def test_adaptive_enrichment_loop():
    """online_adaptive_lrbms.py:121-139 / online_enrichment.py:63-93.  At the reference's HEAD the corrector depends on
    (subdomain, mu) only (the Dirichlet lift by the current solution is commented out, block_swipdg.py:250-261), so for
    one mu every subdomain can gain exactly one vector; the loop is checked for its mechanics (Doerfler + age marking,
    ragged growth, step limit) and its final estimate against the oracle on the very same bases."""
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    from pylrbms_amd.online_enrichment import AdaptiveEnrichment
    from pylrbms_amd.reductor import LRBMSReductor
    p = _problem('OS2015_academic_problem', {'num_subdomains': [4, 4], 'half_num_fine_elements_per_subdomain_and_dim': 16})
    d, data = discretize(p)
    o = oracle_from_problem(p)
    reductor = LRBMSReductor(d, order=0)
    rd = reductor.reduce()
    mu = d.parse_parameter(0.1)
    eta0 = rd.estimate(rd.solve(mu), mu=mu)
    history = []
    loop = AdaptiveEnrichment(p, d, data['block_space'], reductor, rd, target_error=1e-3, marking_doerfler_theta=0.8,
                              marking_max_age=2)
    U, rd2, red2 = loop.solve(mu, enrichment_steps=4, callback=lambda rd_, U_, mu_, info: history.append(dict(info)))
    assert red2 is reductor and rd2 is loop.rd and len(history) == 5
    assert history[0]['eta'] == pytest.approx(eta0, rel=1e-12) and history[0]['local_problem_solves'] == 0
    for h in history:
        assert h['global RB size'] == sum(h['local RB sizes'])
    assert 1 <= history[1]['local_problem_solves'] < 16            # Doerfler marking picks a strict subset first
    assert sorted(set(history[1]['local RB sizes'])) == [1, 2]     # ragged after the first round
    assert history[-1]['local RB sizes'] == [2] * 16               # age marking reaches everyone within 3 rounds
    # final state against the oracle on the same (device-built) bases
    V = [reductor.bases['domain_{}'.format(ii)].tensor[0].cpu().numpy() for ii in range(o.S)]
    oreductor = OracleReductor(o, V)
    ored = oreductor.reduce()
    u_o = ored.solve(0.1)
    eta_o = ored.estimate(u_o, 0.1)
    assert abs(history[-1]['eta'] - eta_o) < 1e-7 * eta_o
    rec_o = np.stack(oreductor.reconstruct(u_o))
    assert np.abs(reductor.reconstruct(U).data.reshape(o.S, o.n) - rec_o).max() < 1e-7 * np.abs(rec_o).max()


@pytest.mark.parametrize('shape, kc, N0, conv', [((6, 5), 4, 38, None), ((9, 8), 2, 18, None), ((5, 5), 2, 5, None),
                                                   ((5, 4), 2, 6, {'oswald_vertex_patch': True})])
def test_incremental_reprojection_equals_the_whole_pass_bitwise(shape, kc, N0, conv):
    """``reduce(touched=marked)`` (reference: online_enrichment.py:52 re-reduces everything after reductor.py:75-78): after the bases
    of a few subdomains grew inside a reserved slab, the fused pass over marked + neighbours -- one int32 indirection in front of
    the workgroup -> subdomain map (lrbms_fused_set_subset) -- leaves EVERY array of the reduced model bit-identical to a whole
    ``reduce()`` on the same bases: the rows it rewrites and the rows it does not touch (which therefore cannot depend on a changed
    basis).  Shapes: the config-3 template at N = 40 (k_f1v, k_prep_lds; 30 subdomains, so the whole pass K-splits the projection
    kernel and the subset pass must do the same), 72 subdomains (no split), odd N (k_f1u, streaming sweeps), and the Oswald vertex
    patch, where the diagonal neighbours of a marked subdomain change too."""
    import torch
    from pylrbms_amd import multiscale_problem
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    from pylrbms_amd.reductor import LRBMSReductor
    p = multiscale_problem.init_grid_and_problem({'num_subdomains': list(shape), 'coarse_per_subdomain': kc})
    d, _ = discretize(p, conventions=conv) if conv else discretize(p)
    eng = d.engine
    S, n = eng.S, eng.t.n
    rng = np.random.default_rng(5)
    if N0 % 2 == 0:
        reductor = LRBMSReductor(d, bases={'domain_{}'.format(ii): rng.standard_normal((N0, n)) for ii in range(S)})
        width = reductor.reserve(N0 + 2)
    else:      # an odd slab width (reserve() pads to even ones): ragged bases, subdomain 1 holds the widest and is never marked
        reductor = LRBMSReductor(d, bases={'domain_{}'.format(ii): rng.standard_normal((N0 if ii == 1 else N0 - 2, n))
                                           for ii in range(S)})
        width = reductor.basis_size()
        assert width == N0
    rd0 = reductor.reduce()
    assert reductor.last_reduce_info == {'incremental': False, 'subdomains': S} and rd0.N == width
    names = ('B_sys', 'rhs_red', 'E_red', 'M_red') + tuple('gram{}'.format(i) for i in range(len(rd0.grams)))
    before = [x.clone() for x in (rd0.B_sys, rd0.rhs_red, rd0.E_red, rd0.M_red) + rd0.grams]
    for rnd, marked in enumerate(([0, S // 2, S - 1], sorted(rng.choice(np.arange(2, S), size=max(2, S // 6), replace=False).tolist()))):
        vecs = eng.ctx.from_numpy(rng.standard_normal((len(marked), n, 1)))
        assert all(reductor._extend_marked(marked, vecs))
        rd1 = reductor.reduce(touched=marked)
        info = reductor.last_reduce_info
        assert info['incremental'] and len(marked) <= info['subdomains'] < S
        assert rd1.B_sys.data_ptr() == rd0.B_sys.data_ptr()                # in place: the previous model's arrays
        inc = [x.clone() for x in (rd1.B_sys, rd1.rhs_red, rd1.E_red, rd1.M_red) + rd1.grams]
        rd2 = reductor.reduce()                                             # the whole pass, fresh arrays
        assert not reductor.last_reduce_info['incremental'] and rd2.B_sys.data_ptr() != rd0.B_sys.data_ptr()
        changed = 0
        for name, a, b, c in zip(names, inc, (rd2.B_sys, rd2.rhs_red, rd2.E_red, rd2.M_red) + rd2.grams, before):
            assert torch.equal(a, b), (rnd, name)
            changed += int(not torch.equal(a, c))
        assert changed >= 10                                                # the round did change the model
        rd0, before = rd2, [x.clone() for x in (rd2.B_sys, rd2.rhs_red, rd2.E_red, rd2.M_red) + rd2.grams]
    # an empty round and a round that outgrows the slab
    rd3 = reductor.reduce(touched=[])
    assert reductor.last_reduce_info == {'incremental': True, 'subdomains': 0} and torch.equal(rd3.B_sys, before[0])
    while reductor.basis_size() == width:
        assert reductor._extend_marked([1], eng.ctx.from_numpy(rng.standard_normal((1, n, 1)))) == [True]
    assert reductor.basis_size() == width + 1                               # grown on demand: no previous model of this width
    rd4 = reductor.reduce(touched=[1])
    assert not reductor.last_reduce_info['incremental'] and rd4.N == width + 1


def test_corrector_solves_on_a_sharded_discretization_match_the_single_rank_ones():
    """A rank of a sharded discretization solves the neighbourhood problems of ITS subdomains on a second engine whose
    local set is local + halo (assembled on the rank, no communication): same correctors as the single-rank run."""
    from pylrbms_amd import multiscale_problem
    from pylrbms_amd.engine import Engine
    from pylrbms_amd.parallel import Communicator
    cfg = {'num_subdomains': [4, 3], 'coarse_per_subdomain': 2}

    def engine(comm):
        p = multiscale_problem.init_grid_and_problem(cfg, mpi_comm=comm)
        lam = p['lambda']
        tb = np.array([c.evaluate(p['mu_bar']) for c in lam['coefficients']])
        return p, Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], tb).assemble()

    p, whole = engine(None)
    theta = np.array([c.evaluate(0.37) for c in p['lambda']['coefficients']])
    ref, _ = whole.local_corrections(theta, list(range(whole.S)))
    ref = ref.cpu().numpy()
    seen = []
    for world in (2, 4):
        for rank in range(world):
            _, eng = engine(Communicator(rank, world))
            assert eng.S_ext > eng.S
            corr, info = eng.local_corrections(theta, list(range(eng.S)))
            assert float(info[:, 1].max()) <= 1e-12
            got = corr.cpu().numpy()
            for i, g in enumerate(eng.local):
                assert np.abs(got[i] - ref[g]).max() < 1e-9 * np.abs(ref[g]).max()
                seen.append(g)
    assert sorted(set(seen)) == list(range(whole.S))


def _even(k):
    return k + (k & 1)


def _check_loop_over_many_parameters(p, d, data, reductor, mus, reserve, min_enriching):
    """AdaptiveEnrichment.solve(mu, enrichment_steps=1) for every mu, as online_adaptive_lrbms.py:166-167 does.  After every call:
    the slab is no wider than the widest real basis plus this call's reserve (even, at most 64); a call that leaves the width
    unchanged re-projected incrementally, and then every array of the reduced model equals a whole pass on the same bases, bit
    for bit.  Returns the loop, the last solution and its estimate."""
    import torch
    from pylrbms_amd.online_enrichment import AdaptiveEnrichment
    eng = d.engine
    loop = AdaptiveEnrichment(p, d, data['block_space'], reductor, reductor.reduce(), target_error=1e-12,
                              marking_doerfler_theta=0.8, marking_max_age=2)
    incremental = enriching = 0
    for k, mu in enumerate(mus):
        width, before = reductor.basis_size(), sum(reductor.local_sizes())
        history = []
        U, rd, _ = loop.solve(mu, enrichment_steps=1, callback=lambda rd_, U_, mu_, info: history.append(dict(info)))
        assert len(history) == 2 and history[0]['eta'] > loop.target_error, k
        enriching += sum(reductor.local_sizes()) > before
        N = reductor.basis_size()
        assert N <= min(64, _even(max(reductor.local_sizes()) + reserve)), (k, N, reductor.local_sizes())
        if N == width:
            assert reductor.last_reduce_info['incremental'], k
            incremental += 1
            fresh = eng.project_and_estimate(d._with_halo(reductor._V), eng.alloc_reduce_buffers(N))
            for a, b in zip((rd.B_sys, rd.rhs_red, rd.E_red, rd.M_red) + tuple(rd.grams), list(fresh['sys']) + list(fresh['grams'])):
                assert torch.equal(a, b), k
    assert enriching >= min_enriching and incremental >= 1, (enriching, incremental)
    return loop, U, history[-1]['eta']


def _check_against_the_oracle(p, reductor, U, eta, mu):
    o = oracle_from_problem(p)
    V = [reductor.bases['domain_{}'.format(ii)].tensor[0].cpu().numpy() for ii in range(o.S)]
    oreductor = OracleReductor(o, V)
    ored = oreductor.reduce()
    u_o = ored.solve(mu)
    eta_o = ored.estimate(u_o, mu)
    assert abs(eta - eta_o) < 1e-7 * eta_o
    rec_o = np.stack(oreductor.reconstruct(u_o))
    assert np.abs(reductor.reconstruct(U).data.reshape(o.S, o.n) - rec_o).max() < 1e-7 * np.abs(rec_o).max()


def test_enrichment_loop_over_twenty_parameters():
    """The reference's online phase (online_adaptive_lrbms.py:112-118, 166-167): OS2015 2 x 2, initial_RB_order 0, extended by the
    solutions at mu_min and mu_max, then 20 random mu with one enrichment step each.  The slab must grow with the real bases, not
    by the reserve on every call (which made reduce(touched=) fall back to the whole pass every time and passed N = 64 after about
    13 parameters from config 3's width)."""
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    from pylrbms_amd.reductor import LRBMSReductor
    p = _problem('OS2015_academic_problem', {'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 4})
    d, data = discretize(p)
    reductor = LRBMSReductor(d, order=0)
    for mu in (p['mu_min'], p['mu_max']):
        reductor.extend_basis(d.solve(mu))
    assert reductor.local_sizes() == [3] * 4
    mus = reductor.reduce().parameter_space.sample_randomly(20, seed=17)
    loop, U, eta = _check_loop_over_many_parameters(p, d, data, reductor, mus, reserve=1, min_enriching=5)
    _check_against_the_oracle(p, reductor, U, eta, mus[-1])


def test_enrichment_loop_from_config3_width():
    """Config 3's template and basis size (k_c = 4, N = 40) on 3 x 3 subdomains: 14 enriching parameters stay within N <= 64
    (the reduced solvers' limit) and the final model matches the oracle on the device-built bases."""
    from pylrbms_amd import multiscale_problem
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    from pylrbms_amd.reductor import LRBMSReductor
    p = multiscale_problem.init_grid_and_problem({'num_subdomains': [3, 3], 'coarse_per_subdomain': 4})
    d, data = discretize(p)
    o = oracle_from_problem(p)
    V0 = energy_orthonormalize(make_bases(o.S, o.n, 40, seed=23), o)
    reductor = LRBMSReductor(d, bases={'domain_{}'.format(ii): V0[ii].T for ii in range(o.S)})
    assert reductor.basis_size() == 40
    mus = [(m,) for m in np.random.default_rng(29).uniform(0.1, 1.0, 14)]
    loop, U, eta = _check_loop_over_many_parameters(p, d, data, reductor, mus, reserve=1, min_enriching=10)
    assert 40 < reductor.basis_size() <= 64
    _check_against_the_oracle(p, reductor, U, eta, mus[-1])
