"""Online enrichment on the 3D / P2 path: the Dirichlet correction blocks, the batched neighbourhood corrector
solves (lrbms3_local_correction_solve), ``enrich_local`` / ``enrich_local_batch`` and the ``AdaptiveEnrichment`` loop against the
CPU reference tests/enrichment3d_ref.py (validated in tests/test_enrichment3d_host.py).  PARITY UNPINNED beyond the oracle (no 3D
reference counterpart)."""
import functools

import numpy as np
import pytest

import common3d as c3
import enrichment3d_ref as ref

pytestmark = pytest.mark.gpu


def problem_dict(p):
    return {'grid': p['grid'], 'lambda': {'functions': p['lambdas'], 'coefficients': p['thetas']}, 'lambda_bar': p['lambda_bar'],
            'lambda_hat': p['lambda_hat'], 'f': p['f'], 'mu_bar': p['mu_bar'], 'mu_hat': p['mu_hat']}


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, oracle, discretization with the corrector data) of a common3d problem, built once per module."""
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import discretize
    p = c3.make_problem(name)
    d, _ = discretize(problem_dict(p), online_enrichment=True)
    return p, c3.oracle_of(p), d


@functools.lru_cache(maxsize=None)
def reference_corrector(name, ii):
    p, o, _ = case(name)
    return ref.corrector(o, ii, p['mu'])


@pytest.mark.parametrize('name', ['aniso_2x2x1', 'kc_3x1x2'])
def test_dirichlet_correction_blocks_match_the_reference(name):
    p, o, d = case(name)
    got = d.engine.ops['D_corr'].cpu().numpy()
    want = ref.dcorr_layout(p, o).reshape(got.shape)
    assert np.abs(want).max() > 0.0
    assert c3.rel(got, want) < 1e-11
    empty = ~np.any(want.reshape(-1, 100) != 0.0, axis=1)     # physical sides and padded positions: exactly zero
    assert empty.any() and not np.any(got.reshape(-1, 100)[empty] != 0.0)


@pytest.mark.parametrize('name', ['aniso_2x2x1', 'interior_3x3x3', 'kc_3x1x2', 'q3_2x1x2', 'cfg5_template'])
def test_correctors_of_every_subdomain_in_one_call_match_the_sparse_lu(name):
    p, o, d = case(name)
    rtol = 1e-12
    corr, info = d.solve_for_local_corrections(list(range(o.S)), p['mu'], rtol=rtol, return_info=True)
    corr = corr.cpu().numpy()
    assert corr.shape == (o.S, o.n) and info.shape == (o.S, 2)
    print(name, 'iterations', info[:, 0].min(), info[:, 0].max(), 'residual', info[:, 1].max())
    for ii in range(o.S):
        err = c3.rel(corr[ii], reference_corrector(name, ii))
        print(name, ii, 'relative error', err)
        assert err < 1e-8, (ii, err)
    assert np.all(info[:, 1] <= rtol) and np.all(info[:, 0] >= 1)


def test_a_corrector_does_not_depend_on_the_batch_it_is_solved_in():
    """Bitwise: the centre (all 7 slots) and a corner (4 slots) of the 3 x 3 x 3 grid solved alone, with all 27, and with all 27 in
    reversed order."""
    import torch
    p, o, d = case('interior_3x3x3')
    every = list(range(27))
    all_c, all_i = d.solve_for_local_corrections(every, p['mu'], return_info=True)
    rev_c, rev_i = d.solve_for_local_corrections(every[::-1], p['mu'], return_info=True)
    for ii in (13, 0):
        assert len(p['grid'].neighborhood_of(ii)) == (7 if ii == 13 else 4)
        one_c, one_i = d.solve_for_local_corrections([ii], p['mu'], return_info=True)
        assert torch.equal(one_c[0], all_c[ii]) and torch.equal(one_c[0], rev_c[26 - ii])
        assert np.array_equal(one_i[0], all_i[ii]) and np.array_equal(one_i[0], rev_i[26 - ii])
    assert len(set(all_i[:, 0])) > 1            # the problems do stop at different iterations


def test_a_neighbourhood_that_is_the_whole_domain_gives_the_full_order_solution():
    p, o, d = case('wide_basis')
    corr = d.solve_for_local_correction(0, None, p['mu'])
    U = d.solve(p['mu'], rtol=1e-12)
    assert c3.rel(corr.cpu().numpy(), U[0].cpu().numpy()) < 1e-8
    assert c3.rel(corr.cpu().numpy(), o.solve(p['mu'])[o.dofs_of(0)]) < 1e-8


def test_the_result_does_not_depend_on_the_content_of_the_work_buffer():
    import torch
    p, o, d = case('kc_3x1x2')
    eng = d.engine
    ops, th, marked = eng.ops, d.theta(p['mu']), [5, 0, 3]
    size = eng.ctx.local_correction_work_size(len(marked))
    out = []
    for fill in (float('nan'), 0.0):
        work = torch.full((size,), fill, dtype=torch.float64, device='cuda')
        corr, info = eng.ctx.local_correction_solve(eng.Q, th, marked, ops['A_diag'], ops['A_cpl'], ops['D_corr'], ops['b'], rtol=1e-12,
                                                    work=work)
        out.append((corr, info))
    assert torch.equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert bool(torch.isfinite(out[0][0]).all())


def test_error_paths_are_errors_not_faults():
    from pylrbms_amd._native import NativeError
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D, discretize
    from pylrbms_amd.grid3d import make_grid3d
    p, o, d = case('aniso_2x2x1')
    with pytest.raises(NativeError, match=r'\(-4\).*subdomain'):                  # LRBMS_E_NOT_CONVERGED
        d.solve_for_local_corrections([0, 1], p['mu'], max_iter=1)
    for bad in ([1, 1], [0, o.S], [-1]):
        with pytest.raises(NativeError, match=r'\(-1\)'):                        # LRBMS_E_INVALID
            d.engine.local_corrections(d.theta(p['mu']), bad)
    # an indefinite neighbourhood operator (cells of aspect ratio 3): p.Ap <= 0 is reported, never returned as a corrector
    ps, os_, ds = case('q1_strip')
    lows = []
    for ii in range(os_.S):
        A = ref.hood_system(os_, ii, ps['mu']).toarray()
        lows.append(np.linalg.eigvalsh(0.5 * (A + A.T)).min())
    print('q1_strip: smallest eigenvalues of the neighbourhood operators', lows)
    assert min(lows) < 0.0
    with pytest.raises(NativeError, match=r'\(-4\).*subdomain'):
        ds.solve_for_local_corrections(list(range(os_.S)), ps['mu'])
    # sharded grid: refused before any device work
    sharded = dict(problem_dict(p), grid=make_grid3d(num_subdomains=p['P'], cubes_per_subdomain_and_dim=p['kc'], kappa=p['kappa'],
                                                     rank=0, world_size=2))
    with pytest.raises(NotImplementedError, match='online_enrichment'):
        discretize(sharded, online_enrichment=True)
    # the default discretize carries no corrector data
    d0, _ = discretize(problem_dict(p))
    assert 'D_corr' not in d0.engine.ops
    red0 = LRBMSReductor3D(d0)
    for call in (lambda: red0.enrich_local_batch([0], None, p['mu']), lambda: red0.enrich_local(0, None, p['mu']),
                 lambda: d0.solve_for_local_correction(0, None, p['mu']), lambda: d0.solve_for_local_corrections([0], p['mu'])):
        with pytest.raises(NotImplementedError, match='online_enrichment=True'):
            call()


def test_enrich_local_and_the_ragged_reduced_model_match_the_oracle():
    """Order-0 bases plus one snapshot; enrich subdomain 1, then the batch [0, 3]: the bases grow only there, each new column
    spans the reference corrector together with the old basis, and the ragged reduced model is the oracle's on the same bases."""
    from oracle.lrbms3d import Reductor3D
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import ExtensionError3D, LRBMSReductor3D
    p, o, d = case('aniso_2x2x1')
    mu = p['mu']
    red = LRBMSReductor3D(d, order=0)
    red.extend_basis(d.solve(0.2, rtol=1e-12))
    assert red.local_sizes() == [2] * o.S
    red.enrich_local(1, None, mu)
    assert red.local_sizes() == [2, 3, 2, 2]
    assert red.enrich_local_batch([0, 3], None, mu) == [0, 3]
    assert red.local_sizes() == [3, 3, 2, 3] and red.basis_size() == 3
    Vh = red.bases.cpu().numpy()
    assert np.all(Vh[2, :, 2] == 0.0)
    for ii in (0, 1, 3):
        want = reference_corrector('aniso_2x2x1', ii)
        coef = np.linalg.lstsq(Vh[ii], want, rcond=None)[0]
        assert np.abs(Vh[ii] @ coef - want).max() < 1e-7 * np.abs(want).max(), ii
    rd = red.reduce()
    assert rd.solution_space.dim == 11
    bases_o = [Vh[ii][:, :nl] for ii, nl in enumerate(red.local_sizes())]
    ored = Reductor3D(o, bases_o)
    ord_ = ored.reduce()
    for m_ in (mu, 0.9):
        u = rd.solve(m_, rtol=1e-13)
        uo = ord_.solve(m_)
        assert float(u[2, 2].abs()) == 0.0                                  # the padded unknown
        assert c3.rel(red.reconstruct(u).cpu().numpy().ravel(), ored.reconstruct(uo)) < 1e-7
        eta_o = ord_.estimate(uo, m_)
        assert abs(rd.estimate(u, m_) - eta_o) < 1e-7 * eta_o
    with pytest.raises(ExtensionError3D):
        red.enrich_local(1, None, mu)                                        # the same corrector again: already in the span
    assert red.enrich_local_batch([1], None, mu) == []                       # ... skipped in the batch form
    assert red.local_sizes() == [3, 3, 2, 3]


def test_the_corrector_of_an_affine_source_uses_the_load_at_mu():
    import affine_source3d_ref as asr
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import discretize
    p = c3.make_problem('aniso_2x2x1')
    src = asr.AffineSource3D(p)
    d, _ = discretize(asr.problem_dict(p), online_enrichment=True)
    mu = 0.8
    c = src.coefficients(mu)
    assert c[1] > 0.0                                                        # the second component is switched on at this mu
    o = src.at(mu)
    assert c3.rel(o.b, sum(cj * src.component(j).b for j, cj in enumerate(c))) < 1e-14
    corr = d.solve_for_local_corrections([0, 2], mu).cpu().numpy()
    for k, ii in enumerate((0, 2)):
        assert c3.rel(corr[k], ref.corrector(o, ii, mu)) < 1e-8
        assert c3.rel(corr[k], ref.corrector(src.d, ii, mu)) > 1e-3          # not the load of sum_j f_j


def test_adaptive_enrichment_loop_in_3d():
    """``AdaptiveEnrichment`` (online_enrichment.py) with the 3D objects as they are: Doerfler marking with theta < 1 and age
    marking, three enrichment rounds on the 3 x 3 x 3 grid."""
    from oracle.lrbms3d import Reductor3D
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    from pylrbms_amd.online_enrichment import AdaptiveEnrichment
    p, o, d = case('interior_3x3x3')
    mu = p['mu']
    red = LRBMSReductor3D(d, order=0)
    want = o.solve(mu)
    history = []

    def callback(rd, U, mu_, data):
        err = red.reconstruct(U).cpu().numpy().ravel() - want
        history.append(dict(data, energy_error=np.sqrt(o.energy_norm2(err, mu_))))
    loop = AdaptiveEnrichment(problem_dict(p), d, d.solution_space, red, red.reduce(), target_error=0.0,
                              marking_doerfler_theta=0.5, marking_max_age=2)
    U, rd, red_out = loop.solve(mu, enrichment_steps=3, callback=callback)
    assert red_out is red and len(history) == 4
    for h in history:
        assert h['global RB size'] == sum(h['local RB sizes']) and len(h['local RB sizes']) == o.S
    assert history[0]['local_problem_solves'] == 0 and 0 < history[1]['local_problem_solves'] < o.S      # a strict subset
    sizes = [h['global RB size'] for h in history]
    print('sizes', sizes, 'marked', [h['local_problem_solves'] for h in history], 'eta', [h['eta'] for h in history],
          'energy error', [h['energy_error'] for h in history])
    assert sizes[0] == o.S and all(b > a for a, b in zip(sizes, sizes[1:]))
    # ragged bases after a round that marked a strict subset (the corrector of a subdomain depends on mu alone, so at one mu a
    # basis grows at most once and the sizes may level out again later)
    assert max(history[1]['local RB sizes']) > min(history[1]['local RB sizes'])
    # nested spaces: the Galerkin error in the energy norm does not increase
    for a, b in zip(history, history[1:]):
        assert b['energy_error'] <= a['energy_error'] * (1.0 + 1e-10)
    assert history[-1]['energy_error'] < history[0]['energy_error']
    # the final reduced model is the oracle's on the final bases
    Vh = red.bases.cpu().numpy()
    ored = Reductor3D(o, [Vh[ii][:, :nl] for ii, nl in enumerate(red.local_sizes())])
    ord_ = ored.reduce()
    uo = ord_.solve(mu)
    assert c3.rel(red.reconstruct(U).cpu().numpy().ravel(), ored.reconstruct(uo)) < 1e-7
    eta_o = ord_.estimate(uo, mu)
    assert abs(history[-1]['eta'] - eta_o) < 1e-7 * eta_o
