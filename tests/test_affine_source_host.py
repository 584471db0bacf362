"""The parameter-dependent affine source of the stationary path on the host, without a GPU: coefficient evaluation,
parameter-type validation, the refusals that come before any device work, and the linearity of the CPU restatement
(tests/affine_source_ref.py) the GPU tests rely on."""
import numpy as np
import pytest

from affine_source_ref import AffineSource, coefficients, make_problem


def test_coefficients_switch_off_on_part_of_the_range():
    from pylrbms_amd.sources import evaluate_coefficients
    from pylrbms_amd.parameters import parse_parameter
    p = make_problem()
    for mu, want in (([0.3], [1.0, 0.0]), ([0.5], [1.0, 0.0]), ([0.75], [1.0, 0.5]), ([1.0], [1.0, 1.0])):
        got = evaluate_coefficients(p['f']['coefficients'], parse_parameter(mu, p['parameter_type']))
        assert got.dtype == np.float64 and list(got) == want, mu
        assert list(coefficients(p, mu)) == want


def test_source_components_keep_the_plain_source_apart():
    from pylrbms_amd.parameters import ConstantParameterFunctional
    from pylrbms_amd.sources import source_components
    p = make_problem()
    f = p['f']['functions'][0]
    assert source_components(dict(p, f=f)) is None
    assert source_components(dict(p, f={'functions': [f], 'coefficients': [1]})) is None
    # a functional, even a constant one, is a coefficient of mu: the affine path
    assert source_components(dict(p, f={'functions': [f], 'coefficients': [ConstantParameterFunctional(1.)]})) is not None
    assert source_components(dict(p, f={'functions': [f], 'coefficients': [2.0]})) is not None
    funcs, coeffs = source_components(p)
    assert len(funcs) == 2 and len(coeffs) == 2
    with pytest.raises(ValueError):
        source_components(dict(p, f={'functions': [f, f], 'coefficients': [1]}))


def test_coefficient_parameter_types_must_be_contained():
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    from pylrbms_amd.parameters import (ExpressionParameterFunctional, ProductParameterFunctional,
                                        ProjectionParameterFunctional)
    from pylrbms_amd.sources import check_coefficients
    p = make_problem()
    pt = p['parameter_type']
    check_coefficients(p['f']['coefficients'], pt)
    check_coefficients([2.0, ProductParameterFunctional([ProjectionParameterFunctional('diffusion', (1,), (0,)), 3.0])], pt)
    bad = [[ExpressionParameterFunctional('k', {'k': ()})],
           [ProjectionParameterFunctional('diffusion', (2,), (1,))],                  # same name, other shape
           [ProductParameterFunctional([ExpressionParameterFunctional('k', {'k': ()})])]]
    for coeffs in bad:
        with pytest.raises(ValueError, match='parameter_type'):
            check_coefficients(coeffs, pt)
        q = dict(p, f={'functions': p['f']['functions'][:1], 'coefficients': coeffs})
        with pytest.raises(ValueError, match='parameter_type'):
            discretize(q)                                                          # before any device work
    with pytest.raises(NotImplementedError, match='parabolic'):
        check_coefficients([ExpressionParameterFunctional('_t', {'_t': ()})], pt)


def test_sharded_grid_is_refused_before_any_device_work():
    from pylrbms_amd import OS2015_academic_problem
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize

    class TwoRanks:
        rank, size = 0, 2

    p = OS2015_academic_problem.init_grid_and_problem({'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 4},
                                                      mpi_comm=TwoRanks())
    assert len(p['grid'].subdomains_on_rank) < p['grid'].num_subdomains
    q = make_problem()
    p = dict(p, f=dict(q['f'], functions=[p['f'], q['f']['functions'][1]]))
    with pytest.raises(NotImplementedError, match='one rank'):
        discretize(p)


def test_restatement_is_linear_in_the_source():
    ref = AffineSource(make_problem())
    assert ref.K == 2 and np.abs(ref.b_K[1]).max() > 0.0
    for mu in ([0.3], [0.8]):
        th = ref.coefficients(mu)
        b = ref.at(mu).b
        assert np.abs(b - th @ ref.b_K).max() <= 1e-13 * np.abs(b).max(), mu
    # the frozen f at a mu with a zero second component is the first component alone
    assert np.array_equal(ref.at([0.3]).b, ref.frozen([1.0, 0.0]).b)


def test_3d_path_refuses_a_multi_component_source_before_any_device_work():
    import common3d as c3
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import discretize
    from pylrbms_amd.parameters import ExpressionParameterFunctional
    p = c3.make_problem('aniso_2x2x1')
    switch = ExpressionParameterFunctional('(diffusion > 0.5) * (2 * diffusion - 1)', {'diffusion': (1,)})
    pd = {'grid': p['grid'], 'lambda': {'functions': p['lambdas'], 'coefficients': p['thetas']}, 'lambda_bar': p['lambda_bar'],
          'lambda_hat': p['lambda_hat'], 'mu_bar': p['mu_bar'], 'mu_hat': p['mu_hat'],
          'f': {'functions': [p['f'], p['f']], 'coefficients': [1, switch]}}
    with pytest.raises(NotImplementedError, match='2D path only'):
        discretize(pd)
    with pytest.raises(NotImplementedError, match='2D path only'):
        discretize(dict(pd, f={'functions': [p['f']], 'coefficients': [switch]}))


def test_solve_stationary_refuses_a_time_dependent_source():
    """InstationaryDuneDiscretization.solve_stationary with a time-dependent source raises before it reads the engine."""
    from pylrbms_amd.discretize_parabolic_block_swipdg import InstationaryDuneDiscretization
    d = InstationaryDuneDiscretization.__new__(InstationaryDuneDiscretization)
    d._src = {'K': 2}
    with pytest.raises(NotImplementedError, match='depends on time'):
        d.solve_stationary([0.5])
