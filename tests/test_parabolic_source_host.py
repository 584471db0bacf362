"""The time-dependent source of the parabolic path on the host, without a GPU: the artificial-channels problem data, the
coefficient table phi, the parameter functionals it needs, and self-checks of the CPU restatement
(tests/parabolic_source_ref.py) that the GPU tests rely on."""
import numpy as np
import pytest

from common import oracle_from_problem
from parabolic_source_ref import ParabolicSource, phi_table

CONFIG = {'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 8}


def _problem(config=CONFIG):
    from pylrbms_amd import artificial_channels_problem
    return artificial_channels_problem.init_grid_and_problem(config)


def test_problem_file_imports_and_has_the_reference_layout():
    p = _problem()
    assert p['parameter_type'] == {'switch': (1,)}
    assert p['parameter_range'] == (0.01, 1)
    assert len(p['lambda']['functions']) == 4 and len(p['lambda']['coefficients']) == 4
    assert len(p['f']['functions']) == 2 and len(p['f']['coefficients']) == 2
    mu = {'switch': [0.3]}
    assert [c.evaluate(mu) for c in p['lambda']['coefficients']] == [0.01, 1.0, 1.0, 0.3]


def test_half_below_four_is_refused_as_in_the_reference():
    from pylrbms_amd import artificial_channels_problem
    with pytest.raises(AssertionError):
        artificial_channels_problem.init_grid_and_problem({'num_subdomains': [8, 8], 'half_num_fine_elements_per_subdomain_and_dim': 2})


@pytest.mark.parametrize('config', [CONFIG, {'num_subdomains': [4, 4], 'half_num_fine_elements_per_subdomain_and_dim': 8}])
def test_every_data_component_is_non_zero_on_the_mesh(config):
    """Every indicator box is hit by element centres: each lambda and f component is non-zero somewhere, and lambda_bar is the
    affine combination at mu_bar."""
    from pylrbms_amd.engine import element_points
    p = _problem(config)
    g = p['grid']
    pts, c, k = element_points(g, range(g.num_subdomains))
    for fn in p['lambda']['functions'] + p['f']['functions']:
        assert np.abs(np.asarray(fn(pts, c, k))).max() > 0.0, fn.name
    th = [cf.evaluate(p['mu_bar']) for cf in p['lambda']['coefficients']]
    comb = sum(t * np.asarray(fn(pts, c, k)) for t, fn in zip(th, p['lambda']['functions']))
    assert np.abs(comb - np.asarray(p['lambda_bar'](pts, c, k))).max() < 1e-14
    assert np.asarray(p['lambda_bar'](pts, c, k)).min() >= 0.01


def test_indicator_function_uses_closed_boxes_at_the_element_centre():
    from pylrbms_amd.functions import make_indicator_function_1x1
    f = make_indicator_function_1x1(None, [[[[0.0, 0.0], [0.5, 0.5]], 2.0], [[[0.5, 0.0], [1.0, 1.0]], 3.0]], 'two')
    centres = np.array([[0.25, 0.25], [0.5, 0.5], [0.75, 0.9], [0.25, 0.75]])
    x = np.zeros((4, 3, 2))                      # the points do not matter, the centre decides
    v = np.asarray(f(x, centres))
    assert v.shape == (4, 3)
    assert list(v[:, 0]) == [2.0, 5.0, 3.0, 0.0]


def test_function_arithmetic():
    from pylrbms_amd.functions import make_constant_function_1x1, make_expression_function_1x1
    a = make_constant_function_1x1(None, 2.0)
    b = make_expression_function_1x1(None, 'x', 'x[0]', order=1)
    x = np.array([[[0.5, 0.0]]])
    c = np.array([[0.5, 0.0]])
    assert float((a - b)(x, c, None)[0, 0]) == 1.5 and float((a + b)(x, c, None)[0, 0]) == 2.5
    assert (a - b).order == 1


def test_expression_parameter_functional_with_none_and_comparisons():
    from pylrbms_amd.parameters import ExpressionParameterFunctional, Parameter
    minus_one = ExpressionParameterFunctional('-1', None)
    assert minus_one.evaluate() == -1.0 and minus_one.evaluate({'switch': [0.4]}) == -1.0
    switch = ExpressionParameterFunctional('sin(2 * 2 * pi * _t) > 0', {'_t': ()})
    assert switch.evaluate({'_t': 0.1}) == 1.0 and switch.evaluate({'_t': 0.3}) == 0.0
    # a parameter with more components than the functional's type (mu plus the time)
    assert switch.evaluate(Parameter({'switch': np.array([0.4]), '_t': np.array(0.1)})) == 1.0
    # what evaluated before evaluates as before
    assert ExpressionParameterFunctional('diffusion', {'diffusion': (1,)}).evaluate([0.3]) == 0.3
    assert ExpressionParameterFunctional('1.', {'diffusion': (1,)}).evaluate([0.3]) == 1.0


def test_phi_table_switch_edges_follow_accumulated_time():
    """t = 0.25, 0.5, ... are reached by t += dt; the switch sin(4 pi t) > 0 is then decided by the rounding of t: at T = 1,
    nt = 20 the accumulated t of step 5 is 0.25 (sin = +1.2e-16: on), of step 10 0.5000000000000001 (sin < 0: off)."""
    p = _problem()
    coeffs = p['f']['coefficients']
    T, nt = 1.0, 20
    phi = phi_table(coeffs, {'switch': np.array([0.5])}, T, nt)
    assert phi.shape == (nt + 1, 2)
    assert np.all(phi[:, 1] == -1.0)
    t, ts = 0.0, [0.0]
    for _ in range(nt):
        t += T / nt
        ts.append(t)
    expect = [1.0 if np.sin(4 * np.pi * tk) > 0 else 0.0 for tk in ts]
    assert list(phi[:, 0]) == expect
    assert phi[0, 0] == 0.0                      # sin(0) = 0 is not > 0
    assert ts[5] == 0.25 and phi[5, 0] == 1.0
    assert ts[10] != 0.5 and phi[10, 0] == 0.0
    assert list(phi[1:5, 0]) == [1.0] * 4 and list(phi[11:15, 0]) == [1.0] * 4


def test_restatement_with_two_components_of_weight_one_is_the_single_f_oracle():
    """K = 2 with f = f_a + f_b and phi = (1, 1): the restatement's trajectory and estimate equal those of the single-f oracle."""
    from oracle.parabolic import OracleParabolic
    from pylrbms_amd import OS2015_academic_problem
    from pylrbms_amd.functions import make_expression_function_1x1
    from pylrbms_amd.parameters import ConstantParameterFunctional
    p = OS2015_academic_problem.init_grid_and_problem({'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 4})
    fa = make_expression_function_1x1(None, 'x', '0.25*pi*pi*(cos(0.5*pi*x[0])*cos(0.5*pi*x[1]))', order=2, name='fa')
    fb = make_expression_function_1x1(None, 'x', '0.25*pi*pi*(cos(0.5*pi*x[0])*cos(0.5*pi*x[1]))', order=2, name='fb')
    p2 = dict(p, f={'functions': [fa, fb], 'coefficients': [ConstantParameterFunctional(1.0), 1.0]})
    T, nt, mu = 0.5, 4, [0.4]
    ref = ParabolicSource(p2, T, nt)
    assert np.all(ref.phi(mu) == 1.0)
    single = OracleParabolic(oracle_from_problem(p), T, nt)
    U, U1 = ref.solve(mu), single.solve(mu)
    assert np.abs(U - U1).max() <= 1e-12 * np.abs(U1).max()
    est, parts = ref.estimate(U1, mu)
    est1, parts1 = single.estimate(U1, ref.parse(mu))
    for a, b in zip(parts, parts1):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    assert abs(est - est1) <= 1e-12 * est1
    # the Gram of the two halves: every entry is a quarter of ||f||^2
    F2 = ref.gram()
    assert np.allclose(F2.sum(axis=(1, 2)), ref.d.local_eta_rf_squared, rtol=1e-12, atol=0)


def test_restatement_with_one_component_gram_is_f2():
    p = _problem()
    p1 = dict(p, f={'functions': [p['f']['functions'][1]], 'coefficients': [p['f']['coefficients'][1]]})
    ref = ParabolicSource(p1, 1.0, 4)
    frozen = ref.frozen([1.0])
    assert np.allclose(ref.gram()[:, 0, 0], frozen.local_eta_rf_squared, rtol=1e-14, atol=0)
    assert np.all(ref.phi({'switch': [0.5]}) == -1.0)


def test_refusals_before_any_device_work():
    """Sharded discretizations, the elliptic reconstruction with such a source and the stationary elliptic path keep raising
    NotImplementedError (all three are refused before an engine is built)."""
    from pylrbms_amd import artificial_channels_problem
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize as discretize_ell
    from pylrbms_amd.discretize_parabolic_block_swipdg import discretize

    class TwoRanks:
        rank, size = 0, 2

    p = artificial_channels_problem.init_grid_and_problem(CONFIG, mpi_comm=TwoRanks())
    with pytest.raises(NotImplementedError, match='one rank'):
        discretize(p, 1.0, 4)
    p = _problem()
    with pytest.raises(NotImplementedError, match='elliptic_reconstruction'):
        discretize(p, 1.0, 4, elliptic_reconstruction=True)
    with pytest.raises(NotImplementedError):
        discretize_ell(p)
