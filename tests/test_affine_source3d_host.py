"""Affine sources on the 3D / P2 path, the parts that need no GPU: the C ABI is declared and bound, the refusal rule of
``BlockDiscretization3D``, the one- / two-argument coefficient dispatch, the row convention of the time table, and the linearity
of the oracle restatement (tests/affine_source3d_ref.py) that the GPU tests compare against."""
import os
import re

import numpy as np
import pytest

import common3d as c3
from affine_source3d_ref import FUNCS, PARABOLIC, STATIONARY, AffineSource3D, problem_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ('lrbms3_assemble_source_gram', 'lrbms3_project_sources', 'lrbms3_reduced_source_terms', 'lrbms3_reduced_solve_batch_src',
               'lrbms3_combine_sources', 'lrbms3_fom_implicit_euler_src', 'lrbms3_reduced_implicit_euler_src')


def test_new_exports_are_declared_in_the_header_and_bound():
    from pylrbms_amd._native3d import SIGNATURES3, Native3DContext
    with open(os.path.join(ROOT, 'include', 'lrbms3d_hip.h')) as fh:
        header = fh.read()
    for name in NEW_EXPORTS:
        m = re.search(r'\bint {}\(([^;]*)\);'.format(name), header)
        assert m, '{} is not declared in include/lrbms3d_hip.h'.format(name)
        assert name in SIGNATURES3, '{} is not bound in SIGNATURES3'.format(name)
        assert len(SIGNATURES3[name][1]) == m.group(1).count(',') + 1, '{}: argument count of the binding'.format(name)
        assert hasattr(Native3DContext, name[len('lrbms3_'):]), '{}: no Native3DContext method'.format(name)


def test_every_3d_export_of_the_header_is_bound():
    from pylrbms_amd._native3d import SIGNATURES3
    with open(os.path.join(ROOT, 'include', 'lrbms3d_hip.h')) as fh:
        declared = set(re.findall(r'^(?:int|int64_t|const char\*) (lrbms3_\w+)\(', fh.read(), flags=re.M))
    assert declared == set(SIGNATURES3)


def test_functionals_and_sharded_grids_are_refused_before_an_engine_is_built(monkeypatch):
    import pylrbms_amd.discretize_elliptic_block_swipdg_3d as mod
    from pylrbms_amd.grid3d import make_grid3d
    from pylrbms_amd.parameters import ExpressionParameterFunctional

    def no_engine(*a, **k):
        raise AssertionError('an engine was built')
    monkeypatch.setattr(mod, 'Engine3D', no_engine)
    p = c3.make_problem('aniso_2x2x1')
    switch = ExpressionParameterFunctional('(diffusion > 0.5) * (2 * diffusion - 1)', {'diffusion': (1,)})
    for coeffs, funcs in (([1, switch], FUNCS), ([switch], FUNCS[:1])):
        with pytest.raises(NotImplementedError, match='2D path only'):
            mod.discretize(problem_dict(p, funcs=funcs, coeffs=coeffs))
    grid = make_grid3d(num_subdomains=p['P'], cubes_per_subdomain_and_dim=p['kc'], kappa=p['kappa'], rank=0, world_size=2)
    with pytest.raises(NotImplementedError, match='2D path only'):
        mod.discretize(dict(problem_dict(p), grid=grid))
    # a coefficient that reads the time belongs to the parabolic discretize
    with pytest.raises(NotImplementedError, match='depends on time'):
        mod.discretize(problem_dict(p, coeffs=PARABOLIC))


@pytest.mark.parametrize('coeffs', [STATIONARY, [2.5, -1.0], [lambda mu: mu]])
def test_numbers_and_callables_pass_the_check_up_to_the_device(coeffs, monkeypatch):
    """The check lets plain numbers and callables through: the next thing ``discretize`` does is build the engine."""
    import pylrbms_amd.discretize_elliptic_block_swipdg_3d as mod

    class Reached(Exception):
        pass

    def engine(grid, lambda_funcs, f, *a, **k):
        x = np.array([[0.1, 0.2, 0.3], [0.5, 0.25, 0.75]])
        want = sum(np.asarray(fn(x), dtype=np.float64) for fn in FUNCS[:len(coeffs)])
        assert np.array_equal(np.asarray(f(x)), want)                  # the engine is built on sum_j f_j
        raise Reached()
    monkeypatch.setattr(mod, 'Engine3D', engine)
    with pytest.raises(Reached):
        mod.discretize(problem_dict(c3.make_problem('aniso_2x2x1'), funcs=FUNCS[:len(coeffs)], coeffs=coeffs))


def test_one_component_with_the_literal_coefficient_one_takes_the_plain_path(monkeypatch):
    import pylrbms_amd.discretize_elliptic_block_swipdg_3d as mod
    seen = {}

    class Reached(Exception):
        pass

    def engine(grid, lambda_funcs, f, *a, **k):
        seen['f'] = f
        raise Reached()
    monkeypatch.setattr(mod, 'Engine3D', engine)
    with pytest.raises(Reached):
        mod.discretize(problem_dict(c3.make_problem('aniso_2x2x1'), funcs=FUNCS[:1], coeffs=[1]))
    assert seen['f'] is FUNCS[0]


def test_coefficient_dispatch_is_decided_from_the_signature():
    from pylrbms_amd.sources3d import coefficient_arity, evaluate_stationary, evaluate_table
    calls = []

    def one(mu):
        calls.append(('one', mu))
        return 2 * mu

    def two(mu, t):
        calls.append(('two', mu, t))
        return mu + t

    def raises_type_error(mu):
        raise TypeError('from inside the coefficient')
    assert [coefficient_arity(c) for c in (1, -1.0, one, two, lambda mu, q=3: mu ** q)] == [0, 0, 1, 2, 1]
    with pytest.raises(TypeError):
        coefficient_arity(lambda: 1.0)
    with pytest.raises(TypeError):
        coefficient_arity('mu')
    # the documented rule: a defaulted parameter is a bound constant, the path never supplies it
    assert coefficient_arity(lambda mu, t=0.0: mu + t) == 1
    assert evaluate_table({'coefficients': [lambda mu, t=7.0: mu + t], 'arity': [1]}, 0.5, 0.25, 1).tolist() == [[7.5], [7.5]]
    with pytest.raises(TypeError, match='signature'):
        coefficient_arity(dict.update)               # no readable signature: TypeError, not inspect's ValueError
    src = {'coefficients': [3, one, two], 'arity': [0, 1, 2]}
    tab = evaluate_table(src, 0.5, 0.25, 2)
    assert np.array_equal(tab, [[3.0, 1.0, 0.5], [3.0, 1.0, 0.75], [3.0, 1.0, 1.0]])
    assert ('two', 0.5, 0.25) in calls and all(len(c) == 2 for c in calls if c[0] == 'one')
    with pytest.raises(NotImplementedError, match='depends on time'):
        evaluate_stationary(src, 0.5)
    assert np.array_equal(evaluate_stationary({'coefficients': [3, one], 'arity': [0, 1]}, 0.5), [3.0, 1.0])
    # a TypeError from inside a coefficient is not mistaken for a wrong arity: it propagates
    with pytest.raises(TypeError, match='from inside'):
        evaluate_table({'coefficients': [raises_type_error], 'arity': [1]}, 0.5, 0.1, 1)


def test_time_table_rows_are_taken_at_t_k():
    """Row k of ``d.source_coefficients(mu)`` is c(mu, k dt): the switch sin(4 pi t) > 0 with T = 0.5, nt = 4 gives 0 1 1 0 0 -- row 0
    at t = 0, the change inside the trajectory."""
    from pylrbms_amd.discretize_parabolic_block_swipdg import ImplicitEulerTimeStepper
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import InstationaryDiscretization3D
    d = InstationaryDiscretization3D.__new__(InstationaryDiscretization3D)
    d.T, d.time_stepper = 0.75, ImplicitEulerTimeStepper(nt=6, solver_options='operator')
    d._src = {'coefficients': PARABOLIC, 'arity': [2, 0]}
    tab = d.source_coefficients(0.3)
    assert tab.shape == (7, 2)
    want = [float(np.sin(4 * np.pi * k * 0.125) > 0) for k in range(7)]
    assert np.array_equal(tab[:, 0], want) and np.array_equal(tab[:, 1], [-1.0] * 7)
    assert tab[0, 0] == 0.0 and 0.0 < tab[:, 0].sum() < 7.0               # the switch changes value inside the trajectory
    with pytest.raises(NotImplementedError, match='depends on time'):
        d.solve_stationary(0.3)
    d._src = None
    assert np.array_equal(d.source_coefficients(0.3), np.ones((7, 1)))


def test_oracle_restatement_is_linear_in_the_components():
    p = c3.make_problem('aniso_2x2x1')
    src = AffineSource3D(p)
    comps = [src.component(j) for j in range(src.K)]
    for mu in (0.3, 0.9):
        phi = src.coefficients(mu)
        o = src.at(mu)
        for key in ('b', 'bdiv'):
            ref = sum(w * getattr(c, key) for w, c in zip(phi, comps))
            assert np.abs(getattr(o, key) - ref).max() <= 1e-13 * np.abs(ref).max(), key
        assert np.abs(o.f2 - np.einsum('j,sjl,l->s', phi, src.gram(), phi)).max() <= 1e-13 * np.abs(o.f2).max()
    # the second coefficient vanishes for mu <= 0.5: exactly the first component alone
    assert src.coefficients(0.3)[1] == 0.0 and src.coefficients(0.9)[1] > 0.0
    o = src.at(0.3)
    for key in ('b', 'bdiv', 'f2'):
        assert np.array_equal(getattr(o, key), getattr(comps[0], key)), key
    # ... and that is the oracle of the plain problem with f = f_0
    plain = c3.oracle_of(p)
    for key in ('b', 'bdiv', 'f2'):
        assert np.array_equal(getattr(o, key), getattr(plain, key)), key
