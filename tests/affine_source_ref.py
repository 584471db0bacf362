"""CPU restatement of the stationary path with a parameter-dependent affine source f(mu) = sum_j theta^f_j(mu) f_j, built on
``oracle.lrbms`` the way tests/parabolic_source_ref.py is.  Test infrastructure only.

* The test problem: the OS2015 academic problem with f = {f_cos, 3 * indicator of a box} and coefficients
  [1, (mu > 0.5) (2 mu - 1)]: the second coefficient is 0 on [0.1, 0.5].
* Every quantity at mu is that of the oracle discretization with f frozen at f(mu) (``SumFunction`` with the weights
  theta^f(mu)): its load vector, ||f||^2, sparse solve, estimator and corrector problems."""
import copy

import numpy as np

from common import oracle_from_problem

SMALL = {'num_subdomains': [2, 2], 'half_num_fine_elements_per_subdomain_and_dim': 4}
BOX = [[[-0.5, -0.5], [0.25, 0.5]], 3.0]


def make_problem(config=SMALL):
    """The OS2015 problem dict with the two-component source (built from existing host functions)."""
    from pylrbms_amd import OS2015_academic_problem
    from pylrbms_amd.functions import make_indicator_function_1x1
    from pylrbms_amd.parameters import ExpressionParameterFunctional
    p = OS2015_academic_problem.init_grid_and_problem(config)
    box = make_indicator_function_1x1(p['grid'], [BOX], 'f_box')
    switch = ExpressionParameterFunctional('(diffusion > 0.5) * (2 * diffusion - 1)', p['parameter_type'])
    return dict(p, f={'functions': [p['f'], box], 'coefficients': [1, switch]})


def coefficients(p, mu):
    from pylrbms_amd.parameters import parse_parameter
    mu = parse_parameter(mu, p['parameter_type'])
    return np.array([c.evaluate(mu) if hasattr(c, 'evaluate') else float(c) for c in p['f']['coefficients']])


def frozen_problem(p, mu):
    """The problem dict with f frozen at f(mu): one source function, the product's existing single-source path."""
    from pylrbms_amd.functions import SumFunction
    return dict(p, f=SumFunction(p['f']['functions'], [float(w) for w in coefficients(p, mu)], name='f_frozen'))


class AffineSource:
    """The oracle discretization of a problem dict whose ``f`` is ``{'functions': [...], 'coefficients': [...]}``."""

    def __init__(self, p, quad=None):
        """``quad``: the oracle's ``QuadratureSpec`` (default: the orders the product picks for the problem)."""
        from pylrbms_amd.functions import SumFunction
        self.p = p
        self.funcs = list(p['f']['functions'])
        self.K = len(self.funcs)
        # the same quadrature orders as the product, which builds its engine on sum_j f_j
        kw = {} if quad is None else {'quad': quad}
        self.d = oracle_from_problem(dict(p, f=SumFunction(self.funcs, [1.0] * self.K)), **kw)
        self.b_K = np.stack([self.frozen(np.eye(self.K)[j]).b for j in range(self.K)])      # [K, ndof]

    def parse(self, mu):
        from pylrbms_amd.parameters import parse_parameter
        return parse_parameter(mu, self.p['parameter_type'])

    def coefficients(self, mu):
        return coefficients(self.p, mu)

    def frozen(self, weights):
        """An oracle discretization with f := sum_j weights[j] f_j (everything else shared with the base)."""
        from pylrbms_amd.functions import SumFunction
        o = copy.copy(self.d)
        o._smp_cache = {}
        o.f = SumFunction(self.funcs, [float(w) for w in weights], name='f_frozen')
        o._assemble_rhs()
        return o

    def at(self, mu):
        return self.frozen(self.coefficients(mu))

    def solve(self, mu):
        """[S, n]: the sparse direct solve with f(mu)."""
        return self.at(mu).solve(self.parse(mu))

    def estimate(self, U, mu):
        """(eta, (nc, r, df), local indicators) of the full-order block vector U [S, n] with f(mu)."""
        return self.at(mu).estimate(np.asarray(U), self.parse(mu), decompose=True)

    def local_correction(self, ii, mu):
        return self.at(mu).solve_for_local_correction(ii, self.parse(mu))
