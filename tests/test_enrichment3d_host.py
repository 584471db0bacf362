"""Host-side tests of the 3D online enrichment: the three checks that validate the CPU reference of the
neighbourhood corrector problems (tests/enrichment3d_ref.py) and the new exports of the library.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

import common3d as c3
import enrichment3d_ref as ref
from oracle.lrbms3d import Discretization3D
from oracle.mesh3d import KuhnMesh3D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ('lrbms3_assemble_dirichlet_correction', 'lrbms3_local_correction_work_size', 'lrbms3_local_correction_solve')


@functools.lru_cache(maxsize=None)
def oracle(name):
    return c3.oracle_of(c3.make_problem(name))


def element_blocks(A, ndof):
    A = A.tocsr()
    out = np.zeros((ndof // 10, 10, 10))
    for e in range(ndof // 10):
        out[e] = A[10 * e:10 * e + 10][:, 10 * e:10 * e + 10].toarray()
    return out


@pytest.mark.parametrize('name', sorted(c3.PROBLEMS))
def test_corrections_of_all_coupling_faces_give_the_all_dirichlet_diagonal_blocks(name):
    """A_q plus the correction on every coupling face, both sides, has the element-diagonal blocks of the operator in which every
    subdomain boundary is a Dirichlet boundary (the oracle's own ``_swipdg(fn, False, True)``)."""
    d = oracle(name)
    for q, fn in enumerate(d.lambda_funcs):
        want = element_blocks(d._swipdg(fn, False, True), d.ndof)
        got = element_blocks(d.A_q[q] + ref.correction_matrix(d, q), d.ndof)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
        assert np.abs(ref.coupling_corrections(d, q)[1]).max() > 1e-3 * np.abs(want).max()      # the correction is not negligible


@pytest.mark.parametrize('kc', [1, 2])
def test_strip_correctors_equal_independent_oracles_on_the_boxes(kc):
    """3 x 1 x 1 strip of cubic cells on [0, 3] x [0, 1]^2: N(0) = {0, 1} with Dirichlet data between 1 and 2 is the problem on the
    box [0, 2] x [0, 1]^2, N(2) = {1, 2} the one on [1, 3] x [0, 1]^2."""
    lams, thetas = [c3._one, c3._lam1], [lambda mu: 1.0, lambda mu: mu]

    def disc(ncubes, nsub, lo, hi):
        mesh = KuhnMesh3D(np.array(ncubes) * kc, nsub, lower_left=lo, upper_right=hi)
        return Discretization3D(mesh, lams, thetas, c3.KAPPA_ANISO, c3._f, c3._lbar, c3._lbar, 0.5, 0.5)
    mu = 0.7
    strip = disc([3, 1, 1], [3, 1, 1], (0.0, 0.0, 0.0), (3.0, 1.0, 1.0))
    left = disc([2, 1, 1], [2, 1, 1], (0.0, 0.0, 0.0), (2.0, 1.0, 1.0))
    right = disc([2, 1, 1], [2, 1, 1], (1.0, 0.0, 0.0), (3.0, 1.0, 1.0))
    assert c3.rel(ref.corrector(strip, 0, mu), left.solve(mu)[left.dofs_of(0)]) <= 1e-12
    assert c3.rel(ref.corrector(strip, 2, mu), right.solve(mu)[right.dofs_of(1)]) <= 1e-12
    # the middle neighbourhood is the whole strip: no correction at all
    assert c3.rel(ref.corrector(strip, 1, mu), strip.solve(mu)[strip.dofs_of(1)]) <= 1e-13


def test_a_neighbourhood_that_is_the_whole_domain_gives_the_global_solution():
    d = oracle('wide_basis')
    mu = c3.PROBLEMS['wide_basis'][6]
    assert d.mesh.neighborhood_of(0) == [0, 1]
    assert np.array_equal(ref.corrector(d, 0, mu), d.solve(mu)[d.dofs_of(0)])


def test_new_exports_are_declared_exported_and_bound():
    import ctypes
    from pylrbms_amd._build import build_native
    from pylrbms_amd._native3d import SIGNATURES3, Native3DContext
    with open(os.path.join(ROOT, 'include', 'lrbms3d_hip.h')) as fh:
        header = fh.read()
    handle = ctypes.CDLL(build_native())
    for name in NEW_EXPORTS:
        m = re.search(r'\b(?:int|int64_t) {}\(([^;]*)\);'.format(name), header)
        assert m, '{} is not declared in include/lrbms3d_hip.h'.format(name)
        assert hasattr(handle, name), '{} is not exported'.format(name)
        assert name in SIGNATURES3, '{} is not bound in SIGNATURES3'.format(name)
        assert len(SIGNATURES3[name][1]) == m.group(1).count(',') + 1, '{}: argument count of the binding'.format(name)
        assert hasattr(Native3DContext, name[len('lrbms3_'):]), '{}: no Native3DContext method'.format(name)


def test_sharded_grids_are_refused_before_an_engine_is_built(monkeypatch):
    import pylrbms_amd.discretize_elliptic_block_swipdg_3d as mod
    from pylrbms_amd.grid3d import make_grid3d

    def no_engine(*a, **k):
        raise AssertionError('an engine was built')
    monkeypatch.setattr(mod, 'Engine3D', no_engine)
    p = c3.make_problem('aniso_2x2x1')
    pd = {'grid': make_grid3d(num_subdomains=p['P'], cubes_per_subdomain_and_dim=p['kc'], kappa=p['kappa'], rank=0, world_size=2),
          'lambda': {'functions': p['lambdas'], 'coefficients': p['thetas']}, 'lambda_bar': p['lambda_bar'],
          'lambda_hat': p['lambda_hat'], 'f': p['f'], 'mu_bar': p['mu_bar'], 'mu_hat': p['mu_hat']}
    with pytest.raises(NotImplementedError, match='online_enrichment'):
        mod.discretize(pd, online_enrichment=True)


def test_extend_marked_is_shared_by_the_2d_and_the_3d_reductor():
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    from pylrbms_amd.reductor import LocalBasisSlab, LRBMSReductor
    assert LRBMSReductor._extend_marked is LocalBasisSlab._extend_marked is LRBMSReductor3D._extend_marked
