"""The NumPy restatement of lrbms3_fom_solve_batch (tests/fom_batch3d_ref.py), pinned on the CPU against the oracle, and the
host side of ``BlockDiscretization3D.solve_batch``.

- The layout map (A_diag / A_cpl -> sparse operator) applied to ``oracle_assembled`` reproduces the oracle's components.
- The preconditioner -- both levels at the call mean -- is symmetric positive definite; for one column it is the single solver's
  (inverse 10 x 10 element blocks plus the Galerkin coarse problem on P1 per subdomain, both at the column's theta).
- ``pcg_iterate`` with it converges to the oracle's direct solve.
- ``mean_theta`` sums in column order.
- The cells of tests/test_fom_batch3d_gpu.py keep every k of K_STEPS: no reference ratio falls below MIN_RATIO, and at k = 6 it
  is still >= 6e-2 with the default load.
- ``solve_batch`` chunks at 64 and hands phi / b_K on (a fake context records the calls)."""
import numpy as np
import pytest

import common3d as c3
import fom_batch3d_ref as ref3
import pcg_ref

_CACHE = {}
CELL_PROBLEMS = ('interior_3x3x3', 'kc_3x1x2', 'q3_2x1x2', 'aniso_2x2x1')


def _case(name):
    """(problem, oracle, the oracle's blocks in the product's layouts with the trailing 100)."""
    if name not in _CACHE:
        p = c3.make_problem(name)
        o = c3.oracle_of(p)
        a = c3.oracle_assembled(p, o)
        A_diag = a['A_diag'].reshape(a['A_diag'].shape[:4] + (100,))
        A_cpl = a['A_cpl'].reshape(a['A_cpl'].shape[:4] + (100,))
        _CACHE[name] = (p, o, A_diag, A_cpl, a['b'])
    return _CACHE[name]


def _ref(name, mus, **kw):
    p, o, A_diag, A_cpl, b = _case(name)
    t = p['grid'].template
    ths = np.stack([c3.theta_of(p, mu) for mu in mus])
    return ref3.BatchFom3DRef(A_diag, A_cpl, t, p['grid'].neighbor_slots, ths, np.ones((len(mus), 1)), b[None], **kw)


@pytest.mark.parametrize('name', ('q3_2x1x2', 'kc_3x1x2', 'q1_strip'))
def test_layout_map_reproduces_the_oracle_components(name):
    p, o, A_diag, A_cpl, _ = _case(name)
    Aq = ref3.component_operators(A_diag, A_cpl, p['grid'].template, p['grid'].neighbor_slots)
    assert len(Aq) == o.Q
    for q in range(o.Q):
        want = o.A_q[q].tocsr()
        assert abs(Aq[q] - want).max() <= 1e-13 * abs(want).max(), (name, q)
    th = c3.theta_of(p, p['mu'])
    want = o.system_matrix(p['mu'])
    assert abs(ref3.combine(Aq, th) - want).max() <= 1e-13 * abs(want).max()


def test_preconditioner_is_spd_with_both_levels_at_the_mean():
    r = _ref('q3_2x1x2', (0.1, 0.37, 1.0))
    assert r.has_coarse and all(M is r.Ms[0] for M in r.Ms)              # one preconditioner per call
    lo, asym = pcg_ref.spd_check(pcg_ref.precond_matrix(r.Ms[0].apply, r.S * r.n))
    assert lo > 0.0 and asym < 1e-12, (lo, asym)
    r0 = _ref('q3_2x1x2', (0.1, 0.37, 1.0), coarse=0)
    assert not r0.has_coarse
    lo, asym = pcg_ref.spd_check(pcg_ref.precond_matrix(r0.Ms[0].apply, r.S * r.n))
    assert lo > 0.0 and asym < 1e-12, (lo, asym)


def test_one_column_is_the_single_solver_preconditioner():
    p, o, _, _, _ = _case('q3_2x1x2')
    mu = 0.37
    r = _ref('q3_2x1x2', (mu,))
    A = o.system_matrix(mu).toarray()                                     # restated from dense NumPy alone
    N, S, n = A.shape[0], o.S, o.n
    D = np.zeros_like(A)
    for e in range(N // 10):
        D[10 * e:10 * e + 10, 10 * e:10 * e + 10] = np.linalg.inv(A[10 * e:10 * e + 10, 10 * e:10 * e + 10])
    R0 = np.kron(np.eye(S), ref3.default_phi(p['grid'].template).T)
    want = D + R0.T @ np.linalg.solve(R0 @ A @ R0.T, R0)
    got = pcg_ref.precond_matrix(r.Ms[0].apply, N)
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize('name', ('q3_2x1x2', 'interior_3x3x3'))
def test_pcg_with_it_reproduces_the_oracle_solve(name):
    p, o, _, _, _ = _case(name)
    mus = (0.1, 0.6, 1.0)
    r = _ref(name, mus)
    X, ratios = r.iterate(400)
    assert ratios.max() < 1e-12, ratios
    for j, mu in enumerate(mus):
        want = o.solve(mu)
        assert np.abs(X[:, j] - want).max() < 1e-8 * np.abs(want).max(), (name, mu)


def test_mean_theta_sums_in_column_order():
    th = np.array([[1.0, 0.1], [1.0, 1e-17], [1.0, 0.7]])
    want = np.array([(1.0 + 1.0 + 1.0) / 3, ((0.1 + 1e-17) + 0.7) / 3])
    assert np.array_equal(ref3.mean_theta(th), want)


def test_mutant_switches_change_the_second_iterate():
    mus = np.linspace(0.1, 1.0, 5)
    p, _, _, _, _ = _case('q3_2x1x2')
    base, _ = _ref('q3_2x1x2', mus).iterate(2)
    for kw in (dict(coarse=0), dict(coarse_theta=c3.theta_of(p, mus[0])), dict(block_theta='own')):
        X, _ = _ref('q3_2x1x2', mus, **kw).iterate(2)
        err = (np.linalg.norm(X - base, axis=0) / np.linalg.norm(base, axis=0)).max()
        assert err > 1e-6, (kw, err)


@pytest.mark.parametrize('name', CELL_PROBLEMS)
def test_every_k_of_the_iterate_tests_is_kept(name):
    from test_pcg_iterates_gpu import K_STEPS, MIN_RATIO
    r = _ref(name, np.linspace(0.1, 1.0, 17))
    for k in K_STEPS:
        _, ratios = r.iterate(k)
        assert ratios.min() >= MIN_RATIO, (name, k, ratios.min())
    assert ratios.min() >= 6e-2, (name, ratios.min())                     # k = 6


# ------------------------------------------------------------------------------------------------------- solve_batch
class _FakeContext:
    def __init__(self, S, n):
        self.S, self.n, self.calls = S, n, []

    def fom_solve_batch(self, thetas, A_diag, A_cpl, phi, b_K, rtol=None, max_iter=None):
        import torch
        thetas, phi = np.asarray(thetas), np.asarray(phi)
        self.calls.append(dict(thetas=thetas, phi=phi, b_K=b_K, A_diag=A_diag, A_cpl=A_cpl, rtol=rtol, max_iter=max_iter))
        nmu = thetas.shape[0]
        X = torch.zeros(self.S, self.n, nmu, dtype=torch.float64)
        X[:] = torch.as_tensor(thetas[:, 1] * phi.sum(axis=1))            # column m carries its own theta and phi
        return X, {'iterations': 10 + len(self.calls), 'relative_residual': 1e-11 * len(self.calls), 'panel_iterations': [1]}


def _fake_discretization(affine):
    import types
    import torch
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import BlockDiscretization3D
    S, n = 3, 20
    d = BlockDiscretization3D.__new__(BlockDiscretization3D)
    ops = {'A_diag': object(), 'A_cpl': object(), 'b': torch.arange(S * n, dtype=torch.float64).reshape(S, n)}
    d.engine = types.SimpleNamespace(S=S, S_ext=S, t=types.SimpleNamespace(n=n), ops=ops, ctx=_FakeContext(S, n))
    d.coefficients = [lambda mu: 1.0, lambda mu: mu]
    d.Q = 2
    if affine:
        d._src = {'coefficients': [2.0, lambda mu: 3.0 * mu, lambda mu: mu * mu], 'arity': [0, 1, 1], 'K': 3,
                  'b_K': torch.ones(3, S, n, dtype=torch.float64)}
    return d


@pytest.mark.parametrize('affine', (False, True))
def test_solve_batch_chunks_at_64_and_hands_the_sources_on(affine):
    d = _fake_discretization(affine)
    ctx = d.engine.ctx
    mus = [float(v) for v in np.linspace(0.1, 1.0, 70)]
    U, info = d.solve_batch(mus, rtol=1e-9, max_iter=123, return_info=True)
    assert tuple(U.shape) == (3, 20, 70) and U.is_contiguous()
    assert [c['thetas'].shape[0] for c in ctx.calls] == [64, 6]
    assert info == (12, 2e-11)                                            # the largest of the two calls
    th = np.concatenate([c['thetas'] for c in ctx.calls])
    ph = np.concatenate([c['phi'] for c in ctx.calls])
    assert np.array_equal(th, np.stack([[1.0, mu] for mu in mus]))
    if affine:
        assert np.array_equal(ph, np.stack([[2.0, 3.0 * mu, mu * mu] for mu in mus]))
        assert all(c['b_K'] is d._src['b_K'] for c in ctx.calls)
    else:
        assert np.array_equal(ph, np.ones((70, 1)))
        for c in ctx.calls:
            assert tuple(c['b_K'].shape) == (1, 3, 20) and c['b_K'].data_ptr() == d.engine.ops['b'].data_ptr()      # a view of b
    for c in ctx.calls:
        assert c['A_diag'] is d.engine.ops['A_diag'] and c['A_cpl'] is d.engine.ops['A_cpl']
        assert c['rtol'] == 1e-9 and c['max_iter'] == 123
    assert np.array_equal(U[0, 0].numpy(), th[:, 1] * ph.sum(axis=1))     # the columns kept their order across the chunks
    assert not isinstance(d.solve_batch(mus[:3]), tuple) and len(ctx.calls) == 3
    with pytest.raises(ValueError):
        d.solve_batch([])
