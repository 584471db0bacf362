"""The NumPy restatement of lrbms_fom_implicit_euler_batch (tests/fom_euler_batch_ref.py), pinned on the CPU, and the host side of
``InstationaryDuneDiscretization.solve_batch``.

- The P1 mass of the restatement is the oracle's L2 product, and the dense reference trajectory equals
  ``oracle.parabolic.OracleParabolic.solve`` on the (4, 3), k_c = 2 grid at three parameters.
- With one column the preconditioner is ``pcg_ref.FomPrecond`` of the step operator, exactly.
- ``iterate`` converges to the first step of the dense reference, also from a non-zero start value, and its ratio is relative to
  the full right-hand side.
- ``solve_batch`` against a recording fake context: chunks of 64, the phi table [nmu, nt + 1, K] with row k at the time of step k,
  views of one panel, the ``as_snapshots`` layout and its limit of 128 vectors, empty ``mus``; ``solve_stationary_batch`` still
  reaches the elliptic batch."""
import types

import numpy as np
import pytest

import fom_euler_batch_ref as ref
import pcg_ref

_ORACLE = {}
MUS = (0.1, 0.37, 1.0)
T_END, NT = 0.05, 3


def _oracle(shape=(4, 3)):
    if shape not in _ORACLE:
        from pylrbms_amd import multiscale_problem
        from common import oracle_from_problem
        p = multiscale_problem.init_grid_and_problem({'num_subdomains': list(shape), 'coarse_per_subdomain': 2})
        d = oracle_from_problem(p)
        _ORACLE[shape] = (p, d, ref.p1_mass(p['grid'].template.area, d.S))
    return _ORACLE[shape]


def _call(mus=MUS, nt=NT, **kw):
    p, d, M = _oracle()
    ths = np.stack([d.theta(mu) for mu in mus])
    phis = np.ones((len(mus), nt + 1, 1))
    return ref.BatchFomEulerRef([A.tocsr() for A in d.A], M, d.S, d.n, ths, T_END / nt, nt, phis, np.asarray(d.b).reshape(1, d.S, d.n),
                                **kw)


def test_mass_is_the_oracle_l2_product():
    p, d, M = _oracle()
    want = d.l2_product.tocsr()
    assert abs(M - want).max() <= 1e-14 * abs(want).max()


def test_reference_trajectory_is_the_oracle_trajectory():
    from oracle.parabolic import OracleParabolic
    p, d, M = _oracle()
    U = _call().trajectories()
    op = OracleParabolic(d, T_END, NT)
    for m, mu in enumerate(MUS):
        want = op.solve(mu).reshape(NT + 1, -1)
        assert np.abs(want[1:]).max() > 0.0
        assert np.abs(U[:, :, m] - want).max() <= 1e-11 * np.abs(want).max(), mu


def test_one_column_is_the_single_solver_preconditioner_exactly():
    p, d, M = _oracle()
    rng = np.random.default_rng(0)
    R = rng.standard_normal((d.S * d.n, 3))
    for coarse in (0, 1):
        c = _call(mus=(0.37,), coarse=coarse)
        F = pcg_ref.FomPrecond(c.As[0], d.S, d.n, coarse)
        B = c.Ms[0]
        assert B.has_coarse == F.has_coarse == (coarse == 1)
        assert np.array_equal(B.Minv, F.Minv)
        if coarse:
            assert np.array_equal(B.A0, F.A0)
        assert np.array_equal(B.apply(R), F.apply(R))


def test_iterate_converges_to_the_first_step_and_scales_its_ratio():
    p, d, M = _oracle()
    rng = np.random.default_rng(1)
    U0 = rng.standard_normal((d.S * d.n, len(MUS))) * 1e-3
    for kw in ({}, {'U0': U0}):
        c = _call(nt=1, **kw)
        X, ratios = c.iterate(300)
        assert ratios.max() < 1e-12, ratios
        U = c.trajectories()
        assert np.abs(X + c.U0 - U[1]).max() <= 1e-9 * np.abs(U[1]).max()
        _, first = c.iterate(0)                                      # |r_0| / |M u_0 + dt b|: 1 from a zero start value only
        assert np.array_equal(first, np.ones(len(MUS))) == (not kw)
        for m in range(len(MUS)):
            b = c.rhs(m, 0, c.U0[:, m])
            assert abs(first[m] - np.linalg.norm(b - c.As[m] @ c.U0[:, m]) / np.linalg.norm(b)) <= 1e-15
    assert np.abs(c.true_residuals(U)).max() < 1e-12 and c.column_errors(U).max() == 0.0


def test_mutants_change_the_second_iterate():
    p, d, M = _oracle()
    mus = np.linspace(0.1, 1.0, 5)
    base, _ = _call(mus=mus, nt=1).iterate(2)
    for kw in (dict(coarse=0), dict(coarse_theta=d.theta(mus[0])), dict(mass_in_blocks=False)):
        X, _ = _call(mus=mus, nt=1, **kw).iterate(2)
        err = (np.linalg.norm(X - base, axis=0) / np.linalg.norm(base, axis=0)).max()
        assert err > 1e-6, (kw, err)


# ------------------------------------------------------------------------------------------------------- solve_batch
class _FakeContext:
    def __init__(self, S, n):
        self.S, self.n, self.calls = S, n, []

    def fom_implicit_euler_batch(self, thetas, dt, nt, A_diag, A_cpl, b_K, phi, U0=None, rtol=None, max_iter=None):
        import torch
        thetas, phi = np.asarray(thetas), np.asarray(phi)
        self.calls.append(dict(thetas=thetas, phi=phi, b_K=b_K, A_diag=A_diag, A_cpl=A_cpl, dt=dt, nt=nt, U0=U0, rtol=rtol, max_iter=max_iter))
        nmu = thetas.shape[0]
        U = torch.zeros(nt + 1, self.S, self.n, nmu, dtype=torch.float64)
        U[:] = torch.as_tensor(thetas[:, 1][None, :] * 100.0 + np.arange(nt + 1)[:, None])[:, None, None, :]    # step k of column m: 100 mu_m + k
        self.panel = U
        return U, {'iterations': 10 * len(self.calls), 'relative_residual': 1e-11 * len(self.calls), 'panel_iterations': [1]}

    def fom_solve_batch(self, thetas, A_diag, A_cpl, phi, b_K, rtol=None, max_iter=None):
        import torch
        self.calls.append(dict(elliptic=True, thetas=np.asarray(thetas), phi=np.asarray(phi)))
        return torch.zeros(self.S, self.n, len(thetas), dtype=torch.float64), {'iterations': 7, 'relative_residual': 1e-12}


class _Coefficient:
    def __init__(self, fn):
        self.fn = fn

    def evaluate(self, mu):
        return float(self.fn(mu))


def _fake_discretization(source, nt=2):
    import torch
    from pylrbms_amd.discretize_parabolic_block_swipdg import ImplicitEulerTimeStepper, InstationaryDuneDiscretization
    from pylrbms_amd.vectorarrays import BlockVectorSpace, SubSpace
    S, n = 3, 12
    d = InstationaryDuneDiscretization.__new__(InstationaryDuneDiscretization)
    d.engine = types.SimpleNamespace(S=S, S_ext=S, t=types.SimpleNamespace(n=n), A_diag=object(), A_cpl=object(),
                                     b=torch.arange(S * n, dtype=torch.float64).reshape(S, n), ctx=_FakeContext(S, n))
    d.parameter_type = {'mu': ()}
    d.lambda_coeffs = [_Coefficient(lambda mu: 1.0), _Coefficient(lambda mu: mu['mu'])]
    d.solution_space = BlockVectorSpace([SubSpace(n, 'u') for _ in range(S)])
    d.T, d.time_stepper, d.initial_data, d._affine_f = 0.5, ImplicitEulerTimeStepper(nt), None, None
    if source:
        d._src = {'coefficients': [2.0, _Coefficient(lambda mu: mu['mu'] * mu['_t']), _Coefficient(lambda mu: 1.0 + mu['_t'])],
                  'b_K': torch.ones(3, S, n, dtype=torch.float64)}
    return d


@pytest.mark.parametrize('source', (False, True))
def test_solve_batch_chunks_at_64_and_hands_the_phi_table_on(source):
    nt = 2
    d = _fake_discretization(source, nt)
    ctx = d.engine.ctx
    mus = [float(v) for v in np.linspace(0.1, 1.0, 70)]
    trajs = d.solve_batch(mus, inverse_options={'precision': 1e-11, 'max_iter': 30000})
    assert isinstance(trajs, list) and len(trajs) == 70
    assert [c['thetas'].shape[0] for c in ctx.calls] == [64, 6]
    assert d.last_solve_info == {'iterations': 30, 'relative_residual': 2e-11}          # summed / the worst of the two calls
    th = np.concatenate([c['thetas'] for c in ctx.calls])
    assert np.array_equal(th, np.stack([[1.0, mu] for mu in mus]))
    ph = np.concatenate([c['phi'] for c in ctx.calls])
    assert ph.shape == (70, nt + 1, 3 if source else 1)
    if source:
        t1 = 0.0 + 0.25                                                                  # accumulated as the time stepper does
        times = [0.0, t1, t1 + 0.25]
        want = np.array([[[2.0, mu * t, 1.0 + t] for t in times] for mu in mus])
        assert np.array_equal(ph, want)
        assert all(c['b_K'] is d._src['b_K'] for c in ctx.calls)
    else:
        assert np.array_equal(ph, np.ones((70, nt + 1, 1)))
        for c in ctx.calls:
            assert tuple(c['b_K'].shape) == (1, 3, 12) and c['b_K'].data_ptr() == d.engine.b.data_ptr()      # a view of b
    for c in ctx.calls:
        assert c['A_diag'] is d.engine.A_diag and c['A_cpl'] is d.engine.A_cpl and c['dt'] == 0.25 and c['nt'] == nt
        assert c['rtol'] == 1e-11 and c['max_iter'] == 30000 and c['U0'] is None
    for m, (mu, U) in enumerate(zip(mus, trajs)):                                        # the columns kept their order
        assert len(U) == nt + 1 and tuple(U.tensor.shape) == (3, 12, nt + 1)
        assert np.array_equal(U.tensor[1, 5].numpy(), 100.0 * mu + np.arange(nt + 1))
    # views of the call's panel: writing the panel shows in the arrays
    ctx.panel[2, 1, 3, 5] = -7.0
    assert float(trajs[64 + 5].tensor[1, 3, 2]) == -7.0
    assert trajs[64].tensor.data_ptr() == ctx.panel.data_ptr()


def test_as_snapshots_layout_and_its_limit():
    nt = 2
    d = _fake_discretization(False, nt)
    mus = [0.1, 0.4, 0.9]
    U = d.solve_batch(mus, as_snapshots=True)
    assert len(U) == len(mus) * nt and U.tensor.is_contiguous()
    want = np.concatenate([100.0 * mu + np.arange(1, nt + 1) for mu in mus])           # steps 1 .. nt, parameter-major
    assert np.array_equal(U.tensor[2, 7].numpy(), want)
    assert len(d.solve_batch([0.5] * 64, as_snapshots=True)) == 128
    calls = len(d.engine.ctx.calls)
    with pytest.raises(ValueError):
        d.solve_batch([0.5] * 65, as_snapshots=True)
    assert len(d.engine.ctx.calls) == calls                                              # refused before any solve
    assert len(d.solve_batch([0.5] * 65)) == 65                                          # (the list has no such limit)


def test_empty_mus_and_the_stationary_batch():
    d = _fake_discretization(False)
    with pytest.raises(ValueError):
        d.solve_batch([])
    with pytest.raises(ValueError):
        d.solve_batch([], as_snapshots=True)
    X = d.solve_stationary_batch([0.2, 0.3])
    assert len(X) == 2 and d.engine.ctx.calls[-1].get('elliptic') and d.last_solve_info['iterations'] == 7
    assert np.array_equal(d.engine.ctx.calls[-1]['thetas'], [[1.0, 0.2], [1.0, 0.3]])
    with pytest.raises(NotImplementedError):
        _fake_discretization(True).solve_stationary_batch([0.2])
