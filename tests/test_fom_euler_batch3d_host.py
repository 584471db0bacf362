"""The NumPy restatement of lrbms3_fom_implicit_euler_batch (tests/fom_euler_batch3d_ref.py), pinned on the CPU against the
oracle, and the host side of ``InstationaryDiscretization3D.solve_batch``.

- The mass in the product's TM layout is the oracle's mass matrix, and the dense reference trajectories equal
  ``parabolic3d_ref.Parabolic3D.solve`` per column.
- For one column the reference is ``pcg3d_ref.fom_euler_step`` (the call mean is the column's theta); the preconditioner is SPD.
- The cells of tests/test_fom_euler_batch3d_gpu.py (first step, DT = 0.05, 17 columns, a start value per column) keep every k of
  K_STEPS (no reference ratio below MIN_RATIO), every mutant reference misses the second iterate by more than MUTANT_FLOOR, and
  max |u_0| / max |x_1| stays at 1.6 (below 1.65): forming U[1] - U[0] loses no digit that TOL_X would see.
- ``solve_batch`` against a recording fake context: chunks [64, 6] for 70 parameters, the phi table [nmu, nt + 1, K], b_K for the
  plain and the affine source, views of one panel shaped as ``solve`` returns, the ``as_snapshots`` order and its limit, empty
  ``mus``; ``solve_stationary_batch`` reaches the elliptic batch with the stationary coefficients."""
import types

import numpy as np
import pytest

import common3d as c3
import fom_batch3d_ref as ref3
import fom_euler_batch3d_ref as ref
import pcg3d_ref as r3
import pcg_ref
from test_fom_batch3d_host import _case
from test_pcg_iterates_gpu import K_STEPS, MIN_RATIO, MUTANT_FLOOR

_PARTS = {}
MUS = (0.1, 0.37, 1.0)


def _parts(name):
    """(problem, oracle, template, components A_q, mass, b [S, n]) of a cell."""
    if name not in _PARTS:
        p, o, A_diag, A_cpl, b = _case(name)
        t = p['grid'].template
        _PARTS[name] = (p, o, t, ref3.component_operators(A_diag, A_cpl, t, p['grid'].neighbor_slots), r3.oracle_mass(o), b)
    return _PARTS[name]


def _call(name, mus, nt=1, dt=ref.DT, U0=None, **kw):
    p, o, t, Aq, mass, b = _parts(name)
    ths = np.stack([c3.theta_of(p, mu) for mu in mus])
    return ref.BatchFomEuler3DRef(Aq, mass, o.S, o.n, ths, dt, nt, np.ones((len(mus), nt + 1, 1)), np.asarray(b)[None], U0=U0,
                                  Phi=ref3.default_phi(t), **kw)


def _cell(name, **kw):
    p, o, t, Aq, mass, b = _parts(name)
    mus = ref.cell_mus(ref.NMU)
    ths = np.stack([c3.theta_of(p, mu) for mu in mus])
    return _call(name, mus, U0=ref.start_values(Aq, ths, b), **kw)


@pytest.mark.parametrize('name', ('q3_2x1x2', 'kc_3x1x2'))
def test_mass_in_the_product_layout_is_the_oracle_mass(name):
    from pylrbms_amd.engine3d import QuadratureSpec3D
    p, o, t, _, mass, _ = _parts(name)
    TM = t.tables(QuadratureSpec3D(p.get('data_degree', 2)))['TM']
    got = ref.mass_from_tables(TM, t.elem_type, o.S)
    assert abs(got - mass).max() <= 1e-14 * abs(mass).max()
    assert abs(mass - o.M).max() == 0.0                                  # (the oracle numbers its DoFs [S][n])


def test_reference_trajectories_are_the_oracle_trajectories():
    from parabolic3d_ref import Parabolic3D
    p, o, _, _, _, _ = _parts(ref.SWEEP)
    nt = 3
    v0 = np.random.default_rng(3).standard_normal((o.S * o.n, len(MUS))) * np.abs(o.solve(p['mu'])).max()
    for U0 in (None, v0):
        U = _call(ref.SWEEP, MUS, nt=nt, dt=0.3 / nt, U0=U0).trajectories()
        for m, mu in enumerate(MUS):
            want = Parabolic3D(o, 0.3, nt).solve(mu, U0=None if U0 is None else U0[:, m]).reshape(nt + 1, -1)
            assert np.abs(want[1:]).max() > 0.0
            assert np.abs(U[:, :, m] - want).max() <= 1e-11 * np.abs(want).max(), mu


@pytest.mark.parametrize('kw', ({}, {'coarse': 0}, {'mass_in_blocks': False}))
def test_one_column_is_the_single_stepper_reference(kw):
    p, o, t, Aq, mass, b = _parts(ref.SWEEP)
    mu = 0.37
    th = c3.theta_of(p, mu)
    u0 = ref.start_values(Aq, th[None], b)
    c = _call(ref.SWEEP, (mu,), U0=u0, **kw)
    single = r3.fom_euler_step(Aq, mass, o.S, o.n, ref3.default_phi(t), th, ref.DT, b, u0[:, 0], **kw)
    for k in (0, 1, 2, 6):
        X, ratios = c.iterate(k)
        X1, ratios1 = single.iterate(k)
        assert np.array_equal(X, X1) and np.abs(ratios - ratios1).max() <= 1e-15 * ratios1.max(), (kw, k)


def test_preconditioner_is_spd_with_both_levels_on_the_step_operator_at_the_mean():
    c = _call(ref.SWEEP, MUS)
    assert c.has_coarse and all(M is c.Ms[0] for M in c.Ms)              # one preconditioner per call
    N = c.S * c.n
    lo, asym = pcg_ref.spd_check(pcg_ref.precond_matrix(c.P.apply, N))
    assert lo > 0.0 and asym < 1e-12, (lo, asym)
    A = c.A_bar.toarray()                                                # restated from dense NumPy alone
    D = np.zeros_like(A)
    for e in range(N // 10):
        D[10 * e:10 * e + 10, 10 * e:10 * e + 10] = np.linalg.inv(A[10 * e:10 * e + 10, 10 * e:10 * e + 10])
    p, _, t, Aq, mass, _ = _parts(ref.SWEEP)
    R0 = np.kron(np.eye(c.S), ref3.default_phi(t).T)
    want = D + R0.T @ np.linalg.solve(R0 @ A @ R0.T, R0)
    assert np.abs(pcg_ref.precond_matrix(c.P.apply, N) - want).max() <= 1e-10 * np.abs(want).max()
    tb = ref3.mean_theta(np.stack([c3.theta_of(p, mu) for mu in MUS]))
    assert abs(c.A_bar - (mass + ref.DT * ref3.combine(Aq, tb))).max() == 0.0


def test_iterate_converges_to_the_first_step_and_scales_its_ratio():
    c = _cell(ref.SWEEP)
    X, ratios = c.iterate(400)
    assert ratios.max() < 1e-12, ratios
    U = c.trajectories()
    assert np.abs(X + c.U0 - U[1]).max() <= 1e-9 * np.abs(U[1]).max()
    _, first = c.iterate(0)                                              # |r_0| / |M u_0 + dt b|, not 1: the references differ
    assert np.abs(first - 1.0).min() > 1e-3, first
    for m in range(c.nmu):
        f = c.rhs(m, 0, c.U0[:, m])
        assert abs(first[m] - np.linalg.norm(f - c.As[m] @ c.U0[:, m]) / np.linalg.norm(f)) <= 1e-14 * first[m]
    zero = _call(ref.SWEEP, MUS)                                         # from zero the start residual is the right-hand side
    assert np.array_equal(zero.iterate(0)[1], np.ones(len(MUS)))
    assert np.abs(c.true_residuals(U)).max() < 1e-12 and c.column_errors(U).max() == 0.0


@pytest.mark.parametrize('name', ref.CELL_PROBLEMS)
def test_every_k_is_kept_and_every_mutant_separates(name):
    p, o, t, Aq, mass, b = _parts(name)
    c = _cell(name)
    assert c.has_coarse
    for k in K_STEPS:
        X, ratios = c.iterate(k)
        assert ratios.min() >= MIN_RATIO, (name, k, ratios.min())
        if k == 1:
            lost = np.abs(c.U0).max(axis=0) / np.abs(X).max(axis=0)
            print('FOM-EULER-BATCH-3D host {}: max |u_0| / max |x_1| = {:.2f}'.format(name, lost.max()))
            assert lost.max() <= ref.U0_RATIO, (name, lost.max())
    print('FOM-EULER-BATCH-3D host {}: reference ratio at k = 6: {:.2g} .. {:.2g}'.format(name, ratios.min(), ratios.max()))
    base, _ = c.iterate(2)
    th0 = c3.theta_of(p, ref.cell_mus(ref.NMU)[0])
    for kw in (dict(coarse=0), dict(coarse_theta=th0), dict(mass_in_blocks=False)):
        X, _ = _cell(name, **kw).iterate(2)
        err = r3.miss(X, base)
        print('FOM-EULER-BATCH-3D host {}: mutant {} misses x_2 by {:.1e}'.format(name, sorted(kw)[0], err))
        assert err > MUTANT_FLOOR, (name, kw, err)


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
        self.calls.append(dict(elliptic=True, thetas=np.asarray(thetas), phi=np.asarray(phi), b_K=b_K))
        return torch.zeros(self.S, self.n, len(thetas), dtype=torch.float64), {'iterations': 7, 'relative_residual': 1e-12}


def _fake_discretization(source, nt=2, time_dependent=True):
    import torch
    from pylrbms_amd.discretize_parabolic_block_swipdg import ImplicitEulerTimeStepper
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import InstationaryDiscretization3D
    S, n = 3, 20
    d = InstationaryDiscretization3D.__new__(InstationaryDiscretization3D)
    ops = {'A_diag': object(), 'A_cpl': object(), 'b': torch.arange(S * n, dtype=torch.float64).reshape(S, n)}
    d.engine = types.SimpleNamespace(S=S, S_ext=S, t=types.SimpleNamespace(n=n), ops=ops, ctx=_FakeContext(S, n))
    d.coefficients = [lambda mu: 1.0, lambda mu: mu]
    d.Q = 2
    d.T, d.time_stepper = 0.5, ImplicitEulerTimeStepper(nt=nt, solver_options='operator')
    d.initial_data = torch.zeros(S, n, dtype=torch.float64)
    if source:
        second = (lambda mu, t: mu * t) if time_dependent else (lambda mu: 3.0 * mu)
        d._src = {'coefficients': [2.0, second, lambda mu: mu * mu], 'arity': [0, 2 if time_dependent else 1, 1], 'K': 3,
                  'b_K': torch.ones(3, S, n, dtype=torch.float64)}
    return d


@pytest.mark.parametrize('source', (False, True))
def test_solve_batch_chunks_at_64_and_hands_the_phi_table_on(source):
    nt = 2
    d = _fake_discretization(source, nt)
    ctx = d.engine.ctx
    mus = [float(v) for v in np.linspace(0.1, 1.0, 70)]
    trajs, info = d.solve_batch(mus, rtol=1e-11, max_iter=30000, return_info=True)
    assert isinstance(trajs, list) and len(trajs) == 70
    assert [c['thetas'].shape[0] for c in ctx.calls] == [64, 6]
    assert info == (30, 2e-11) and d.last_solve_info == info              # summed / the worst of the two calls
    th = np.concatenate([c['thetas'] for c in ctx.calls])
    assert np.array_equal(th, np.stack([[1.0, mu] for mu in mus]))
    ph = np.concatenate([c['phi'] for c in ctx.calls])
    assert ph.shape == (70, nt + 1, 3 if source else 1)
    if source:
        want = np.array([[[2.0, mu * (k * 0.25), mu * mu] for k in range(nt + 1)] for mu in mus])      # row k at t_k = k dt
        assert np.array_equal(ph, want)
        assert all(c['b_K'] is d._src['b_K'] for c in ctx.calls)
    else:
        assert np.array_equal(ph, np.ones((70, nt + 1, 1)))
        for c in ctx.calls:
            assert tuple(c['b_K'].shape) == (1, 3, 20) and c['b_K'].data_ptr() == d.engine.ops['b'].data_ptr()      # a view of b
    for c in ctx.calls:
        assert c['A_diag'] is d.engine.ops['A_diag'] and c['A_cpl'] is d.engine.ops['A_cpl'] and c['dt'] == 0.25 and c['nt'] == nt
        assert c['rtol'] == 1e-11 and c['max_iter'] == 30000 and c['U0'] is d.initial_data
    for m, (mu, U) in enumerate(zip(mus, trajs)):                         # shaped as ``solve`` returns; the columns kept their order
        assert tuple(U.shape) == (3, 20, nt + 1)
        assert np.array_equal(U[1, 5].numpy(), 100.0 * mu + np.arange(nt + 1))
    # views of the call's panel: writing the panel shows in the trajectories
    ctx.panel[2, 1, 3, 5] = -7.0
    assert float(trajs[64 + 5][1, 3, 2]) == -7.0
    assert trajs[64].data_ptr() == ctx.panel.data_ptr()
    assert not isinstance(d.solve_batch(mus[:3]), tuple) and len(ctx.calls) == 3


def test_as_snapshots_order_and_its_limit():
    nt = 2
    d = _fake_discretization(False, nt)
    mus = [0.1, 0.4, 0.9]
    U = d.solve_batch(mus, as_snapshots=True)
    assert tuple(U.shape) == (3, 20, len(mus) * nt) and U.is_contiguous()
    want = np.concatenate([100.0 * mu + np.arange(1, nt + 1) for mu in mus])           # steps 1 .. nt, parameter-major
    assert np.array_equal(U[2, 7].numpy(), want)
    assert d.solve_batch([0.5] * 64, as_snapshots=True).shape[2] == 128
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
    X, info = d.solve_stationary_batch([0.2, 0.3], return_info=True)
    last = d.engine.ctx.calls[-1]
    assert tuple(X.shape) == (3, 20, 2) and last.get('elliptic') and info == (7, 1e-12)
    assert np.array_equal(last['thetas'], [[1.0, 0.2], [1.0, 0.3]]) and np.array_equal(last['phi'], np.ones((2, 1)))
    d = _fake_discretization(True, time_dependent=False)                                 # an affine source that does not read the time
    d.solve_stationary_batch([0.2, 0.3])
    last = d.engine.ctx.calls[-1]
    assert last.get('elliptic') and np.array_equal(last['phi'], [[2.0, 3.0 * 0.2, 0.2 * 0.2], [2.0, 3.0 * 0.3, 0.3 * 0.3]])
    assert last['b_K'] is d._src['b_K']
    d = _fake_discretization(True)
    with pytest.raises(NotImplementedError):
        d.solve_stationary_batch([0.2])
    assert not d.engine.ctx.calls                                                        # refused before any solve
