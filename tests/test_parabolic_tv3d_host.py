"""Time-dependent diffusion coefficients on the 3D / P2 parabolic path on the host, without a GPU.

- The NumPy restatement of the three ``lrbms3_*_tv`` exports (tests/parabolic_tv3d_ref.py) with constant tables reproduces
  ``Parabolic3D.solve``, ``ParabolicReduced3D.solve`` and ``ParabolicReduced3D.estimate`` of tests/parabolic3d_ref.py to 1e-12.
- On the inputs of every cell of tests/test_parabolic_tv3d_gpu.py every fault switch of the restatement misses the right one by more
  than 1e-6 (the device tolerances are 1e-8 or tighter): an export with that fault could not pass there.  Two faults cannot show
  everywhere, by construction: 'column0' is the right table in a call of one column, and with nt = 1 the time mean IS row 1 (the
  solver cells have nt >= 2).
- The table plumbing of the Python layer on a recording fake context, the problem file's ``switch_off_after`` and the declared
  surface."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import common3d as c3
import fom_batch3d_ref as ref3
import fom_euler_batch3d_ref as fe
import parabolic_batch3d_ref as rb
import parabolic_estimate_batch3d_ref as pe
import parabolic_tv3d_ref as tv
from parabolic3d_ref import Parabolic3D, ParabolicReduced3D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ('lrbms3_fom_implicit_euler_batch_tv', 'lrbms3_reduced_implicit_euler_batch_tv',
           'lrbms3_reduced_parabolic_estimate_batch_tv_work_size', 'lrbms3_reduced_parabolic_estimate_batch_tv')
FLOOR = 1e-6

_RED = {}


def _reduced(name, N, pad=0):
    """(problem, oracle, reduced reference, model of the estimate restatement, rhs [S, N], keep [S, N]) from the CPU oracle on the
    bases of the GPU cells; pad > 0: subdomain 1 has ``pad`` vectors fewer, zero-padded."""
    key = (name, N, pad)
    if key not in _RED:
        from test_parabolic_batch3d_host import padded_model
        from test_parabolic_estimate_batch3d_host import _oracle
        p, o = _oracle(name)
        V = c3.make_bases3d(o.S, o.n, N, seed=pe.BASIS_SEED)
        sizes = [N - pad if ii == 1 else N for ii in range(o.S)]
        red = ParabolicReduced3D(o, [V[ii][:, :sizes[ii]] for ii in range(o.S)], 0.75, 3)
        nbr, B, M, rhs, keep = padded_model(p, red, N)
        model = None if pad else pe.model_from_oracle(p, o, red.rd, red.M_blocks, N)
        _RED[key] = (p, o, red, model, dict(nbr=nbr, B=B, M=M, rhs=rhs, keep=keep))
    return _RED[key]


# ------------------------------------------------------------------------------------------------------------ constant tables
def test_constant_tables_reproduce_the_full_order_trajectories():
    from test_fom_euler_batch3d_host import MUS, _parts
    p, o, t, Aq, mass, b = _parts(fe.SWEEP)
    nt, T = 3, 0.3
    ths = np.stack([c3.theta_of(p, mu) for mu in MUS])
    c = tv.BatchFomEulerTv3DRef(Aq, mass, o.S, o.n, tv.constant_table(ths, nt), T / nt, nt, np.ones((len(MUS), nt + 1, 1)),
                                np.asarray(b)[None], Phi=ref3.default_phi(t))
    U = c.trajectories()
    for m, mu in enumerate(MUS):
        want = Parabolic3D(o, T, nt).solve(mu).reshape(nt + 1, -1)
        assert np.abs(want[1:]).max() > 0.0
        assert np.abs(U[:, :, m] - want).max() <= 1e-12 * np.abs(want).max(), mu
    twin = fe.BatchFomEuler3DRef(Aq, mass, o.S, o.n, ths, T / nt, nt, np.ones((len(MUS), nt + 1, 1)), np.asarray(b)[None],
                                 Phi=ref3.default_phi(t))
    assert abs(c.A_bar - twin.A_bar).max() <= 1e-15 * abs(twin.A_bar).max()          # the preconditioner of the twin
    for k in (1, 2, 5):
        assert np.abs(c.iterate(k)[0] - twin.iterate(k)[0]).max() <= 1e-12 * np.abs(twin.iterate(k)[0]).max()


def test_constant_tables_reproduce_the_reduced_trajectories_and_estimates():
    name = 'aniso_2x2x1'
    N = c3.PROBLEMS[name][5]
    p, o, red, model, h = _reduced(name, N)
    nt, dt = red.nt, red.dt
    mus = (0.2, p['mu'], 0.9)
    ths = np.stack([c3.theta_of(p, mu) for mu in mus])
    tab = tv.constant_table(ths, nt)
    U = tv.dense_euler_batch_tv(h['B'], h['M'], h['nbr'], tab, dt, nt, rhs=h['rhs'])
    from test_parabolic_estimate_batch3d_host import _against, _coef
    coef = np.repeat(_coef(o, mus)[:, None, :], nt + 1, axis=1)
    out = tv.estimate_outputs_tv(model, tab, coef, dt, U)
    twin = pe.estimate_outputs(model, ths, coef[:, 0], dt, U)
    for m, mu in enumerate(mus):
        u_o = red.solve(mu)
        assert np.abs(U[..., m].reshape(nt + 1, -1) - u_o).max() <= 1e-12 * np.abs(u_o).max(), mu
        est, parts = red.estimate(U[..., m].reshape(nt + 1, -1), mu)
        _against(out, m, est, parts, dt, 1e-12, (name, mu))
    for k in ('eta_loc', 'time_deriv_nc', 'time_residual', 'eta', 'est'):
        assert np.abs(out[k] - twin[k]).max() <= 1e-14 * np.abs(twin[k]).max(), k
    # the time means of a constant table are its rows up to the rounding of the sum; nt = 1: row 1 exactly, whatever row 0 holds
    assert np.abs(tv.time_means(tab) - ths).max() <= 2.0 ** -52
    one = tv.switch_table(3, 1, o.Q)
    assert np.array_equal(tv.time_means(one), one[:, 1])


# -------------------------------------------------------------------------------- every fault misses at the cells of the GPU test
def _step_faults(nmu):
    return [f for f in tv.STEP_FAULTS if not (f == 'column0' and nmu == 1)]


@pytest.mark.parametrize('name, N, nmu, nt', tv.RED_CELLS + (tv.RED_START_CELL, tv.RED_PAD_CELL))
def test_stepping_faults_miss_at_the_reduced_cells(name, N, nmu, nt):
    pad = 2 if (name, N, nmu, nt) == tv.RED_PAD_CELL else 0
    p, o, red, model, h = _reduced(name, N, pad)
    tab = tv.switch_table(nmu, nt, o.Q, base=pe.cell_thetas(p, nmu))
    assert (tab > 0.0).all() and (tab[:, 1, -1] > 5.0 * tab[:, 2, -1]).all()               # the switch between the steps 1 and 2
    kw = dict(rhs=h['rhs'], keep=h['keep'] if pad else None)
    good = tv.dense_euler_batch_tv(h['B'], h['M'], h['nbr'], tab, tv.DT, nt, **kw)
    if (name, N, nmu, nt) == tv.RED_START_CELL:                                             # (checked beside the zero start)
        kw['U0'] = tv.start_panel(o.S, N, nmu, np.abs(good).max())
        good = tv.dense_euler_batch_tv(h['B'], h['M'], h['nbr'], tab, tv.DT, nt, **kw)
    assert np.abs(good[1:]).max() > 0.0
    for fault in _step_faults(nmu):
        bad = tv.dense_euler_batch_tv(h['B'], h['M'], h['nbr'], tab, tv.DT, nt, fault=fault, **kw)
        miss = float(rb.column_errors(bad, good).max())
        assert miss > FLOOR, (name, N, nmu, nt, fault, miss)


def test_stepping_faults_miss_at_the_reduced_source_cell():
    name, N, nmu, nt, K = tv.RED_SOURCE_CELL
    p, o, red, model, h = _reduced(name, N)
    tab = tv.switch_table(nmu, nt, o.Q, base=pe.cell_thetas(p, nmu))
    rhs_K, phis = tv.source_rhs(h['rhs'], K), tv.switching_phis(nmu, nt, K)
    assert (phis[:, :, 0] > 0).any() and (phis[:, :, 0] < 0).any()
    good = tv.dense_euler_batch_tv(h['B'], h['M'], h['nbr'], tab, tv.DT, nt, rhs_K=rhs_K, phis=phis)
    for fault in _step_faults(nmu):
        bad = tv.dense_euler_batch_tv(h['B'], h['M'], h['nbr'], tab, tv.DT, nt, rhs_K=rhs_K, phis=phis, fault=fault)
        assert float(rb.column_errors(bad, good).max()) > FLOOR, fault


def _fom_cell(name, nmu, nt, K, start, fault=None, **kw):
    from test_fom_euler_batch3d_host import _parts
    p, o, t, Aq, mass, b = _parts(name)
    tab = tv.switch_table(nmu, nt, o.Q, base=np.stack([c3.theta_of(p, mu) for mu in fe.cell_mus(nmu)]))
    b_K, phis = tv.fom_source(np.asarray(b), K, nmu, nt)
    U0 = fe.start_values(Aq, tab[:, 1], b) if start else None
    return tv.BatchFomEulerTv3DRef(Aq, mass, o.S, o.n, tab, tv.DT, nt, phis, b_K, U0=U0, Phi=ref3.default_phi(t), fault=fault, **kw)


@pytest.mark.parametrize('name, nmu, nt, K, start', tv.FOM_CELLS)
def test_stepping_faults_miss_at_the_full_order_cells(name, nmu, nt, K, start):
    good = _fom_cell(name, nmu, nt, K, start)
    for fault in tv.STEP_FAULTS:
        miss = float(good.column_errors(_fom_cell(name, nmu, nt, K, start, fault=fault).trajectories()).max())
        assert miss > FLOOR, (name, fault, miss)


def test_preconditioner_faults_miss_every_iterate_of_both_solvers():
    """nt = 2, the first step capped at k iterations: the k-th iterate with the preconditioner at row 1 alone, and at the mean of
    the rows 0 .. nt, is more than 1e-6 away from the one at the mean of the rows 1 .. nt, for every k the GPU test runs."""
    name, N, nmu = tv.ITERATE_CELL
    p, o, red, model, h = _reduced(name, N)
    tab = tv.switch_table(nmu, 2, o.Q, base=pe.cell_thetas(p, nmu))
    assert tv.reduced_precond(h['B'], h['M'], h['nbr'], tab, tv.DT).has_coarse
    name_f, nmu_f = tv.FOM_ITERATE_CELL
    good_f = _fom_cell(name_f, nmu_f, 2, 1, True)
    for k in tv.K_ITER:
        X, ratios = tv.reduced_first_step_iterates(h['B'], h['M'], h['nbr'], tab, tv.DT, h['rhs'], k)
        assert ratios.min() > 1e-9                                           # no column is done before k
        Xf, _ = good_f.iterate(k)
        for fault in tv.PRECOND_FAULTS:
            Xb, _ = tv.reduced_first_step_iterates(h['B'], h['M'], h['nbr'], tab, tv.DT, h['rhs'], k, fault=fault)
            miss = float((np.linalg.norm(Xb - X, axis=0) / np.linalg.norm(X, axis=0)).max())
            Xfb, _ = _fom_cell(name_f, nmu_f, 2, 1, True, fault=fault).iterate(k)
            miss_f = float((np.linalg.norm(Xfb - Xf, axis=0) / np.linalg.norm(Xf, axis=0)).max())
            print('TV3D host k={} {}: reduced {:.2e}, full order {:.2e}'.format(k, fault, miss, miss_f))
            assert miss > FLOOR and miss_f > FLOOR, (k, fault, miss, miss_f)


TOUCHED = {'column0': 'eta_loc', 'elliptic_row_k1': 'eta_loc', 'residual_row_k': 'tr2', 'coef_row0': 'eta'}


@pytest.mark.parametrize('name, N, nmu, nt', tv.EST_CELLS)
def test_estimate_faults_miss_at_the_estimate_cells(name, N, nmu, nt):
    p, o, red, model, h = _reduced(name, N)
    U = pe.panel(o.S, N, nmu, nt)
    tab, coef = tv.switch_table(nmu, nt, o.Q, base=pe.cell_thetas(p, nmu)), tv.coef_table(nmu, nt)
    good = tv.estimate_outputs_tv(model, tab, coef, tv.DT, U)
    assert good['nc_dU'].min() >= -1e-12 * good['nc_dU'].max() and good['nc_dU'].max() > 0.0       # the clamp hides nothing
    for fault in tv.ESTIMATE_FAULTS:
        if fault == 'column0' and nmu == 1:
            continue
        miss = pe.worst(tv.estimate_outputs_tv(model, tab, coef, tv.DT, U, fault=fault), good, tv.DT)
        assert miss[TOUCHED[fault]] > FLOOR and miss['est'] > FLOOR, (name, N, nmu, nt, fault, miss)


def test_estimate_with_a_switching_source_sees_a_shifted_theta_row():
    """The source terms of U[k] read theta row k too (through the flux image): with K >= 1 the elliptic fault shows in the r row."""
    from test_parabolic_estimate_batch3d_host import _source_model
    p, o, src, red, model, source, N = _source_model()
    nmu, nt = 3, red.nt
    U = pe.panel(o.S, N, nmu, nt)
    phi = np.stack([np.stack([src.coefficients(mu, k * red.dt) for k in range(nt + 1)]) for mu in (0.2, p['mu'], 0.9)])
    tab, coef = tv.switch_table(nmu, nt, o.Q, base=pe.cell_thetas(p, nmu)), tv.coef_table(nmu, nt)
    good = tv.estimate_outputs_tv(model, tab, coef, red.dt, U, phi=phi, source=source)
    const = tv.estimate_outputs_tv(model, tv.constant_table(tab[:, 0], nt), coef[:, :1].repeat(nt + 1, axis=1), red.dt, U, phi=phi,
                                   source=source)
    twin = pe.estimate_outputs(model, tab[:, 0], coef[:, 0], red.dt, U, phi=phi, source=source)
    assert np.abs(const['eta_loc'] - twin['eta_loc']).max() <= 1e-14 * np.abs(twin['eta_loc']).max()
    bad = tv.estimate_outputs_tv(model, tab, coef, red.dt, U, phi=phi, source=source, fault='elliptic_row_k1')
    assert float(np.abs(bad['eta_loc'][1] - good['eta_loc'][1]).max() / np.abs(good['eta_loc'][1]).max()) > FLOOR


# ---------------------------------------------------------------------------------------------------------- declared surface
def test_the_four_symbols_are_declared_and_bound():
    from pylrbms_amd._native3d import SIGNATURES3, Native3DContext
    with open(os.path.join(ROOT, 'include', 'lrbms3d_hip.h')) as fh:
        header = fh.read()
    for name in EXPORTS:
        assert re.search(r'\b{}\s*\('.format(name), header), name
        assert name in SIGNATURES3, name
    twins = {n: n.replace('_tv', '') for n in EXPORTS}
    assert SIGNATURES3[EXPORTS[0]] == SIGNATURES3[twins[EXPORTS[0]]]                       # theta_t in the place of theta
    assert SIGNATURES3[EXPORTS[1]] == SIGNATURES3['lrbms3_reduced_implicit_euler_batch_src']
    assert SIGNATURES3[EXPORTS[2]] == SIGNATURES3[twins[EXPORTS[2]]] and SIGNATURES3[EXPORTS[3]] == SIGNATURES3[twins[EXPORTS[3]]]
    for m in ('fom_implicit_euler_batch_tv', 'reduced_implicit_euler_batch_tv', 'reduced_parabolic_estimate_batch_tv'):
        assert callable(getattr(Native3DContext, m)), m


# ------------------------------------------------------------------------------------------------------------- table plumbing
def test_arity_of_a_diffusion_coefficient_and_the_wording_for_sources():
    from pylrbms_amd.sources3d import coefficient_arity, diffusion_arities
    assert diffusion_arities([lambda mu: 1.0, lambda mu, t: mu + t, lambda mu, t=0.0: mu, lambda mu, q=2: mu ** q]) == [1, 2, 1, 1]
    with pytest.raises(TypeError, match='a diffusion coefficient takes'):
        diffusion_arities([lambda: 1.0])
    with pytest.raises(TypeError, match='a diffusion coefficient takes'):
        diffusion_arities([lambda mu, t, s: 1.0])
    with pytest.raises(TypeError, match='diffusion coefficient'):
        diffusion_arities([1.0])
    with pytest.raises(TypeError, match='signature of the diffusion coefficient'):
        diffusion_arities([dict.update])
    # today's text for sources, word for word
    with pytest.raises(TypeError, match=r'^a source coefficient takes \(mu\) or \(mu, t\); this one takes 0 positional arguments$'):
        coefficient_arity(lambda: 1.0)
    with pytest.raises(TypeError, match=r"^a source coefficient of the 3D path is a number or a callable, not 'str'$"):
        coefficient_arity('mu')
    with pytest.raises(TypeError, match='the signature of the source coefficient'):
        coefficient_arity(dict.update)
    assert list(inspect.signature(coefficient_arity).parameters) == ['c', 'what']


def test_times_are_shared_with_the_source_table():
    from pylrbms_amd import sources3d
    dt, nt = 0.75 / 6, 6
    times = sources3d.table_times(dt, nt)
    assert times.tolist() == [k * dt for k in range(nt + 1)]
    seen = []
    src = {'coefficients': [lambda mu, t: seen.append(t) or mu * t], 'arity': [2]}
    tab = sources3d.evaluate_table(src, 0.5, dt, nt)
    assert seen == times.tolist() and tab[:, 0].tolist() == [0.5 * t for t in times.tolist()]
    d = _fake_d(nt=nt, T=0.75, tv=True)
    seen_theta = []
    d.coefficients[1] = lambda mu, t: seen_theta.append(t) or 1.0 + mu * t
    d.diffusion_coefficients(0.5)
    assert seen_theta == times.tolist()                                                   # phi and theta cannot disagree on t_k


class _Spy:
    """Records every call of a context method by name; the three ``_tv`` wrappers and their twins return zero panels."""

    def __init__(self, S=3, n=20, N=4):
        self.S, self.n, self.N, self.calls = S, n, N, []

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)

        def call(*a, **kw):
            import torch
            self.calls.append((name, a, kw))
            if name.startswith('fom_implicit_euler_batch'):
                th = np.asarray(a[0])
                return torch.zeros(a[2] + 1, self.S, self.n, th.shape[0], dtype=torch.float64), {'iterations': 3, 'relative_residual': 1e-12,
                                                                                                 'panel_iterations': [3]}
            if name.startswith('reduced_implicit_euler_batch'):
                th = np.asarray(a[1])
                return torch.zeros(a[3] + 1, self.S, self.N, th.shape[0], dtype=torch.float64), (3, 1e-13)
            if name.startswith('reduced_parabolic_estimate_batch'):
                nmu, nt = np.asarray(a[1]).shape[0], a[4]
                z = lambda *s: torch.zeros(*s, dtype=torch.float64)      # noqa: E731
                return {'eta_loc': z(3, nt + 1, self.S, nmu), 'time_deriv_nc': z(nt, self.S, nmu), 'time_residual': z(nt, nmu),
                        'eta': z(nt + 1, nmu), 'est': z(nmu)}
            raise AssertionError('unexpected native call ' + name)
        return call

    def names(self):
        return [c[0] for c in self.calls]


def _fake_d(nt=2, T=0.5, tv=True, source=False):
    import torch
    from pylrbms_amd.discretize_parabolic_block_swipdg import ImplicitEulerTimeStepper
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import InstationaryDiscretization3D
    S, n = 3, 20
    d = InstationaryDiscretization3D.__new__(InstationaryDiscretization3D)
    ops = {'A_diag': object(), 'A_cpl': object(), 'b': torch.arange(S * n, dtype=torch.float64).reshape(S, n)}
    d.engine = types.SimpleNamespace(S=S, S_ext=S, t=types.SimpleNamespace(n=n), ops=ops, ctx=_Spy(S, n), hdiam=0.5)
    d.coefficients = [lambda mu: 2.0, (lambda mu, t: float(mu) if t <= 0.25 else 0.1) if tv else (lambda mu: float(mu))]
    d._theta_arity, d._tv = [1, 2 if tv else 1], tv
    d.Q, d.mu_bar, d.mu_hat = 2, 0.5, 0.25
    d.T, d.time_stepper = T, ImplicitEulerTimeStepper(nt=nt, solver_options='operator')
    d.initial_data = torch.zeros(S, n, dtype=torch.float64)
    if source:
        d._src = {'coefficients': [2.0, lambda mu, t: mu * t], 'arity': [0, 2], 'K': 2, 'b_K': torch.ones(2, S, n, dtype=torch.float64),
                  'F2': object(), 'bdiv_K': object()}
    return d


def _fake_rd(d, N=4, source=False):
    import torch
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import InstationaryReducedDiscretization3D
    rd = InstationaryReducedDiscretization3D.__new__(InstationaryReducedDiscretization3D)
    S = d.engine.S
    rd.d, rd.N, rd.T, rd.time_stepper = d, N, d.T, d.time_stepper
    rd.out = {'B_sys': torch.zeros(d.Q, S, 7, N, N, dtype=torch.float64), 'rhs_red': torch.zeros(S, N, dtype=torch.float64)}
    rd.M_red = torch.zeros(S, N, N, dtype=torch.float64)
    rd.rhs_red_K = torch.zeros(2, S, N, dtype=torch.float64) if source else None
    rd.r_fd_K = object() if source else None
    rd._zero = (rd.out, d.engine.ops)
    d.engine.ctx.N = N
    return rd


def test_tables_rows_and_references_at_t_zero():
    d = _fake_d(nt=2, T=0.5)                       # dt = 0.25: rows at t = 0, 0.25, 0.5; the switch closes after t* = 0.25
    tab = d.diffusion_coefficients(0.8)
    assert tab.tolist() == [[2.0, 0.8], [2.0, 0.8], [2.0, 0.1]]
    with pytest.raises(NotImplementedError, match='no single row'):
        d.theta(0.8)
    # alpha of row k: c_0(mu, t_k) / c_0(mu_bar, 0); gamma likewise: mu_bar sits at t = 0 (0.5, never 0.1)
    assert d.alpha(0.8, d.mu_bar, 0.5) == 1.0 and d.gamma(0.8, d.mu_bar, 0.25) == 0.8 / 0.5 and d.gamma(0.8, d.mu_bar, 0.5) == 1.0
    assert d.gamma(0.05, d.mu_bar, 0.5) == 1.0 and d.gamma(0.05, d.mu_hat, 0.5) == 1.0
    coef = d._estimator_coefficients(0.8)
    assert coef.shape == (3, 2) and coef[0].tolist() == coef[1].tolist()
    assert coef[1, 0] == np.sqrt(0.8 / 0.5) and coef[2, 0] == 1.0 and coef[2, 1] == 1.0
    assert list(d._theta_at(d.mu_bar, 0.0)) == [2.0, 0.5]                                 # what the engine gets as theta_bar
    plain = _fake_d(tv=False)
    assert plain.diffusion_coefficients(0.8).tolist() == [[2.0, 0.8]] * 3 and plain.theta(0.8).tolist() == [2.0, 0.8]


def test_a_nonpositive_entry_is_a_value_error_naming_q_and_k():
    d = _fake_d(nt=2, T=0.5)
    d.coefficients[1] = lambda mu, t: mu if t < 0.5 else 0.0
    with pytest.raises(ValueError, match=r'q = 1 .* k = 2'):
        d.diffusion_coefficients(0.8)
    d.coefficients[1] = lambda mu, t: float('nan')
    with pytest.raises(ValueError, match=r'q = 1 .* k = 0'):
        d.solve_batch([0.8])
    assert d.engine.ctx.calls == []


def test_elliptic_discretize_refuses_a_time_dependent_coefficient_before_an_engine_is_built(monkeypatch):
    import pylrbms_amd.discretize_elliptic_block_swipdg_3d as mod
    import pylrbms_amd.discretize_parabolic_block_swipdg_3d as par

    def no_engine(*a, **k):
        raise AssertionError('an engine was built')
    monkeypatch.setattr(mod, 'Engine3D', no_engine)
    p = c3.make_problem('aniso_2x2x1')
    pd = {'grid': p['grid'], 'lambda': {'functions': p['lambdas'], 'coefficients': p['thetas']}, 'lambda_bar': p['lambda_bar'],
          'lambda_hat': p['lambda_hat'], 'f': p['f'], 'mu_bar': p['mu_bar'], 'mu_hat': p['mu_hat']}
    pd['lambda'] = dict(pd['lambda'], coefficients=[lambda mu: 1.0, lambda mu, t: mu * (1.0 + t)])
    with pytest.raises(NotImplementedError, match='parabolic discretize'):
        mod.discretize(pd)
    with pytest.raises(TypeError, match='diffusion coefficient'):
        mod.discretize(dict(pd, **{'lambda': dict(pd['lambda'], coefficients=[lambda mu: 1.0, lambda: 2.0])}))

    class Reached(Exception):
        pass

    def engine(grid, lam, f, lbar, lhat, data_degree=2, device_index=0, theta_bar=None):
        assert list(theta_bar) == [1.0, p['mu_bar']]                                      # theta_bar at t = 0
        raise Reached()
    monkeypatch.setattr(mod, 'Engine3D', engine)
    with pytest.raises(Reached):
        par.discretize(pd, 0.5, 2)


def test_every_refusal_comes_before_the_engine_is_touched():
    d = _fake_d()
    for call in (lambda: d.theta(0.5), lambda: d.solve_stationary(0.5), lambda: d.solve_stationary_batch([0.5])):
        with pytest.raises(NotImplementedError, match='depend on time'):
            call()
    import torch
    for N, Q, calls in ((33, 2, ('solve', 'solve_batch', 'estimate', 'estimate_batch')), (32, 3, ('estimate', 'estimate_batch'))):
        d = _fake_d()
        d.Q = Q
        if Q == 3:
            d.coefficients.append(lambda mu: 1.0)
            d._theta_arity.append(1)
        rd = _fake_rd(d, N=N)
        u = torch.zeros(3, 3, N, dtype=torch.float64)
        for name in calls:
            fn = {'solve': lambda: rd.solve(0.5), 'solve_batch': lambda: rd.solve_batch([0.5]),
                  'estimate': lambda: rd.estimate(u, 0.5), 'estimate_batch': lambda: rd.estimate_batch(u[None], [0.5], native=False)}[name]
            with pytest.raises(NotImplementedError, match='N = 33 > 32' if N == 33 else 'Q N = 96 > 64'):
                fn()
        assert d.engine.ctx.calls == []
    rd = _fake_rd(_fake_d())
    with pytest.raises(ValueError, match='whole trajectory'):
        rd.estimate_batch(torch.zeros(1, 2, 3, 4, dtype=torch.float64), [0.5], native=True)
    assert rd.d.engine.ctx.calls == []


@pytest.mark.parametrize('source', (False, True))
def test_every_call_of_a_time_dependent_discretization_runs_a_tv_export(source):
    import torch
    d = _fake_d(source=source)
    spy, nt = d.engine.ctx, 2
    U = d.solve(0.8)
    assert tuple(U.shape) == (3, 20, nt + 1) and d.last_solve_info == (3, 1e-12)
    trajs = d.solve_batch([0.3, 0.8, 0.9])
    assert len(trajs) == 3 and spy.names() == ['fom_implicit_euler_batch_tv'] * 2
    th1, th3 = np.asarray(spy.calls[0][1][0]), np.asarray(spy.calls[1][1][0])
    assert th1.shape == (1, nt + 1, 2) and th3.shape == (3, nt + 1, 2)
    assert th3[1].tolist() == [[2.0, 0.8], [2.0, 0.8], [2.0, 0.1]] and np.array_equal(th1[0], th3[1])
    phi = np.asarray(spy.calls[1][1][6])
    assert phi.shape == (3, nt + 1, 2 if source else 1)
    if source:
        assert phi[1].tolist() == [[2.0, 0.0], [2.0, 0.8 * 0.25], [2.0, 0.8 * 0.5]]
    rd = _fake_rd(d, source=source)
    spy.calls.clear()
    u = rd.solve(0.8)
    us = rd.solve_batch([0.3, 0.8])
    assert tuple(u.shape) == (nt + 1, 3, 4) and tuple(us.shape) == (2, nt + 1, 3, 4)
    assert spy.names() == ['reduced_implicit_euler_batch_tv'] * 2
    assert np.asarray(spy.calls[1][1][1]).shape == (2, nt + 1, 2) and ('phi' in spy.calls[1][2]) == source
    spy.calls.clear()
    for native in (False, True):
        est, parts = rd.estimate(u, 0.8)
        res = rd.estimate_batch(us, [0.3, 0.8], native=native)
        assert len(res) == 2 and len(parts) == 5
    assert spy.names() == ['reduced_parabolic_estimate_batch_tv'] * 4
    a = spy.calls[1][1]
    assert np.asarray(a[1]).shape == (2, nt + 1, 2) and np.asarray(a[2]).shape == (2, nt + 1, 2)
    assert np.array_equal(np.asarray(a[2])[1], d._estimator_coefficients(0.8)) and a[3] == 0.25 and a[4] == nt
    assert ('phi' in spy.calls[1][2]) == source
    assert isinstance(est, float) and torch.is_tensor(u)


def test_a_time_independent_discretization_calls_no_tv_export():
    d = _fake_d(tv=False)
    spy = d.engine.ctx
    d.solve_batch([0.3, 0.8])
    rd = _fake_rd(d)
    us = rd.solve_batch([0.3, 0.8])
    rd.estimate_batch(us, [0.3, 0.8], native=True)
    assert spy.names() == ['fom_implicit_euler_batch', 'reduced_implicit_euler_batch', 'reduced_parabolic_estimate_batch']
    assert np.asarray(spy.calls[0][1][0]).shape == (2, 2) and np.asarray(spy.calls[2][1][2]).shape == (2, 2)


def test_switch_off_after_in_the_problem_file(monkeypatch):
    from pylrbms_amd import multiscale_problem3d as mp
    from pylrbms_amd.sources3d import diffusion_arities
    monkeypatch.setattr(mp, 'make_grid3d', lambda **kw: 'grid')
    cfg = {'num_subdomains': [2, 2, 2], 'cubes_per_subdomain': 1}
    plain, sw = mp.init_grid_and_problem(cfg), mp.init_grid_and_problem(cfg, switch_off_after=0.3)
    assert inspect.signature(mp.init_grid_and_problem).parameters['switch_off_after'].default is None
    assert diffusion_arities(plain['lambda']['coefficients']) == [1, 1] and diffusion_arities(sw['lambda']['coefficients']) == [1, 2]
    c = sw['lambda']['coefficients'][1]
    assert c(0.7, 0.0) == 0.7 and c(0.7, 0.3) == 0.7 and c(0.7, 0.3000001) == 0.1 and sw['parameter_range'][0] == 0.1
    assert sorted(plain) == sorted(sw) and sw['mu_bar'] == plain['mu_bar'] == 1.0
    x = np.array([[0.1, 0.2, 0.3], [0.6, 0.3, 0.8]])
    for k in ('lambda_bar', 'lambda_hat'):
        assert np.array_equal(sw[k](x), plain[k](x))                                      # mu_bar / mu_hat sit at t = 0
    assert plain['lambda']['coefficients'][1](0.7) == 0.7
