"""The 2D offline assembly (csrc/assemble.hip) against the CPU oracle across quadrature rule sets (tests/quadrature_cases.py): the
rule set is a caller-visible parameter (``Engine(..., quadrature=)``, ``discretize(..., quadrature=)``) that decides every loop
length and sample-record offset of the assembly kernels.  The data oscillate inside every element, so a wrong offset, point order
or rule length shows far above the tolerance (tests/test_quadrature_cases_host.py asserts that on the oracle).

Tolerances are those of tests/test_parity_gpu.py: 1e-11 relative (max norm) for assembled / projected arrays, 1e-10 for the reduced
solve; the corrector, affine-source and API checks use the bounds of their own test files."""
import ctypes
import functools

import numpy as np
import pytest

import quadrature_cases as qc
from common import compare_all, energy_orthonormalize, make_bases, theta_bar_of, theta_of

pytestmark = pytest.mark.gpu

TOL = qc.TOL
CORR_TOL = 1e-8                # tests/test_enrichment_gpu.py
LRBMS_E_INVALID = -1           # include/lrbms_hip.h


def _engine(p, spec, **kw):
    from pylrbms_amd.engine import Engine
    lam = p['lambda']
    return Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar_of(p), quadrature=spec,
                  **kw)


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, oracle, assembled engine) at the rule set ``name``, once per module."""
    p, d = qc.oracle_2d(name)
    return p, d, _engine(p, qc.spec_2d(name)).assemble()


def _host(x):
    return x.detach().cpu().numpy()


def _flux_rows_error(p, d, eng):
    got, dropped = qc.flux_rows_dense(p, _host(eng.F), d.mesh)
    want = qc.oracle_flux_rows(d)
    assert dropped == 0.0                                       # nothing behind a physical side
    return qc.rel(got, want)


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize('name', list(qc.RULE_SETS_2D))
def test_every_array_matches_the_oracle_per_rule_set(name):
    p, d, eng = case(name)
    assert eng.quadrature.as_dict() == d.quad.as_dict()
    V = energy_orthonormalize(make_bases(d.S, d.n, qc.N_2D, seed=5), d)
    res = compare_all(p, eng, V, qc.MU_2D, oracle=d)
    assert res.pop('cg_iterations') > 0
    res['F'] = _flux_rows_error(p, d, eng)
    worst = max(res, key=lambda k: res[k] / (1e-10 if k == 'u_solve' else TOL))
    print('rule set', name, 'worst', worst, res[worst], 'F', res['F'], 'u_solve', res['u_solve'])
    bad = {k: v for k, v in res.items() if not (v < (1e-10 if k == 'u_solve' else TOL))}
    assert not bad, bad


# ------------------------------------------------------------------------------- Dirichlet correction and affine sources
@pytest.mark.parametrize('name', qc.DCORR_AND_SOURCE_SETS_2D)
def test_dirichlet_correction_matches_the_oracle_neighbourhood_system(name):
    """``lrbms_assemble_dirichlet_correction`` reads the coupling-face samples at o_sysf with stride nfs: the neighbourhood operator
    built from the assembled A_diag, A_cpl and D_corr (tests/pcg_ref.py) against the oracle's ``local_correction_system(...,
    rules='system')`` at the parity tolerance, and the corrector solves against its sparse LU at the bound of
    tests/test_enrichment_gpu.py."""
    import pcg_ref
    p, d, eng = case(name)
    t, nbr = p['grid'].template, np.asarray(p['grid'].neighbor_slots)
    D = eng.ctx.assemble_dirichlet_correction(eng.lam)
    arrays = [_host(x) for x in (eng.A_diag, eng.A_cpl, D)]
    assert np.abs(arrays[2]).max() > 1e-3 * np.abs(arrays[0]).max()
    d_mu = qc.MU_2D
    theta = theta_of(p, d_mu)
    worst = 0.0
    for ii in range(d.S):
        A, dofs = pcg_ref.hood_operator_2d(*arrays, theta, t, nbr, ii)
        want, _, hood, want_dofs = d.local_correction_system(ii, d_mu, rules='system')
        assert np.array_equal(dofs, want_dofs)
        worst = max(worst, float(abs(A - want).max() / abs(want).max()))
    print('rule set', name, 'neighbourhood operator', worst)
    assert worst < TOL
    corr, info = eng.local_corrections(theta, list(range(d.S)))
    corr = _host(corr)
    for ii in range(d.S):
        ref = d.solve_for_local_correction(ii, d_mu)
        err = float(np.abs(corr[ii] - ref).max() / np.abs(ref).max())
        print('rule set', name, 'corrector', ii, err)
        assert err < CORR_TOL, (ii, err)


@pytest.mark.parametrize('name', qc.DCORR_AND_SOURCE_SETS_2D)
def test_source_gram_and_load_vectors_match_the_affine_source_reference(name):
    """``lrbms_assemble_source_gram`` (rule f2 at o_ff2) and the per-component load vectors (rule rhs at o_frhs) of two source
    components against tests/affine_source_ref.py at the rule set, at the bound of tests/test_affine_source_gpu.py."""
    import torch
    from affine_source_ref import AffineSource
    from pylrbms_amd.functions import make_expression_function_1x1
    from pylrbms_amd.parameters import ExpressionParameterFunctional
    from pylrbms_amd.sources import setup_sources
    p, d, eng = case(name)
    second = make_expression_function_1x1(p['grid'], 'x', qc.F_SECOND_2D, name='f_second')
    switch = ExpressionParameterFunctional('(diffusion > 0.5) * (2 * diffusion - 1)', p['parameter_type'])
    pa = dict(p, f={'functions': [p['f'], second], 'coefficients': [1, switch]})
    ref = AffineSource(pa, quad=qc.oracle_spec_2d(name))
    src = setup_sources(eng, ref.funcs, pa['f']['coefficients'])
    e_b = qc.rel(_host(src['b_K']), ref.b_K.reshape(2, eng.S, eng.t.n))
    o = ref.d
    w = o._tri(o.quad.f2)['w']
    fv = np.stack([o._vol(fn, o.quad.f2) for fn in ref.funcs]).reshape(2, o.S, o.nT, -1)
    F2_ref = np.einsum('k,se,jsek,lsek->sjl', w, o.mesh.area.reshape(o.S, o.nT), fv, fv)
    e_g = qc.rel(_host(src['F2']), F2_ref)
    print('rule set', name, 'b_K', e_b, 'F2', e_g)
    assert e_b < 1e-12 and e_g < 1e-12
    for j in range(2):                                          # the diagonal is the oracle's own ||f_j||^2
        assert qc.rel(_host(src['F2'])[:, j, j], ref.frozen(np.eye(2)[j]).local_eta_rf_squared) < 1e-12
    assert torch.equal(src['F2'], src['F2'].transpose(1, 2))
    # one component: the engine's own f2 and b, bit for bit
    assert torch.equal(eng.ctx.assemble_source_gram(eng.f_smp[None].contiguous()).reshape(-1), eng.f2)
    assert torch.equal(src['b_K'][0], eng.b)


# ---------------------------------------------------------------------------------------------------------- padded records
def _assemble_all(eng, rec):
    """Every assembly export on the sample records ``rec`` (dict of device tensors) -> dict of outputs."""
    c = eng.ctx
    out = {}
    out['A_diag'], out['A_cpl'] = c.assemble_swipdg(rec['lam'])
    out['b'], out['f2'], out['ceps'] = c.assemble_rhs(rec['f_smp'], rec['lhat'])
    out['P_diag'], out['ebar'], out['caa'], out['Aab'], out['Bbb'] = c.assemble_products(eng.theta_bar, rec['lam'], rec['lam_df'],
                                                                                       rec['lbar'], rec['lhat'])
    out['F'] = c.assemble_flux(rec['lam'])
    out['F2'] = c.assemble_source_gram(rec['f_smp'][None].contiguous())
    out['D_corr'] = c.assemble_dirichlet_correction(rec['lam'])
    return out


def _records(eng):
    return {k: getattr(eng, k) for k in qc.RECORDS_2D}


@pytest.mark.parametrize('name', qc.PADDED_SETS_2D)
def test_sample_records_with_gaps_give_the_same_bits(name):
    """``lrbms_set_quadrature`` admits layouts with gaps (every offset and stride is validated with >=): the same rules with every
    offset moved up and every stride enlarged, NaN in every gap, give every assembled array bit for bit."""
    import torch
    p, d, eng = case(name)
    c = eng.ctx
    packed = c.quad
    base = _assemble_all(eng, _records(eng))
    gaps = qc.padded_quadrature(packed)
    rec = {k: c.from_numpy(qc.relayout_record(_host(v), packed, gaps, k)) for k, v in _records(eng).items()}
    assert all(bool(torch.isnan(v).any()) for v in rec.values())
    try:
        c._check(c.lib.lrbms_set_quadrature(c.handle, ctypes.byref(gaps)), 'lrbms_set_quadrature')
        c.quad = gaps
        out = _assemble_all(eng, rec)
        torch.cuda.synchronize()
    finally:
        c.set_quadrature(eng.quadrature)
    for k in base:
        assert torch.equal(base[k], out[k]), (name, k)
    again = _assemble_all(eng, _records(eng))                   # and the packed layout is back
    for k in base:
        assert torch.equal(base[k], again[k]), (name, k)


# --------------------------------------------------------------------------------------------------------------- refusals
def _bad_quadratures(q):
    """(label, quadrature, expected message) of every refusal of lrbms_set_quadrature."""
    def mutate(fn):
        g = qc.clone_quadrature(q)
        fn(g)
        return g

    def asym(g):
        g.energy_face.t[0] += 1e-12

    return [('tri n = 0', mutate(lambda g: setattr(g.rhs, 'n', 0)), 'triangle rule size out of range'),
            ('tri n = 17', mutate(lambda g: setattr(g.df_ab, 'n', 17)), 'triangle rule size out of range'),
            ('edge n = 5', mutate(lambda g: setattr(g.flux_face, 'n', 5)), 'edge rule size out of range'),
            ('edge asymmetric', mutate(asym), 'edge rules must be symmetric'),
            ('o_sysf one short', mutate(lambda g: setattr(g, 'o_sysf', g.o_sysf - 1)), 'inconsistent sample record layout'),
            ('nfs one short', mutate(lambda g: setattr(g, 'nfs', g.nfs - 1)), 'inconsistent sample record layout')]


def test_set_quadrature_refusals_leave_the_context_intact():
    import torch
    p, d, eng = case(qc.CONTROL_2D)
    c = eng.ctx
    base = _assemble_all(eng, _records(eng))
    assert qc.rel(_host(base['A_diag']), _host(eng.A_diag)) == 0.0
    for label, bad, message in _bad_quadratures(c.quad):
        rc = c.lib.lrbms_set_quadrature(c.handle, ctypes.byref(bad))
        assert rc == LRBMS_E_INVALID, (label, rc)
        assert message in c.lib.lrbms_last_error(c.handle).decode(), (label, c.lib.lrbms_last_error(c.handle))
        out = _assemble_all(eng, _records(eng))
        for k in base:
            assert torch.equal(base[k], out[k]), (label, k)
    assert c.lib.lrbms_set_quadrature(c.handle, None) == LRBMS_E_INVALID


# ------------------------------------------------------------------------------------------------------------- end to end
def test_discretize_solve_estimate_at_the_uniform_rule():
    """``discretize(p, quadrature=QuadratureSpec.uniform(5))``: the full-order solve and estimate against the oracle at that spec, at
    the bounds of tests/test_api_gpu.py."""
    from pylrbms_amd.discretize_elliptic_block_swipdg import discretize
    from pylrbms_amd.quadrature import QuadratureSpec
    p, o = qc.oracle_2d('uniform5')
    d, _ = discretize(p, quadrature=QuadratureSpec.uniform(5))
    assert d.engine.quadrature.as_dict() == o.quad.as_dict()
    mu = d.parse_parameter(qc.MU_2D)
    U = d.solve(mu)
    U_ref = o.solve(qc.MU_2D)
    e_u = float(np.abs(U.data.reshape(o.S, o.n) - U_ref).max() / np.abs(U_ref).max())
    eta, (nc, r, df), ind = d.estimate(U, mu=mu, decompose=True)
    eta_o, (nc_o, r_o, df_o), ind_o = o.estimate(U.data.reshape(o.S, o.n), qc.MU_2D, decompose=True)
    errs = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in ((nc[:, 0], nc_o), (r[:, 0], r_o), (df[:, 0], df_o), (ind[:, 0], ind_o))]
    print('uniform(5) end to end: u', e_u, 'eta', abs(eta - eta_o) / eta_o, 'terms', errs)
    assert e_u < 1e-8
    assert abs(eta - eta_o) < 1e-9 * eta_o
    assert max(errs) < 1e-9


# ------------------------------------------------------------------------------------------------------- one-point df_bb
@functools.lru_cache(maxsize=None)
def _one_point_case():
    from common import oracle_from_problem
    from oracle.quadrature import QuadratureSpec as OracleSpec
    from pylrbms_amd.quadrature import QuadratureSpec
    p = qc.problem_2d()
    d = oracle_from_problem(p, quad=OracleSpec.uniform(1))
    return p, d, _engine(p, QuadratureSpec.uniform(1)).assemble()


def test_one_point_df_bb_blocks_match_the_oracle_and_are_singular():
    """``QuadratureSpec.uniform(1)`` (and ``uniform(0)``): the element blocks Bbb of a one-point df_bb rule against the oracle -- and
    singular in both (rank <= 2: three RT0 functions at one point of the plane), unlike those of the three-point rule."""
    p, d, eng = _one_point_case()
    got = _host(eng.Bbb).reshape(-1, 3, 3)
    err = qc.rel(got, np.asarray(d.bb_blocks))
    print('uniform(1) Bbb', err)
    assert err < TOL
    lo = np.linalg.eigvalsh(0.5 * (got + got.transpose(0, 2, 1)))[:, 0]
    scale = np.abs(got).max()
    assert np.abs(lo).max() < 1e-12 * scale
    _, _, ctl = case(qc.CONTROL_2D)
    assert np.linalg.eigvalsh(_host(ctl.Bbb).reshape(-1, 3, 3))[:, 0].min() > 1e-4 * scale


def test_one_point_df_bb_default_engine_matches_the_oracle():
    """The default path of ``Engine`` on ``uniform(1)``: it selects f2_form 1 (the flux Grams as R^T B R, no Cholesky of the
    singular Bbb), so the fused pass returns finite G_bb / G_rdd that match the oracle like every other array; the forms that
    factor Bbb are refused for such a rule set."""
    from pylrbms_amd.quadrature import QuadratureSpec
    p, d, eng = _one_point_case()
    assert eng.ctx.fused_supported(eng.Q, qc.N_2D, factored=True) and eng.ctx.fused_supported(eng.Q, qc.N_2D)
    V = energy_orthonormalize(make_bases(d.S, d.n, qc.N_2D, seed=5), d)
    res = compare_all(p, eng, V, qc.MU_2D, oracle=d)
    assert res.pop('cg_iterations') > 0
    for k in ('fused_G_bb', 'fused_G_rdd', 'fused_dense_G_bb', 'fused_dense_G_rdd', 'G_bb', 'G_rdd', 'eta_factored'):
        assert np.isfinite(res[k]), k
    worst = max(res, key=lambda k: res[k] / (1e-10 if k == 'u_solve' else TOL))
    print('uniform(1) default engine: worst', worst, res[worst], 'fused_G_bb', res['fused_G_bb'], 'fused_G_rdd', res['fused_G_rdd'])
    bad = {k: v for k, v in res.items() if not (v < (1e-10 if k == 'u_solve' else TOL))}
    assert not bad, bad
    for form in (0, 2):
        with pytest.raises(ValueError, match='one-point df_bb'):
            _engine(p, QuadratureSpec.uniform(0), conventions={'f2_form': form})
    _engine(p, QuadratureSpec.uniform(1), conventions={'f2_form': 1})
