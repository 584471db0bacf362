"""The 3D / P2 offline assembly (k3_asm, k3_scalars, k3_assemble_flux, k3_source_gram and the Dirichlet-correction kernel of
csrc/lrbms3d.hip, sources3d.hip, enrich3d.hip) against the CPU oracle across the quadrature degree ``Engine3D(..., data_degree=)``: the degree decides the
reduction length of every k3_asm operator (single partial chunks of ASM_KC points up to 23 chunks with a tail,
tests/test_quadrature_cases_host.py) and every offset of the sample records.  Data: tests/quadrature_cases.py (Q = 3 components
that oscillate inside every element; the host tests assert that they tell the degrees apart).

Tolerances are those of tests/test_parity3d_gpu.py: 1e-11 relative (max norm) for assembled / projected arrays, 1e-10 for the
estimator terms and the reduced solve; the source-Gram and corrector checks use the bounds of their own test files."""
import functools

import numpy as np
import pytest

import common3d as c3
import quadrature_cases as qc

pytestmark = pytest.mark.gpu

TOL = qc.TOL


@functools.lru_cache(maxsize=None)
def case(grid, degree):
    """(problem, oracle, its assembled arrays, assembled engine with the corrector data), once per module."""
    p, d, ref = qc.oracle_3d(grid, degree)
    eng = c3.engine_of(p)
    assert eng.spec.data_degree == degree == d.deg
    return p, d, ref, eng.assemble(online_enrichment=True)


def _assembled_errors(ref, ops):
    return {k: c3.rel(ops[k].cpu().numpy().reshape(ref[k].shape), ref[k]) for k in qc.ARRAYS_3D}


def _check_assembled_and_pass(grid, degree):
    from pylrbms_amd.engine3d import expand_factored
    p, d, ref, eng = case(grid, degree)
    errs = _assembled_errors(ref, eng.ops)
    worst = max(errs, key=errs.get)
    print('grid', grid, 'degree', degree, 'assembled worst', worst, errs[worst])
    assert all(v < TOL for v in errs.values()), errs
    # ---- one pass on the assembled operators: projected arrays, estimator terms, reduced solve
    N = p['N']
    V = c3.make_bases3d(d.S, d.n, N, seed=3)
    out = eng.project_and_estimate(eng.ctx.from_numpy(V))
    rd = c3.reduce_with_oracle(p, d, V)
    got = {k: v.cpu().numpy() for k, v in expand_factored(eng, out, d.Q, N).items()}
    worst = {}
    for ii in range(d.S):
        want = c3.oracle_dense_blocks(p, d, rd, ii)
        for k in ('G_nc', 'G_bb', 'G_rdd', 'r_fd'):
            worst[k] = max(worst.get(k, 0.0), c3.rel(got[k][ii], want[k]))
        worst['G_ab'] = max(worst.get('G_ab', 0.0), c3.rel(got['G_ab'][:, ii], want['G_ab']))
        worst['G_aa'] = max(worst.get('G_aa', 0.0), c3.rel(got['G_aa'][:, :, ii], want['G_aa']))
        worst['B_sys'] = max(worst.get('B_sys', 0.0), c3.rel(got['B_sys'][:, ii], want['B_sys']))
        worst['rhs_red'] = max(worst.get('rhs_red', 0.0), c3.rel(got['rhs_red'][ii], rd.rhs[ii]))
    k = max(worst, key=worst.get)
    print('grid', grid, 'degree', degree, 'projected worst', k, worst[k])
    assert all(v < TOL for v in worst.values()), worst
    u = np.random.default_rng(5).standard_normal((d.S, N))
    th = c3.theta_of(p, p['mu'])
    eta = eng.reduced_estimate(th, eng.ctx.from_numpy(u), out).cpu().numpy()
    e_eta = [c3.rel(a, b) for a, b in zip(eta, rd.local_terms([u[ii] for ii in range(d.S)], p['mu']))]
    us, (it, res) = eng.reduced_solve(th, out, rtol=1e-13)
    e_u = c3.rel(us.cpu().numpy(), np.stack(rd.solve(p['mu'])))
    print('grid', grid, 'degree', degree, 'eta', e_eta, 'u', e_u)
    assert max(e_eta) < 1e-10 and res <= 1e-13 and it > 0 and e_u < 1e-10
    return p, d, eng


@pytest.mark.parametrize('degree', (qc.CONTROL_3D,) + qc.DEGREES_3D)
def test_assembly_and_pass_match_the_oracle_per_degree(degree):
    _check_assembled_and_pass('first', degree)


@pytest.mark.parametrize('degree', qc.DEGREES_SECOND_GRID_3D)
def test_assembly_and_pass_with_padded_side_tables(degree):
    """k_c = (2, 1, 1): the sides have 2, 4 and 4 faces, the side tables hold ncf = 4 -- rows of padded positions stay exactly zero."""
    p, d, eng = _check_assembled_and_pass('second', degree)
    t = p['grid'].template
    assert int(t.side_count.min()) < t.ncf
    pad = np.arange(t.ncf)[None, :] >= np.asarray(t.side_count)[:, None]                          # [6, ncf]
    for k in ('A_cpl', 'D_corr'):
        x = eng.ops[k].cpu().numpy().reshape(d.Q, d.S, 6, t.ncf, 100)
        assert np.abs(x).max() > 0.0 and not np.any(x[:, :, pad] != 0.0), k


# ------------------------------------------------------------------------------------------------- other assembly exports
@pytest.mark.parametrize('degree', qc.DEGREES_EXPORTS_3D)
def test_source_gram_matches_the_affine_source_reference(degree):
    """``lrbms3_assemble_source_gram`` (K = 2) and the per-component b / bdiv against tests/affine_source3d_ref.py at the degree, at
    the bounds of tests/test_affine_source3d_gpu.py."""
    import torch
    from affine_source3d_ref import AffineSource3D
    from pylrbms_amd.sources3d import setup_sources3d
    p, d, _, eng = case('first', degree)
    funcs = [p['f'], qc.f_second_3d]
    src = AffineSource3D(p, funcs=funcs, coeffs=[1, 1])
    assert src.d.deg == degree
    s = setup_sources3d(eng, funcs, [1, 1], [0, 0])
    e_g = c3.rel(s['F2'].cpu().numpy(), src.gram())
    comps = [src.component(j) for j in range(2)]
    e_b = max(c3.rel(s['b_K'][j].cpu().numpy().ravel(), comps[j].b) for j in range(2))
    e_d = max(c3.rel(s['bdiv_K'][j].cpu().numpy().ravel(), comps[j].bdiv) for j in range(2))
    print('degree', degree, 'F2', e_g, 'b_K', e_b, 'bdiv_K', e_d)
    assert e_g < 1e-12 and e_b < 1e-12 and e_d < 1e-12
    assert torch.equal(s['F2'], s['F2'].transpose(1, 2))
    assert torch.equal(eng.ctx.assemble_source_gram(eng.f_smp[None].contiguous()).reshape(-1), eng.ops['f2'])


@pytest.mark.parametrize('degree', qc.DEGREES_EXPORTS_3D)
def test_dirichlet_correction_matches_the_reference(degree):
    """``lrbms3_assemble_dirichlet_correction`` against tests/enrichment3d_ref.py at the degree, at the bound of
    tests/test_enrichment3d_gpu.py; physical sides exactly zero."""
    import enrichment3d_ref as ref
    p, d, _, eng = case('first', degree)
    got = eng.ops['D_corr'].cpu().numpy()
    want = ref.dcorr_layout(p, d).reshape(got.shape)
    assert np.abs(want).max() > 0.0
    print('degree', degree, 'D_corr', c3.rel(got, want))
    assert c3.rel(got, want) < 1e-11
    empty = ~np.any(want.reshape(-1, 100) != 0.0, axis=1)
    assert empty.any() and not np.any(got.reshape(-1, 100)[empty] != 0.0)


# ---------------------------------------------------------------------------------------------------------- padded records
def test_sample_records_with_gaps_give_the_same_bits():
    """``lrbms3_mesh_upload`` takes o_fs, o_ff, o_c and the three strides from the descriptor: the layout of degree 1 with every
    offset and stride enlarged, NaN in the gaps and tails, the tables unchanged -- every assembled array bit for bit."""
    import torch
    from pylrbms_amd._native3d import Native3DContext
    degree = qc.DEGREE_PADDED_3D
    p, d, _, eng = case('first', degree)
    grid, t = p['grid'], p['grid'].template
    gaps = qc.PaddedSpec3D(degree)
    ctx = Native3DContext(0)
    ctx.mesh_upload(t, gaps, t.tables(eng.spec), eng.nbr, grid.phys_mask[eng.ext], eng.S, eng.S_ext)
    lam = ctx.from_numpy(gaps.relayout_lam(eng.lam.cpu().numpy()))
    lhat = ctx.from_numpy(gaps.relayout_tail(eng.lhat.cpu().numpy(), gaps.hat_stride))
    f_smp = ctx.from_numpy(gaps.relayout_tail(eng.f_smp.cpu().numpy(), gaps.f_stride))
    assert all(bool(torch.isnan(x).any()) for x in (lam, lhat, f_smp))
    out = {}
    out['A_diag'], out['A_cpl'] = ctx.assemble_system(lam)
    out['b'], out['f2'], out['ceps'], out['bdiv'] = ctx.assemble_rhs(f_smp, lhat)
    out['ebar'], out['Aaa'], out['Aab'], out['Bbb'] = ctx.assemble_products(lam, eng.lbar, lhat)
    out['Cf'] = ctx.assemble_flux(lam)
    out['P_diag'] = ctx.assemble_energy_product(eng.theta_bar, lam)
    out['D_corr'] = ctx.assemble_dirichlet_correction(lam)
    F2 = ctx.assemble_source_gram(f_smp[None].contiguous())
    torch.cuda.synchronize()
    assert set(out) == set(eng.ops)
    for k in out:
        assert torch.equal(out[k], eng.ops[k]), k
    assert torch.equal(F2.reshape(-1), eng.ops['f2'])
