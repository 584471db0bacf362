"""The affine-source exports of the 3D path under poisoned work and inside guard bands, in the style of
tests/test_work_poison_gpu.py (whose ``Guard`` / ``poisoned`` are used): every tensor the wrapper allocates for a call -- the work
area and the outputs -- lies between sentinel bands and is zero-filled in one run, NaN-filled in the other.  Results and ``info``
must be identical, the bands intact; the zero-filled result is also checked against a plain reference."""
import numpy as np
import pytest

import common3d as c3
from affine_source3d_ref import problem_dict
from test_work_poison_gpu import _rel, poisoned

pytestmark = pytest.mark.gpu

_CACHE = {}


def _setup():
    if not _CACHE:
        from pylrbms_amd.discretize_parabolic_block_swipdg_3d import discretize
        p = c3.make_problem('aniso_2x2x1')
        d, _ = discretize(problem_dict(p, coeffs=[1, 0.5]), 0.3, 3)
        eng = d.engine
        Vt = eng.ctx.from_numpy(c3.make_bases3d(eng.S, eng.t.n, p['N'], seed=7))
        work = eng.alloc_work(p['N'])
        out = eng.project_and_estimate(Vt, work=work)
        rhs_K, rfd_K = eng.ctx.project_sources(d.Q, d._src['b_K'], d._src['bdiv_K'], Vt, work)
        _CACHE.update(p=p, d=d, Vt=Vt, work=work, out=out, rhs_K=rhs_K, rfd_K=rfd_K, M_red=eng.ctx.project_mass(Vt))
    return _CACHE


@pytest.mark.parametrize('nmu', [1, 17, 64])
@pytest.mark.parametrize('prebuilt', [False, True])
def test_reduced_solve_batch_src(nmu, prebuilt):
    c = _setup()
    d, eng, out = c['d'], c['d'].engine, c['out']
    th = np.stack([d.theta(0.1 + 0.9 * k / nmu) for k in range(nmu)])
    phi = np.random.default_rng(nmu).standard_normal((nmu, 2))
    if prebuilt:
        eng.ctx.reduced_precond_use(eng.ctx.reduced_precond_build(d.Q, d.theta(0.5), out['B_sys']))
    try:
        u, info = poisoned(eng.ctx, lambda: eng.ctx.reduced_solve_batch_src(d.Q, th, phi, out['B_sys'], c['rhs_K']))
    finally:
        eng.ctx.reduced_precond_use(None)
    for m in sorted({0, nmu - 1}):
        ref, _ = eng.ctx.reduced_solve(d.Q, th[m], out['B_sys'], eng.ctx.combine_sources(phi[m], c['rhs_K']))
        assert _rel(u[:, :, m], ref) < 1e-10


def test_implicit_euler_src_exports():
    import torch
    c = _setup()
    d, eng, out = c['d'], c['d'].engine, c['out']
    th, nt = d.theta(c['p']['mu']), 3
    phi = np.array([[0.0, 0.0], [1.0, -1.0], [0.0, -1.0], [1.0, 0.5]])
    src = d._src
    U, info = poisoned(eng.ctx, lambda: eng.ctx.fom_implicit_euler_src(d.Q, th, d.dt, nt, eng.ops['A_diag'], eng.ops['A_cpl'],
                                                                       src['b_K'], phi))
    # step by step through the existing export with the combined load vector
    ref = [eng.ctx.zeros(eng.S, eng.t.n)]
    for k in range(nt):
        b = eng.ctx.combine_sources(phi[k + 1], src['b_K'])
        ref.append(eng.ctx.fom_implicit_euler(d.Q, th, d.dt, 1, eng.ops['A_diag'], eng.ops['A_cpl'], b, U0=ref[-1])[0][1])
    assert _rel(U, torch.stack(ref)) < 1e-8
    u, info = poisoned(eng.ctx, lambda: eng.ctx.reduced_implicit_euler_src(d.Q, th, d.dt, nt, out['B_sys'], c['M_red'], c['rhs_K'], phi))
    ref = [eng.ctx.zeros(eng.S, c['p']['N'])]
    for k in range(nt):
        rhs = eng.ctx.combine_sources(phi[k + 1], c['rhs_K'])
        ref.append(eng.ctx.reduced_implicit_euler(d.Q, th, d.dt, 1, out['B_sys'], c['M_red'], rhs, U0=ref[-1])[0][1])
    assert _rel(u, torch.stack(ref)) < 1e-9


def test_setup_projection_and_source_term_exports():
    import torch
    c = _setup()
    d, eng, out, src = c['d'], c['d'].engine, c['out'], c['d']._src
    F2 = poisoned(eng.ctx, lambda: eng.ctx.assemble_source_gram(src['f_smp_K']))
    assert torch.equal(F2, src['F2'])
    rhs_K, rfd_K = poisoned(eng.ctx, lambda: eng.ctx.project_sources(d.Q, src['b_K'], src['bdiv_K'], c['Vt'], c['work']))
    assert torch.equal(rhs_K, c['rhs_K']) and torch.equal(rfd_K, c['rfd_K'])
    assert _rel(rhs_K, torch.einsum('ksn,snj->ksj', src['b_K'], c['Vt'])) < 1e-12
    y = poisoned(eng.ctx, lambda: eng.ctx.combine_sources([0.25, -2.0], src['b_K']))
    assert _rel(y, 0.25 * src['b_K'][0] - 2.0 * src['b_K'][1]) < 1e-14
    odd = src['b_K'].reshape(2, -1)[:, :-1].contiguous()                # an odd length: the scalar form of the kernel
    y = poisoned(eng.ctx, lambda: eng.ctx.combine_sources([0.25, -2.0], odd))
    assert _rel(y, 0.25 * odd[0] - 2.0 * odd[1]) < 1e-14
    L = 11                                                               # two workgroups of eight columns, the second one partial
    u = eng.ctx.from_numpy(np.random.default_rng(1).standard_normal((eng.S, c['p']['N'], L)))
    th = np.stack([d.theta(0.2 + 0.05 * l) for l in range(L)])
    phi = np.random.default_rng(2).standard_normal((L, 2))
    args = (src['F2'], c['rfd_K'], src['bdiv_K'], out['Rb'], u, eng.ops['ceps'], eng.hdiam)
    t = poisoned(eng.ctx, lambda: eng.ctx.reduced_source_terms(d.Q, th, phi, *args))
    for l in (0, 7, 10):                                                 # column by column: the same numbers from a launch of one
        one = eng.ctx.reduced_source_terms(d.Q, th[l:l + 1], phi[l:l + 1], src['F2'], c['rfd_K'], src['bdiv_K'], out['Rb'],
                                           u[:, :, l:l + 1].contiguous(), eng.ops['ceps'], eng.hdiam)
        assert torch.equal(t[:, l], one[:, 0])
