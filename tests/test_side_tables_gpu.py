"""The context-owned side tables of the fused pass (csrc/fused.hip, k_side_tables; LRBMS_OPT_SIDE_TABLES) -- runs on the MI355X box
(`-m gpu`).

The thin side kernels read everything that does not depend on the basis -- the side-face records of ``thin_rt_body``, ``Ksc`` and
the ``M_ab`` rows of ``thin_ncf_body`` -- from tables the assembly exports build and the context keeps.  Checked here, on the smallest grids that have
every neighbour pattern (3 x 3 subdomains, k_c = 2: interior, edge and corner subdomains; 8 triangles per coarse square, n_T = 32):

- kept tables (option 1) against tables rebuilt in every pass (option 0): the same bits in all twelve outputs, over Q, even and odd
  N, both output layouts, the vertex patch, a subset pass and a template whose sides differ in face and vertex count; every shape
  also against the unfused kernels, one of them against the oracle;
- staleness: arrays re-assembled IN PLACE (same pointers, new content) must not meet the tables of their earlier content, and
  arrays that are not the context's (clones) are given tables of their own in that pass; further load vectors assembled into
  arrays of their own (one ``lrbms_assemble_rhs`` per source component) do not disown the engine's ``b``;
- a Bbb block that is not SPD still marks its subdomain's G_bb NaN, whether the tables are kept or rebuilt;
- the phases of the pass called separately and the one-call step, from a NaN-filled work buffer."""
import numpy as np
import pytest

from common import compare_all, energy_orthonormalize, make_bases, oracle_from_problem, problem_with_q_components, theta_bar_of

pytestmark = pytest.mark.gpu

TOL = 1e-11            # test_dispatch_parity_gpu.py: every array against the oracle / the unfused kernels
SOLVE_TOL = 1e-10      # ... and the reduced solve
SHAPE, KC = (3, 3), 2


def _problem(Q, shape=SHAPE, kc=KC, seed=7):
    if Q == 2 and seed == 7:
        from pylrbms_amd import multiscale_problem
        return multiscale_problem.init_grid_and_problem({'num_subdomains': list(shape), 'coarse_per_subdomain': kc})
    return problem_with_q_components(shape, kc, Q, seed=seed)


def _rectangular_problem():
    """3 x 2 subdomains of 2 x 3 coarse squares on [0, 3] x [0, 2]: sides 0 / 3 have 4 faces and 5 vertices, sides 1 / 2 have 6 and 7."""
    from pylrbms_amd.functions import make_constant_function_2x2, make_expression_function_1x1
    from pylrbms_amd.grid import DDSubdomainsGrid, make_boundary_info
    from pylrbms_amd.parameters import ExpressionParameterFunctional
    grid = DDSubdomainsGrid([0, 0], [3, 2], (6, 6), (3, 2))
    pt = {'diffusion': (1,)}
    return {'grid': grid, 'boundary_info': make_boundary_info(grid, {'type': 'xt.grid.boundaryinfo.alldirichlet'}),
            'lambda': {'functions': [make_expression_function_1x1(grid, 'x', '1+x[0]*x[1]'),
                                     make_expression_function_1x1(grid, 'x', '0.5+sin(x[0])*sin(x[0])')],
                       'coefficients': [ExpressionParameterFunctional('1.', pt), ExpressionParameterFunctional('diffusion', pt)]},
            'lambda_bar': make_expression_function_1x1(grid, 'x', '1.5+x[0]*x[1]+sin(x[0])*sin(x[0])'),
            'lambda_hat': make_expression_function_1x1(grid, 'x', '1.5+x[0]*x[1]+sin(x[0])*sin(x[0])'),
            'kappa': make_constant_function_2x2(grid, [[2., 0.5], [0.5, 1.]]),
            'f': make_expression_function_1x1(grid, 'x', 'exp(x[0])*cos(3*x[1])'),
            'mu_bar': (1.,), 'mu_hat': (1.,)}


def _engine(p, conventions=None, theta_bar=None, assemble=True):
    from pylrbms_amd.engine import Engine
    lam = p['lambda']
    eng = Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'],
                 theta_bar_of(p) if theta_bar is None else theta_bar, conventions=conventions)
    return eng.assemble() if assemble else eng


def _args(eng, V, buf, **other):
    a = {k: getattr(eng, k) for k in ('b', 'ebar', 'Aab', 'Bbb')}
    a.update(other)
    return (V, eng.F, eng.A_diag, eng.A_cpl, eng.P_diag, a['b'], a['ebar'], eng.caa, a['Aab'], a['Bbb'], buf['work'], buf['sys'],
            buf['grams'])


def _outputs(buf):
    return list(buf['sys']) + list(buf['grams'])


def _poison(buf):
    for x in _outputs(buf) + [buf['work']]:
        x.fill_(float('nan'))


def _run(eng, V, buf, phases=(0,), **other):
    """The pass into NaN-filled outputs and work; -> (clones of the outputs, timing names of the kernels that ran)."""
    _poison(buf)
    eng.ctx.kernel_timing(True)
    try:
        for ph in phases:
            eng.ctx.project_estimate_fused(*_args(eng, V, buf, **other), phase=ph)
        ran = {k for k, _ in eng.ctx.kernel_timing_read()}
    finally:
        eng.ctx.kernel_timing(False)
    return [x.clone() for x in _outputs(buf)], ran


def _assert_equal(got, want, tag):
    import torch
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(b).all()), (tag, i)
        assert torch.equal(a, b), '{}: output {} differs (max |diff| {})'.format(
            tag, i, float((a - b).abs().nan_to_num(float('inf')).max()))


def _kept_vs_rebuilt(eng, V, N, factored, check_unfused=True):
    """Option 1 (tables kept: no builder launch in the pass) against option 0 (rebuilt in every pass), twelve (dense layout: ten)
    outputs bit for bit; then against the unfused kernels.

    Both options run the same table-reading kernels on tables of the same builder: their bit-equality shows that KEEPING equals
    REBUILDING, nothing more.  That the tables reproduce the expressions the kernels evaluated before rests on the comparison with
    the unfused kernels below (1e-11), on ``test_against_the_oracle`` and on the ``bench.py --dump-outputs`` comparison of the
    parent's and this library's outputs (bit-identical; ``profiles/r12_thin_ab.txt``)."""
    from pylrbms_amd.engine import expand_factored_grams
    buf = eng.alloc_reduce_buffers(N, factored=factored)
    assert len(_outputs(buf)) == (12 if factored else 10)
    try:
        _run(eng, V, buf)                                # (an engine shared with a test that handed it foreign arrays rebuilds once)
        kept, ran1 = _run(eng, V, buf)
        assert 'k_side_tables' not in ran1, sorted(ran1)
        eng.ctx.set_option('side_tables', 0)
        rebuilt, ran0 = _run(eng, V, buf)
        assert 'k_side_tables' in ran0, sorted(ran0)
    finally:
        eng.ctx.set_option('side_tables', 1)
    _assert_equal(kept, rebuilt, 'kept vs rebuilt')
    again, ran = _run(eng, V, buf)                       # back at option 1: the tables of the last rebuild serve
    assert 'k_side_tables' not in ran, sorted(ran)
    _assert_equal(again, kept, 'kept again')
    if check_unfused:
        ref = eng.project_and_estimate(V, fused=False)
        ref = list(ref['sys']) + list(ref['grams'])
        got = kept[:4] + list(expand_factored_grams(tuple(kept[4:]))) if factored else kept
        floor = float(V.abs().max()) ** 2 * 1e-3
        for i, (a, b) in enumerate(zip(got, ref)):
            assert a.shape == b.shape, i
            err = float((a - b).abs().max()) / max(float(b.abs().max()), floor)
            assert err <= TOL, (i, err)
    return kept, buf


_ENGINES = {}


def _shared_engine(Q):
    if Q not in _ENGINES:
        _ENGINES[Q] = _engine(_problem(Q))
    return _ENGINES[Q]


@pytest.mark.parametrize('N', [6, 7])
@pytest.mark.parametrize('Q', [1, 2, 3])
def test_kept_tables_give_the_bits_of_rebuilt_ones(Q, N):
    """Factored layout; N = 7 runs the one-column paths of the thin kernels."""
    eng = _shared_engine(Q)
    assert eng.t.n_T == 8 * KC * KC and eng.S == 9 and eng.ctx.fused_supported(Q, N, factored=True)
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=3 + N))
    _kept_vs_rebuilt(eng, V, N, True)


def test_dense_layout():
    eng = _shared_engine(2)
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, 6, seed=21))
    for streams in (-1, 0):          # k_thin (one launch) and the separate k_thin_rt
        eng.ctx.set_option('streams', streams)
        try:
            _kept_vs_rebuilt(eng, V, 6, False)
        finally:
            eng.ctx.set_option('streams', -1)


def test_unforked_factored_pass():
    """LRBMS_OPT_STREAMS 0 in the factored layout: k_thin3 on the caller's stream."""
    eng = _shared_engine(2)
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, 6, seed=22))
    eng.ctx.set_option('streams', 0)
    try:
        _kept_vs_rebuilt(eng, V, 6, True)
    finally:
        eng.ctx.set_option('streams', -1)


def test_vertex_patch():
    eng = _engine(_problem(2), conventions={'oswald_vertex_patch': True})
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, 6, seed=23))
    _kept_vs_rebuilt(eng, V, 6, True, check_unfused=False)       # (the patch enters through the factored layout only)


def test_subset_pass_into_the_buffers_of_a_whole_pass():
    import torch
    eng = _shared_engine(2)
    N = 6
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=24))
    whole, buf = _kept_vs_rebuilt(eng, V, N, True)
    subset = [0, 4, 5, 8]                                 # a corner, the interior subdomain, an edge, another corner
    rest = torch.tensor([i for i in range(eng.S) if i not in subset], device=V.device)
    for opt in (1, 0):
        eng.ctx.set_option('side_tables', opt)
        try:
            for x in _outputs(buf):
                x.fill_(7.0)
            buf['work'].fill_(float('nan'))
            eng.project_and_estimate(V, buf, subset=subset)
        finally:
            eng.ctx.set_option('side_tables', 1)
        sub = torch.tensor(subset, device=V.device)
        for i, (a, b) in enumerate(zip(whole, _outputs(buf))):
            sdim = 1 if (a.dim() >= 2 and a.shape[0] == eng.Q and a.shape[1] == eng.S) else 0
            if a.dim() >= 3 and a.shape[0] == eng.Q and a.shape[1] == eng.Q and a.shape[2] == eng.S:
                sdim = 2
            assert torch.equal(a.index_select(sdim, sub), b.index_select(sdim, sub)), (opt, i)
            assert bool((b.index_select(sdim, rest) == 7.0).all()), (opt, i)


def test_sides_of_different_face_and_vertex_count():
    eng = _engine(_rectangular_problem())
    t = eng.t
    assert eng.S == 6 and t.n_T == 48
    V = eng.ctx.from_numpy(make_bases(eng.S, t.n, 6, seed=25))
    _kept_vs_rebuilt(eng, V, 6, True)


def test_against_the_oracle():
    p = _problem(2)
    eng = _engine(p)
    d = oracle_from_problem(p)
    V = energy_orthonormalize(make_bases(d.S, d.n, 6, seed=3), d)
    res = compare_all(p, eng, V, 0.3, oracle=d)
    assert res.pop('cg_iterations') > 0
    assert 'fused_B_sys' in res and 'fused_dense_B_sys' in res
    bad = {k: v for k, v in res.items() if not (v < (SOLVE_TOL if k == 'u_solve' else TOL))}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------- staleness

def _second_data(Q=2):
    """Another coefficient field and another theta_bar on the grid of _problem(2)."""
    p2 = problem_with_q_components(SHAPE, KC, Q, seed=11)
    return p2, np.array([0.7, 0.35])


def test_reassembly_in_place_does_not_leave_stale_tables():
    """Assemble, pass, assemble again INTO THE SAME ARRAYS with another theta_bar and coefficient field, pass: the bits of a fresh
    context assembled with the second data.  (A build that keys the kept tables on the pointers alone fails here.)"""
    N = 6
    eng = _engine(problem_with_q_components(SHAPE, KC, 2, seed=5))      # (the same kind of data functions as the second data: one quadrature)
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=31))
    buf = eng.alloc_reduce_buffers(N, factored=True)
    first, _ = _run(eng, V, buf)
    p2, tb2 = _second_data()
    fresh = _engine(p2, theta_bar=tb2)
    want, _ = _run(fresh, fresh.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=31)), fresh.alloc_reduce_buffers(N, factored=True))
    src = fresh                                            # its sampled data (same device), handed to the first context's exports
    assert eng.ctx.quad.lam_stride == src.ctx.quad.lam_stride and eng.lam.shape == src.lam.shape
    ptrs = [x.data_ptr() for x in (eng.b, eng.ebar, eng.Aab, eng.Bbb)]
    c = eng.ctx
    eng.A_diag, eng.A_cpl = c.assemble_swipdg(src.lam)
    eng.F = c.assemble_flux(src.lam)
    c.assemble_rhs(src.f_smp, src.lhat, out=(eng.b, eng.f2, eng.ceps))
    c.assemble_products(tb2, src.lam, src.lam_df, src.lbar, src.lhat, out=(eng.P_diag, eng.ebar, eng.caa, eng.Aab, eng.Bbb))
    assert ptrs == [x.data_ptr() for x in (eng.b, eng.ebar, eng.Aab, eng.Bbb)]
    got, ran = _run(eng, V, buf)
    assert 'k_side_tables' not in ran, sorted(ran)         # the assembly exports built the tables of the new content
    _assert_equal(got, want, 're-assembled in place')
    assert any(not bool((a == b).all()) for a, b in zip(got[4:], first[4:]))      # (the second data is another problem)


def test_new_right_hand_side_in_place():
    """Only b changes (lrbms_assemble_rhs into the same array): r_fd, F_side and rhs_red follow."""
    N = 6
    p = _problem(2)
    eng = _engine(p)
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=32))
    buf = eng.alloc_reduce_buffers(N, factored=True)
    first, _ = _run(eng, V, buf)
    f2nd = (eng.f_smp * 1.75 + 0.5).contiguous()
    fresh = _engine(p, assemble=False)
    fresh.f_smp = fresh.ctx.from_numpy(f2nd.cpu().numpy())
    fresh.assemble()
    want, _ = _run(fresh, fresh.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=32)), fresh.alloc_reduce_buffers(N, factored=True))
    ptr = eng.b.data_ptr()
    eng.ctx.assemble_rhs(f2nd, eng.lhat, out=(eng.b, eng.f2, eng.ceps))
    assert eng.b.data_ptr() == ptr
    got, _ = _run(eng, V, buf)
    _assert_equal(got, want, 'new b in place')
    r_fd = 4 + 1
    assert not bool((got[r_fd] == first[r_fd]).all())


def test_arrays_that_are_not_the_contexts_get_their_own_tables():
    """A pass handed clones of the assembled arrays rebuilds the tables (one extra launch, k_side_tables) in EVERY such pass -- the
    library cannot see a write into an array it did not assemble -- and gives the same bits; modified clones give the bits of a
    context that assembled the modified data."""
    N = 6
    eng = _shared_engine(2)
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=33))
    buf = eng.alloc_reduce_buffers(N, factored=True)
    _run(eng, V, buf)
    want, ran = _run(eng, V, buf)
    assert 'k_side_tables' not in ran
    clones = {k: getattr(eng, k).clone() for k in ('b', 'ebar', 'Aab', 'Bbb')}
    for _ in range(2):
        got, ran = _run(eng, V, buf, **clones)
        assert 'k_side_tables' in ran, sorted(ran)
        _assert_equal(got, want, 'clones')
    one = {'b': clones['b']}                               # one foreign array among the context's own
    got, ran = _run(eng, V, buf, **one)
    assert 'k_side_tables' in ran
    _assert_equal(got, want, 'cloned b')
    clones['b'].mul_(2.0)                                  # written behind the library's back: the rebuilt tables follow
    clones['ebar'].mul_(0.5)
    got, ran = _run(eng, V, buf, **clones)
    assert 'k_side_tables' in ran
    r_fd, F_nc = 4 + 1, 4 + 7
    assert bool((got[r_fd] == 2.0 * want[r_fd]).all()) and bool((got[F_nc][..., 2 * N:] == 0.5 * want[F_nc][..., 2 * N:]).all())
    back, ran = _run(eng, V, buf)                          # the context's own arrays again: rebuilt once, then kept
    assert 'k_side_tables' in ran
    _assert_equal(back, want, 'own arrays again')
    _, ran = _run(eng, V, buf)
    assert 'k_side_tables' not in ran


def test_further_load_vectors_do_not_disown_the_engines():
    """``lrbms_assemble_rhs`` once per source component into arrays of their own (``sources.setup_sources``): the passes go on with
    ``eng.b`` and its kept tables -- no builder launch, the same bits.  A pass that is handed one of the new load vectors builds its
    tables once and keeps them; back at ``eng.b`` likewise."""
    N = 6
    eng = _engine(_problem(2))
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=36))
    buf = eng.alloc_reduce_buffers(N, factored=True)
    want, ran = _run(eng, V, buf)
    assert 'k_side_tables' not in ran, sorted(ran)
    eng.ctx.kernel_timing(True)
    try:
        others = [eng.ctx.assemble_rhs((eng.f_smp * (2.0 + j)).contiguous(), eng.lhat) for j in range(3)]
        built = {k for k, _ in eng.ctx.kernel_timing_read()}
    finally:
        eng.ctx.kernel_timing(False)
    assert 'k_side_tables' not in built, sorted(built)      # (nor a table build for a component no pass is handed)
    for _ in range(2):
        got, ran = _run(eng, V, buf)
        assert 'k_side_tables' not in ran, sorted(ran)
        _assert_equal(got, want, 'eng.b after further load vectors')
    b2 = others[2][0]
    first, ran = _run(eng, V, buf, b=b2)
    assert 'k_side_tables' in ran
    again, ran = _run(eng, V, buf, b=b2)
    assert 'k_side_tables' not in ran, sorted(ran)           # an array this context assembled: kept
    _assert_equal(again, first, 'second load vector')
    r_fd = 4 + 1
    assert bool((first[r_fd] == 4.0 * want[r_fd]).all())     # (f scaled by 4: exact in every term)
    back, ran = _run(eng, V, buf)
    assert 'k_side_tables' in ran
    _assert_equal(back, want, 'back at eng.b')
    _, ran = _run(eng, V, buf)
    assert 'k_side_tables' not in ran
    from pylrbms_amd.sources import setup_sources             # the project's own caller of that pattern
    src = setup_sources(eng, [eng._init_args[2]], [1.0])
    assert src['K'] == 1
    got, ran = _run(eng, V, buf)
    assert 'k_side_tables' not in ran, sorted(ran)
    _assert_equal(got, want, 'after setup_sources')


def _registered(ctx, kind):
    import ctypes
    buf = (ctypes.c_void_p * 64)()
    n = ctx.lib.lrbms_assembled_arrays(ctx.handle, kind, buf, 64)
    assert 0 <= n <= 64
    return [int(buf[i] or 0) for i in range(n)]


def test_a_fresh_clone_after_setup_sources_is_foreign():
    """``setup_sources`` with K = 3 components registers three more load vectors.  A freshly allocated clone of ``b`` handed to a pass
    afterwards must not land on an address the context still trusts: the binding holds every registered array, so the clone is
    foreign -- both passes build their tables, and the second follows what was written into the clone in between."""
    import gc
    from pylrbms_amd.sources import setup_sources
    N = 6
    eng = _engine(_problem(2))
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=37))
    buf = eng.alloc_reduce_buffers(N, factored=True)
    want, _ = _run(eng, V, buf)
    f = eng._init_args[2]
    src = setup_sources(eng, [f, f, f], [1.0, 1.0, 1.0])
    assert src['K'] == 3
    known = _registered(eng.ctx, 2)
    assert eng.b.data_ptr() in known and len(known) == 4
    pinned = {ptr for kind, ptr in eng.ctx._pins if kind == 2}
    assert pinned == set(known)                             # pins and register agree
    for kind, name in ((0, 'Bbb'), (1, 'Aab'), (3, 'ebar')):
        assert _registered(eng.ctx, kind) == [getattr(eng, name).data_ptr()]
    # loose load vectors as well (assembled into arrays of their own and dropped by the caller): still registered, so still held
    for j in range(3):
        eng.ctx.assemble_rhs((eng.f_smp * (2.0 + j)).contiguous(), eng.lhat)
    del src
    gc.collect()
    known = set(_registered(eng.ctx, 2))
    assert len(known) == 7
    clones = [eng.b.clone() for _ in range(8)]              # more fresh blocks of that size than load vectors were dropped
    assert not ({c.data_ptr() for c in clones} & known)
    r_fd = 4 + 1
    for clone in clones[:2]:
        got, ran = _run(eng, V, buf, b=clone)
        assert 'k_side_tables' in ran, sorted(ran)
        _assert_equal(got, want, 'clone of b')
        clone.mul_(2.0)                                     # written behind the library's back
        got, ran = _run(eng, V, buf, b=clone)
        assert 'k_side_tables' in ran, sorted(ran)
        assert bool((got[r_fd] == 2.0 * want[r_fd]).all()) and not bool((want[r_fd] == 0.0).all())


def test_many_load_vectors_do_not_evict_the_array_of_the_kept_tables():
    """More load vectors than the register remembers (32): the oldest go, the binding lets go of them, but the ``b`` the kept tables
    were built from stays -- the passes with ``eng.b`` launch no builder."""
    N = 6
    eng = _engine(_problem(2))
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=38))
    buf = eng.alloc_reduce_buffers(N, factored=True)
    want, _ = _run(eng, V, buf)
    f_smp = (eng.f_smp * 2.0).contiguous()
    for _ in range(40):
        eng.ctx.assemble_rhs(f_smp, eng.lhat)
    known = _registered(eng.ctx, 2)
    assert len(known) == 32 and known[0] == eng.b.data_ptr()
    assert {ptr for kind, ptr in eng.ctx._pins if kind == 2} == set(known)
    got, ran = _run(eng, V, buf)
    assert 'k_side_tables' not in ran, sorted(ran)
    _assert_equal(got, want, 'eng.b after 40 further load vectors')


# ---------------------------------------------------------------------------------------------------------- non-SPD Bbb

@pytest.mark.parametrize('opt', [1, 0])
def test_non_spd_flux_mass_still_marks_its_subdomain(opt):
    import torch
    N = 6
    eng = _shared_engine(2)
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=34))
    buf = eng.alloc_reduce_buffers(N, factored=True)
    good, _ = _run(eng, V, buf)
    Bbb = eng.Bbb.clone()
    B4 = Bbb.view(eng.S, -1, 3, 3)
    s0, T0 = eng.S // 2, B4.shape[1] // 3
    B4[s0, T0, 1, 1] = -B4[s0, T0, 1, 1]                   # pivot 1 of the Cholesky factor < 0
    eng.ctx.set_option('side_tables', opt)
    try:
        _poison(buf)
        eng.ctx.project_estimate_fused(*_args(eng, V, buf, Bbb=Bbb), phase=0)
    finally:
        eng.ctx.set_option('side_tables', 1)
    G_bb, G_bb_good = buf['grams'][3], good[4 + 3]
    assert bool(torch.isnan(G_bb[s0]).all())
    others = [s for s in range(eng.S) if s != s0]
    assert torch.equal(G_bb[others], G_bb_good[others]) and bool(torch.isfinite(G_bb_good).all())


# ---------------------------------------------------------------------------------------------------------- work buffer, call order

@pytest.mark.parametrize('opt', [1, 0])
def test_phases_from_a_poisoned_work_buffer(opt):
    """Phases 1 - 4 called separately and the one-call step (phase 5), the work buffer NaN-filled in front of each sequence: the bits
    of the whole pass.  (Option 0: the call that runs the halo-dependent half rebuilds the tables.)"""
    import torch
    N = 6
    eng = _shared_engine(2)
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=35))
    buf = eng.alloc_reduce_buffers(N, factored=True)
    want, _ = _run(eng, V, buf)
    eng.ctx.set_option('side_tables', opt)
    try:
        for phases in ((1, 2), (3, 4, 2), (5,), (0,)):
            got, ran = _run(eng, V, buf, phases=phases)
            assert ('k_side_tables' in ran) == (opt == 0), (phases, sorted(ran))
            _assert_equal(got, want, phases)
        # the halo-dependent half alone, over outputs and a work buffer that keep only what the first half wrote
        _poison(buf)
        eng.ctx.project_estimate_fused(*_args(eng, V, buf), phase=1)
        torch.cuda.synchronize()
        eng.ctx.project_estimate_fused(*_args(eng, V, buf), phase=2)
        _assert_equal([x.clone() for x in _outputs(buf)], want, 'phase 1, sync, phase 2')
    finally:
        eng.ctx.set_option('side_tables', 1)
