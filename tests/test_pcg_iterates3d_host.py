"""The restatements of tests/pcg3d_ref.py and the cells of tests/test_pcg_iterates3d_gpu.py, on the CPU.

- A mirror of the host dispatch of pylrbms_amd/csrc/online3d.hip and lrbms3d.hip, read from the source text: ``launch_matvec3``
  (N <= 16 | N <= 32 | VALU), ``red_batch_run`` (number of groups, installed or not), the ``nc`` ladder of ``fom_coarse``, both loops of
  ``sum_partials`` and of ``k3_reduce1`` as functions of the partial count, and the dynamic LDS of ``k3_block_inverse`` either side
  of 65 536 bytes.  The cell lists of the GPU module must reach every branch; the ``nc S > 8192 -> none`` rung of ``fom_coarse``
  (8 193 subdomains) is checked here only.
- On operators that exist on the CPU (the oracle's ``Reductor3D`` blocks through ``common3d.oracle_dense_blocks``, its assembled
  full-order blocks through ``common3d.oracle_assembled``, its mass matrix): every restated preconditioner is SPD, the reference
  PCG of every cell type converges to the direct solve, and every mutant of a cell misses the reference at k = MUTANT_K by more
  than MUTANT_FLOOR while the reference ratio there is still >= MIN_RATIO."""
import re

import numpy as np
import pytest

import common3d as c3
import fom_batch3d_ref as ref3
import pcg3d_ref as r3
import pcg_ref
import test_pcg_iterates3d_gpu as cells
from test_pcg_iterates_gpu import MIN_RATIO, MUTANT_FLOOR, TOL_X

LDS_DEFAULT = 64 * 1024
K2 = cells.MUTANT_K


def _src():
    return c3.source3d()


# ------------------------------------------------------------------------------------------------ the dispatch mirror
def _function(src, head):
    """The text of the function whose definition starts with ``head``, up to the first closing brace in column 0."""
    at = src.index(head)
    return src[at:src.index('\n}\n', at)]


def partial_loop(src, head):
    """(threads, unroll) of a partial-sum function: ``for (; k + (U - 1) * T < S; k += U * T)`` then ``for (; k < S; k += T)``."""
    body = _function(src, head)
    a, t1, u, t2 = map(int, re.search(r'for \(; k \+ (\d+) \* (\d+) < S; k \+= (\d+) \* (\d+)\)', body).groups())
    t3 = int(re.search(r'for \(; k < S; k \+= (\d+)\)', body).group(1))
    assert t1 == t2 == t3 and a == u - 1, (head, a, t1, u, t2, t3)
    return t1, u


def loop_rounds(count, threads, unroll):
    """{(rounds of the unrolled body, rounds of the tail)} over the threads of a partial sum of ``count`` entries."""
    out = set()
    for i in range(threads):
        k, body, tail = i, 0, 0
        while k + (unroll - 1) * threads < count:
            k += unroll * threads
            body += 1
        while k < count:
            k += threads
            tail += 1
        out.add((body, tail))
    return out


def loop_kinds(count, threads, unroll):
    """Which of {'body', 'tail', 'body+tail'} some thread of the sum goes through."""
    return {('body' if b else '') + ('+' if b and t else '') + ('tail' if t else '') for b, t in loop_rounds(count, threads, unroll)} - {''}


def block_inverse_lds(N, src):
    expr = re.search(r'hipLaunchKernelGGL\(k3_block_inverse, dim3\(S\), dim3\(256\), ([^,]*\([^)]*\)), st, N, w\.Amu', src).group(1)
    return int(eval(expr.replace('sizeof(double)', '8'), {}, {'N': N}))


def matvec_form(N, valu, src):
    """The kernel ``launch_matvec3`` picks: ('mfma', row tiles) or ('valu',)."""
    body = _function(src, 'void launch_matvec3(')
    bound = int(re.search(r'if \(mfma_mv && N <= (\d+)\)', body).group(1))
    forms = re.findall(r'k3b_matvec_mfma<(\d), MASS>', body)
    assert forms == ['1', '2'] and 'hipLaunchKernelGGL(k3b_matvec<MASS>' in body
    if valu:
        return ('valu',)
    return ('mfma', 1 if N <= bound else 2)


def batch_limits(src):
    body = _function(src, 'int lrbms3_reduced_solve_batch(')
    return tuple(map(int, re.search(r'N > (\d+) \|\| nmu < 1 \|\| nmu > (\d+)', body).groups()))


def batch_groups(nmu, src):
    """Columns per group of ``red_batch_run``."""
    body = _function(src, 'int red_batch_run(')
    w = int(re.search(r'const int ng = \(nmu \+ (\d+)\) / (\d+);', body).group(2))
    assert w == r3.GROUP and 'G.nm = nmu - G.m0 < {0} ? nmu - G.m0 : {0};'.format(w) in body
    assert 'mean.v[q] += theta[(G.m0 + m) * Q + q] / G.nm;' in body                      # what ``group_means`` restates
    assert 'const double* A0inv = ctx->user_pc_N == N ? ctx->user_pc : nullptr;' in body
    return [min(w, nmu - g) for g in range(0, nmu, w)]


def fom_nc(nc, S, coarse_opt, src):
    """The ``nc`` ``fom_coarse`` arrives at before the factorisation (0: the element blocks alone)."""
    cap = int(re.search(r'constexpr int FOM_MAX_COARSE = (\d+);', src).group(1))
    body = _function(src, 'int fom_coarse(')
    assert 'int nc = coarse_env ? ctx->fom_nc : 0;' in body
    assert 'if (nc > 1 && (long)nc * S > FOM_MAX_COARSE) nc = 1;' in body and 'if ((long)nc * S > FOM_MAX_COARSE) nc = 0;' in body
    assert 'if (hinfo != 0) nc = 0;' in body
    assert cap == ref3.COARSE_MAX
    nc = nc if coarse_opt else 0
    if nc > 1 and nc * S > cap:
        nc = 1
    if nc * S > cap:
        nc = 0
    return nc


def _count(shape):
    return int(np.prod(shape))


def test_cells_reach_both_loops_of_the_partial_sums():
    src = _src()
    t, u = partial_loop(src, '__device__ inline double sum_partials(')
    assert (t, u) == (64, 8)
    kinds = [loop_kinds(_count(g), t, u) for g in cells.PARTIAL_GRIDS]
    assert {'tail'} in kinds, 'no cell runs the tail of sum_partials alone'
    assert {'body'} in kinds, 'no cell runs the unrolled body of sum_partials alone'
    assert {'body', 'tail'} in kinds, 'no cell has threads in the body and threads in the tail'
    assert {'body+tail'} in kinds, 'no cell runs body then tail in every thread'
    assert [_count(g) for g in cells.PARTIAL_GRIDS] == [448, 504, 512, 600]
    # every other cell of the single solve is below the body: the large grids are the only ones that reach it
    assert loop_kinds(27, t, u) == {'tail'}
    t, u = partial_loop(src, '__global__ __launch_bounds__(256) void k3_reduce1(')
    assert (t, u) == (256, 8)
    S = _count(cells.REDUCE_GRID)
    assert loop_kinds(S, t, u) == {'body+tail', 'body'} and S == 2197        # red_cg: |r|^2 over S partials
    assert all(loop_kinds(_count(g), t, u) == {'tail'} for g in cells.PARTIAL_GRIDS)
    # fom_cg on the capped grid: r.z over nblk + M = 2 S partials (two rounds of the body, then the tail), |r|^2 and p.Ap over nblk = S
    assert _count(cells.CAP_GRID) == S and loop_rounds(2 * S, t, u) == {(2, 1), (2, 2)}


def test_cells_reach_both_sides_of_the_block_inverse_lds_threshold():
    src = _src()
    first = next(N for N in range(1, 65) if block_inverse_lds(N, src) > LDS_DEFAULT)
    assert block_inverse_lds(64, src) == 66048
    assert {N for _, N in cells.LDS_CELLS} == {first - 1, first} == {63, 64}
    limit = int(re.search(r'N < 1 \|\| N > (\d+) \|\| !theta \|\| !B_sys \|\| !rhs_red \|\| !work \|\| !u\)', src).group(1))
    assert limit == 64


def test_cells_reach_every_matvec_form_and_group_count():
    src = _src()
    nmax, mmax = batch_limits(src)
    assert (nmax, mmax) == (32, 64) and cells.NMAX == nmax
    forms = {matvec_form(N, False, src) for N, _ in cells.BATCH_CELLS} | {matvec_form(cells.VALU_CELL[0], True, src)}
    assert forms == {('mfma', 1), ('mfma', 2), ('valu',)}
    Ns = {N for N, _ in cells.BATCH_CELLS}
    assert {16, 17, nmax} <= Ns                                             # both sides of the row-tile bound, the largest N
    groups = {nmu: batch_groups(nmu, src) for _, nmu in cells.BATCH_CELLS}
    assert {len(g) for g in groups.values()} == {1, 2, 3, 4}
    assert [1] in groups.values() and [16] in groups.values() and [16, 1] in groups.values() and [16] * 4 in groups.values()
    assert len(batch_groups(cells.VALU_CELL[1], src)) > 1 and len(batch_groups(cells.SRC_CELL[1], src)) > 1
    # every cell runs with and without an installed preconditioner (the parametrisation of the GPU test)
    S_big = _count(cells.BIG_INSTALLED[0])
    rows = int(re.search(r'k3b_coarse_apply, dim3\(\(unsigned\)\(\(S \+ (\d+)\) / (\d+)\)\)', src).group(2))
    assert S_big % rows not in (0,) and S_big // rows >= 2                  # a partial last workgroup behind full ones


def test_cells_reach_every_rung_of_the_fom_coarse_ladder():
    src = _src()
    S3 = 27
    nc_of = {'p1': 4, 'constants': 1, 'off': 4, 'deficient': 2}
    reached = {fom_nc(nc_of[space], S3, space != 'off', src) for name, space in cells.FOM_CELLS if name == cells.SWEEP}
    assert reached == {4, 1, 0, 2}                                          # (2: the factorisation then fails, ``hinfo != 0``)
    assert {space for _, space in cells.FOM_CELLS} == {'p1', 'constants', 'off', 'deficient'}
    assert {name for name, _ in cells.FOM_CELLS} == {'interior_3x3x3', 'kc_3x1x2', 'q3_2x1x2'}
    assert fom_nc(4, _count(cells.CAP_GRID), True, src) == 1                # constants instead of P1
    assert fom_nc(4, 2048, True, src) == 4 and fom_nc(4, 2049, True, src) == 1
    # the last rung -- no GPU cell: 8 193 subdomains
    assert fom_nc(4, 8192, True, src) == 1 and fom_nc(4, 8193, True, src) == 0 and fom_nc(1, 8193, True, src) == 0
    # the reference takes the same ladder
    import scipy.sparse as sp
    for S, want in ((3, 4), (2049, 1)):
        P = ref3.BatchFomPrecond3D(sp.identity(10 * S, format='csr'), sp.identity(10 * S, format='csr'), S, 10,
                                   np.concatenate([np.ones((10, 1)), np.eye(10)[:, :3]], axis=1))
        assert P.A1.shape == (want * S, want * S)


def test_the_loops_honour_max_iter_and_the_euler_steps_finish_a_missed_step():
    """What the GPU module relies on, from the source: the loops stop at max_iter exactly, and a step of the single Euler
    steppers that misses rtol still adds u_k to the correction (U[k + 1] = u_k + d_k) before the call returns."""
    src = _src()
    for head in ('int red_cg(', 'int fom_cg('):
        body = _function(src, head)
        assert 'while (it < max_iter) {' in body and 'k < check && it < max_iter; ++k, ++it' in body
        assert 'if (info) info[0] = it, info[1] = rel;' in body
    assert 'if (G.done || G.it >= max_iter) continue;' in _function(src, 'int red_batch_iterate(')
    # k3p_axpy lives beside red_euler_run (online3d.hip), which launches it directly; fom_euler_run reaches it through launch_axpy
    for head, launch in (('int fom_euler_run(', 'launch_axpy('), ('int red_euler_run(', 'hipLaunchKernelGGL(k3p_axpy')):
        body = _function(src, head)
        miss = body.index('if (rc != LRBMS_OK && rc != LRBMS_E_NOT_CONVERGED) return rc;')
        axpy = body.index(launch, miss)
        assert body.index('if (rc != LRBMS_OK) return rc;', axpy) > axpy
    assert 'hipLaunchKernelGGL(k3p_axpy' in _function(src, 'void launch_axpy(')


def test_mirror_fails_on_a_changed_dispatch():
    """Scratch copies of the source: a moved row-tile bound and a shorter unroll change what the mirror reports."""
    src = _src()
    moved = src.replace('if (mfma_mv && N <= 16)', 'if (mfma_mv && N <= 20)', 1)
    assert moved != src and {matvec_form(N, False, moved) for N, _ in cells.BATCH_CELLS if N > 16} != \
        {matvec_form(N, False, src) for N, _ in cells.BATCH_CELLS if N > 16}
    body = _function(src, '__device__ inline double sum_partials(')
    short = src.replace(body, body.replace('k + 7 * 64 < S; k += 8 * 64', 'k + 3 * 64 < S; k += 4 * 64'), 1)
    t, u = partial_loop(short, '__device__ inline double sum_partials(')
    assert (t, u) == (64, 4) and {'tail'} not in [loop_kinds(_count(g), t, u) for g in cells.PARTIAL_GRIDS]


def test_group_means_accumulate_in_column_order():
    th = np.array([[1.0, 0.1], [1.0, 1e-17], [1.0, 0.7]] + [[1.0, 0.3]] * 14)
    m = r3.group_means(th)
    acc = 0.0
    for v in th[:16, 1]:
        acc = acc + v / 16
    assert m.shape == (2, 2) and m[0, 1] == acc and m[1, 1] == 0.3 / 1 and m[0, 0] == 1.0


# ------------------------------------------------------------------------------------------- operators on the CPU: reduced
_RED, _FOM = {}, {}


def _reduced(name, N, pad=None):
    """The oracle's reduced system in the product's layout: dict(p, o, nbr, B [Q, S, 7, N, N], rhs [S, N], M [S, N, N], keep)."""
    key = (name, N, pad)
    if key not in _RED:
        p = c3.make_problem(name)
        o = c3.oracle_of(p)
        V = c3.make_bases3d(o.S, o.n, N, seed=3)
        keep = np.ones((o.S, N))
        if pad is not None:
            V[pad[0], :, N - pad[1]:] = 0.0
            keep[pad[0], N - pad[1]:] = 0.0
        pN = dict(p, N=N)
        rd = c3.reduce_with_oracle(pN, o, V)
        B = np.stack([c3.oracle_dense_blocks(pN, o, rd, ii)['B_sys'] for ii in range(o.S)], axis=1)
        Mt = o.M.tocsr()
        M = np.stack([V[ii].T @ (Mt[o.dofs_of(ii)][:, o.dofs_of(ii)] @ V[ii]) for ii in range(o.S)])
        _RED[key] = dict(p=p, o=o, nbr=np.asarray(p['grid'].neighbor_slots), B=B, rhs=np.stack(rd.rhs), M=M, keep=keep, rd=rd)
    return _RED[key]


def _cut(s, N):
    return np.ascontiguousarray(s['B'][..., :N, :N]), np.ascontiguousarray(s['rhs'][:, :N])


def _thetas(s, nmu):
    return np.stack([c3.theta_of(s['p'], mu) for mu in cells._mus(nmu)])


def _separates(cell, mutant, what):
    """The mutant misses the reference at k = MUTANT_K by more than MUTANT_FLOOR while the reference ratio is still >= MIN_RATIO."""
    X, ratios = cell.iterate(K2)
    assert ratios[np.linalg.norm(X, axis=0) > 0.0].min() >= MIN_RATIO, (what, ratios)
    err = r3.miss(mutant.iterate(K2)[0], X)
    assert err > MUTANT_FLOOR, (what, err)
    return err


def _converges(cell, k, cols=None):
    X, ratios = cell.iterate(k)
    assert ratios.max() < 1e-12, ratios.max()
    for j in (range(cell.m) if cols is None else cols):
        if cell.cols[:, j].any():
            ref = cell.solve(j)
            assert np.linalg.norm(X[:, j] - ref) < 1e-9 * np.linalg.norm(ref), j


def test_reduced_operator_of_the_seven_slot_layout_is_the_oracle_system():
    s = _reduced('q3_2x1x2', 6)
    o, rd = s['o'], s['rd']
    mu = s['p']['mu']
    A = pcg_ref.reduced_operator(pcg_ref.combine_reduced(s['B'], c3.theta_of(s['p'], mu)), s['nbr']).toarray()
    x = np.linalg.solve(A, s['rhs'].ravel())
    want = np.concatenate(rd.solve(mu))
    assert np.linalg.norm(x - want) < 1e-10 * np.linalg.norm(want)
    assert np.abs(A - A.T).max() < 1e-12 * np.abs(A).max()


def test_restated_reduced_preconditioners_are_spd():
    s = _reduced(cells.SWEEP, 5)
    B, rhs = s['B'], s['rhs']
    n = rhs.size
    th, th_b = c3.theta_of(s['p'], 0.3), c3.theta_of(s['p'], cells.BUILD_MU)
    for apply in (r3.reduced_blocks_precond(B, th), r3.reduced_two_level(B, s['nbr'], th_b, th_b), r3.reduced_two_level(B, s['nbr'], th, th_b),
                  r3.reduced_blocks_precond(B, th, s['M'], cells.DT), r3.reduced_blocks_precond(B, th, None, cells.DT)):
        lo, asym = pcg_ref.spd_check(pcg_ref.precond_matrix(apply, n))
        assert lo > 0.0 and asym < 1e-12, (lo, asym)


def test_single_reduced_reference_converges_and_sees_its_blocks():
    s = _reduced(cells.SWEEP, 17)
    th = c3.theta_of(s['p'], s['p']['mu'])
    for N in (1, 2, 5, 17):
        B, rhs = _cut(s, N)
        cell = r3.reduced_single(B, s['nbr'], th, rhs)
        _converges(cell, 27 * N)
        _separates(cell, r3.reduced_single(B, s['nbr'], th, rhs, block_theta=c3.theta_of(s['p'], cells.BUILD_MU)), ('single', N))


def test_ragged_reference_keeps_the_padded_unknowns_at_zero():
    name, N, sub, count = cells.RAGGED_CELL
    s = _reduced(name, N, pad=(sub, count))
    keep = s['keep']
    assert not s['B'][:, sub, 3, N - 1].any() and not s['rhs'][sub, N - count:].any()
    cell = r3.reduced_single(s['B'], s['nbr'], c3.theta_of(s['p'], s['p']['mu']), s['rhs'], keep=keep)
    for k in cells.K_STEPS:
        X, _ = cell.iterate(k)
        assert np.all(X.reshape(keep.shape)[keep == 0] == 0.0)
    _converges(cell, 27 * N)


@pytest.mark.parametrize('N, nmu', cells.BATCH_CELLS + (cells.VALU_CELL, cells.SRC_CELL[:2]))
def test_batch_references_converge_and_every_mutant_is_separable(N, nmu):
    s = _reduced(cells.SWEEP, cells.NMAX)
    B, rhs = _cut(s, N)
    thetas = _thetas(s, nmu)
    cols = np.repeat(rhs.reshape(-1, 1), nmu, axis=1)
    th_b = c3.theta_of(s['p'], cells.BUILD_MU)
    assert np.abs(thetas - th_b).max(axis=1).min() > 1.0                   # the build parameter is away from every column
    means = r3.group_means(thetas)
    assert len({tuple(m) for m in means}) == len(means)                    # the group means differ
    plain = r3.reduced_batch(B, s['nbr'], thetas, cols)
    some = sorted({0, nmu // 2, nmu - 1})
    if nmu <= 17:
        _converges(plain, 27 * N, some)
    if nmu > 1:
        _separates(plain, r3.reduced_batch(B, s['nbr'], thetas, cols, blocks='own'), ('own', N, nmu))
    if nmu > r3.GROUP:
        _separates(plain, r3.reduced_batch(B, s['nbr'], thetas, cols, blocks='call'), ('call', N, nmu))
    inst = r3.reduced_batch(B, s['nbr'], thetas, cols, build_theta=th_b)
    if nmu <= 17:
        _converges(inst, 27 * N, some)
    for kw in (dict(coarse=None), dict(coarse='own'), dict(blocks='group')):
        _separates(inst, r3.reduced_batch(B, s['nbr'], thetas, cols, build_theta=th_b, **kw), (kw, N, nmu))


# ---------------------------------------------------------------------------------------- operators on the CPU: full order
def _fom(name):
    if name not in _FOM:
        p = c3.make_problem(name)
        o = c3.oracle_of(p)
        a = c3.oracle_assembled(p, o)
        t = p['grid'].template
        Aq = ref3.component_operators(a['A_diag'].reshape(a['A_diag'].shape[:4] + (100,)), a['A_cpl'].reshape(a['A_cpl'].shape[:4] + (100,)),
                                      t, p['grid'].neighbor_slots)
        _FOM[name] = (p, o, t, Aq, a['b'])
    return _FOM[name]


@pytest.mark.parametrize('name', sorted({name for name, _ in cells.FOM_CELLS}))
def test_fom_references_converge_and_every_mutant_is_separable(name):
    p, o, t, Aq, b = _fom(name)
    S, n = o.S, o.n
    th = c3.theta_of(p, p['mu'])
    spaces = [space for nm, space in cells.FOM_CELLS if nm == name]
    for space in spaces:
        Phi = cells._phi_of(t, space)
        cell = r3.fom_single(Aq, S, n, Phi, th, b, coarse=0 if space == 'off' else 1)
        assert cell.precond.has_coarse == (space in ('p1', 'constants'))
        lo, asym = pcg_ref.spd_check(pcg_ref.precond_matrix(cell.Ms[0], S * n)) if S * n <= 2000 else (1.0, 0.0)
        assert lo > 0.0 and asym < 1e-12, (space, lo, asym)
        for k in cells.K_STEPS:
            assert cell.iterate(k)[1].min() >= MIN_RATIO, (name, space, k)
        if space == 'p1':
            X, ratios = cell.iterate(400)
            want = o.solve(p['mu'])
            assert ratios.max() < 1e-12 and np.abs(X[:, 0] - want).max() < 1e-8 * np.abs(want).max()
        blocks = r3.fom_single(Aq, S, n, None, th, b)
        if cell.precond.has_coarse:
            _separates(cell, blocks, (name, space, 'no coarse'))
            _separates(cell, r3.fom_single(Aq, S, n, Phi, th, b, coarse_theta=c3.theta_of(p, cells.BUILD_MU)), (name, space, 'theta'))
            other = cells._phi_of(t, {'p1': 'constants', 'constants': 'p1'}[space])
            _separates(cell, r3.fom_single(Aq, S, n, other, th, b), (name, space, 'space'))
        else:
            assert r3.miss(cell.iterate(K2)[0], blocks.iterate(K2)[0]) == 0.0
            _separates(cell, r3.fom_single(Aq, S, n, ref3.default_phi(t), th, b), (name, space, 'p1'))


def test_kept_inverse_reference_is_separable_from_the_solves_own():
    name, mu_keep = cells.KEPT_CELL
    p, o, t, Aq, b = _fom(name)
    th = c3.theta_of(p, p['mu'])
    Phi = ref3.default_phi(t)
    cell = r3.fom_single(Aq, o.S, o.n, Phi, th, b, coarse_theta=c3.theta_of(p, mu_keep))
    for k in cells.K_STEPS:
        assert cell.iterate(k)[1].min() >= MIN_RATIO, k
    _separates(cell, r3.fom_single(Aq, o.S, o.n, Phi, th, b), 'kept')


def test_uncapped_mutant_is_the_dense_two_level_preconditioner():
    """``SparseCoarseFomPrecond3D`` (the P1 mutant of the capped grid) equals ``BatchFomPrecond3D`` below the cap."""
    p, o, t, Aq, b = _fom('q3_2x1x2')
    A = ref3.combine(Aq, c3.theta_of(p, p['mu']))
    Phi = ref3.default_phi(t)
    dense = ref3.BatchFomPrecond3D(A, A, o.S, o.n, Phi)
    sparse = r3.fom_precond(A, A, o.S, o.n, Phi, capped=False)
    assert isinstance(sparse, r3.SparseCoarseFomPrecond3D) and dense.has_coarse
    R = np.random.default_rng(0).standard_normal((o.S * o.n, 3))
    assert np.abs(sparse.apply(R) - dense.apply(R)).max() < 1e-12 * np.abs(dense.apply(R)).max()
    assert np.abs(sparse.apply(R[:, 0]) - dense.apply(R[:, 0])).max() < 1e-12 * np.abs(dense.apply(R)).max()


# ------------------------------------------------------------------------------------------------------ the Euler steps
@pytest.mark.parametrize('name', cells.EULER_PROBLEMS)
def test_euler_step_references_converge_and_every_mutant_is_separable(name):
    N = c3.PROBLEMS[name][5]
    s = _reduced(name, N)
    p, o = s['p'], s['o']
    th = c3.theta_of(p, p['mu'])
    dt = cells.DT
    # reduced
    u0 = cells._u0(np.abs(r3.reduced_single(s['B'], s['nbr'], th, s['rhs']).solve()).max(), (o.S, N))
    cell = r3.reduced_euler_step(s['B'], s['M'], s['nbr'], th, dt, s['rhs'], u0)
    assert 0.0 < cell.scale[0] and np.isfinite(cell.scale[0])
    X, ratios = cell.iterate(o.S * N)
    assert ratios.max() < 1e-12
    from parabolic_batch3d_ref import dense_euler
    want = dense_euler(s['B'], s['M'], s['nbr'], th, dt, 1, rhs=s['rhs'], U0=u0)[1].ravel()
    assert np.linalg.norm(u0.ravel() + X[:, 0] - want) < 1e-10 * np.linalg.norm(want)
    _separates(cell, r3.reduced_euler_step(s['B'], s['M'], s['nbr'], th, dt, s['rhs'], u0, mass_in_blocks=False), (name, 'reduced mass'))
    # full order
    _, _, t, Aq, b = _fom(name)
    mass = r3.oracle_mass(o)
    assert abs(mass - mass.T).max() <= 1e-14 * abs(mass).max() and abs(mass - o.M).max() == 0.0      # (the oracle numbers its DoFs [S][n])
    Phi = ref3.default_phi(t)
    v0 = cells._u0(np.abs(o.solve(p['mu'])).max(), (o.S, o.n))
    cell = r3.fom_euler_step(Aq, mass, o.S, o.n, Phi, th, dt, b, v0)
    assert cell.precond.has_coarse
    lo, asym = pcg_ref.spd_check(pcg_ref.precond_matrix(cell.Ms[0], o.S * o.n))
    assert lo > 0.0 and asym < 1e-12, (lo, asym)
    X, ratios = cell.iterate(600)
    assert ratios.max() < 1e-12
    from parabolic3d_ref import Parabolic3D
    want = Parabolic3D(o, dt, 1).solve(p['mu'], U0=v0)[1].ravel()
    assert np.abs(v0.ravel() + X[:, 0] - want).max() < 1e-8 * np.abs(want).max()
    _separates(cell, r3.fom_euler_step(Aq, mass, o.S, o.n, Phi, th, dt, b, v0, mass_in_blocks=False), (name, 'fom mass'))
    _separates(cell, r3.fom_euler_step(Aq, mass, o.S, o.n, Phi, th, dt, b, v0, coarse=0), (name, 'fom coarse'))
