"""What tests/test_parabolic_tv_dispatch_gpu.py relies on, shown without a GPU:

1. its cell tables reach every choice the host code of the three _tv drivers makes (restated here from online.hip / fom.hip, with a
   check that the restated lines still stand in the source): the group width, the k-steps of the panel matvec, the number of groups
   under both settings of LRBMS_OPT_SOLVE_VALU, the panels of the full-order driver, the uploads of the coefficient table in chunks
   of 256 doubles, the table slot [m][Q] of the mass coefficient for Q = 2 .. 4, both sides of the block inverse's LDS opt-in;
2. the references move by far more than the tolerances under the faults the cells are meant to catch: lost start values, row k in
   place of k + 1, a preconditioner at row 1 only or at the rows 0 .. nt (the iterates, by more than MUTANT_FLOOR + TOL_X), a
   coefficient table whose second chunk is lost or shifted;
3. a table that is constant in time reproduces ``parabolic_batch_ref.dense_euler_batch`` from the same start values.

The oracle's projection of the same kind of bases (``oracle_system`` of tests/test_parabolic_dispatch_host.py) stands in for the
product's projection on the GPU."""
import os

import numpy as np
import pytest

import parabolic_tv_ref as tv
import test_parabolic_tv_dispatch_gpu as g
from parabolic_batch_ref import column_errors, dense_euler_batch
from test_parabolic_batch_gpu import T_END, TOL_TRAJ
from test_parabolic_dispatch_host import cut, oracle_system
from test_parabolic_estimate_batch_gpu import TOL as TOL_EST
from test_pcg_iterates_gpu import MUTANT_FLOOR, TOL_X

FLOOR = 1e4                                   # x the tolerance of the cell: what a faulty reference must miss by
BMAX = 64                                     # widest group (online.hip)
CHUNK = 256                                   # doubles per k_pe_put launch (PeTable)


def _source(name):
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, '..', 'pylrbms_amd', 'csrc', name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------- 1. the host's choices
def group_width(nmu, valu=0):
    return 16 if valu or nmu <= 16 else 32 if nmu <= 32 else 64


def ksc_n(N):
    return 4 if N <= 16 else 8 if N <= 32 else 10 if N <= 40 else 12 if N <= 48 else 16


def groups(nmu, valu=0):
    GW = group_width(nmu, valu)
    return (nmu + GW - 1) // GW


def chunks(nmu, nt):
    nc = nmu * (nt + 1) * 2
    return [min(CHUNK, nc - c0) for c0 in range(0, nc, CHUNK)]


def inverse_lds(N):
    return 8 * 2 * N * (N | 1)


def test_the_cells_reach_every_choice_of_the_host():
    online, fom, dev = _source('online.hip'), _source('fom.hip'), _source('lrbms_dev.h')
    # the restated lines
    assert 'if (ctx->opt_solve_valu != 0 || nmu <= 16) return 16;' in online and 'return nmu <= 32 ? 32 : 64;' in online
    assert 'const int ksc_n = N <= 16 ? 4 : N <= 32 ? 8 : N <= 40 ? 10 : N <= 48 ? 12 : 16;' in online
    assert online.count('const int ng = (nmu + GW - 1) / GW;') >= 3 and 'BcgGroup g[4];' in online
    assert 'BMAX = {}'.format(BMAX) in online + dev
    # the reduced driver: width x k-steps of the wide panels, panels of 16 past N = 32, full groups
    reached = {(group_width(nmu), ksc_n(N)) for N, nmu in g.REDUCED_CELLS}
    assert reached >= {(32, 10), (64, 4), (64, 8), (64, 12), (64, 16)}
    assert {(group_width(nmu), ksc_n(N)) for N, nmu in g.SOURCE_CELLS} == {(32, 10), (64, 12)}
    assert sum(group_width(nmu) == 16 and N > 32 for N, nmu in g.REDUCED_CELLS) >= 2
    assert {nmu for _, nmu in g.REDUCED_CELLS if nmu == group_width(nmu)} == {16, 32, 64}
    assert g.RAGGED_CELL in g.REDUCED_CELLS and g.RAGGED_CELL[1] == group_width(g.RAGGED_CELL[1]) == 32
    assert all(groups(nmu) == 1 for _, nmu in g.REDUCED_CELLS + g.U0_CELLS + g.ITERATE_CELLS)
    assert {group_width(nmu) for _, nmu in g.U0_CELLS} == {16, 64} and {group_width(nmu) for _, nmu in g.ITERATE_CELLS} == {16, 32, 64}
    assert {g.nt_of(N, nmu) for N, nmu in g.REDUCED_CELLS} == {2, 3}
    # the VALU form: two, three (a partial last one) and four full groups, with the gather / scatter path (ng > 1); the wide
    # panels never run more than one group, so their table [group][step][BMAX][8] behind the twin's work is sized for the two
    # groups it reserves, and the panels of 16 read their table from the kernel arguments (G.th), never through theta_dev
    assert [(groups(nmu, 1), nmu % 16) for _, nmu, _ in g.VALU_CELLS] == [(2, 1), (3, 8), (4, 0)]
    assert all(groups(nmu, 1) == ng for _, nmu, ng in g.VALU_CELLS)
    assert all(groups(nmu) == 1 for nmu in range(1, 65)) and max(groups(nmu, 1) for nmu in range(1, 65)) == 4
    assert 'if (ng == 1) G.ug = un;' in online and 'if (ng > 1) {' in online
    assert 'reduced_implicit_euler_batch_work_size(ctx, N, nmu) + 2L * nt * 8 * BMAX;' in online
    assert 'if (tv && GW > 16) {' in online and 'if (step == 0 && GW > 16)' in online
    assert 'k_bcg_matvec_mfma<16, MASS>), dim3(S), dim3(256), P.lds_mfma, G.st, S, ctx->nbr, Q, N, G.nm, G.th, op.B_sys' in online
    assert {N * 16 <= 768 for N, _, _ in g.VALU_CELLS} == {True, False}            # k_bcg_matvec<3> and <BCG_KMAX>
    assert '} else if (NM <= 768) {' in online
    # Q: the coefficient of M_red sits at slot [m][Q] of the wide panels' table; Q = 2 .. 4 there, Q = 8 on panels of 16
    assert '(P.mass && m < G.nm && q == Q) ? 1.0 : 0.0' in online
    assert 'if (nmu > 16 && Q > 4)' in online
    wide = {Q for Q, nmu, _ in g.Q_CELLS if nmu > 16} | {2}
    assert wide == {2, 3, 4} and {(Q, group_width(nmu)) for Q, nmu, _ in g.Q_CELLS} == {(3, 32), (4, 64), (8, 16)}
    assert {ksc_n(N) for _, _, N in g.Q_CELLS} == {8, 10} and max(N for _, _, N in g.Q_CELLS) <= g.Q_NB
    # the block inverse of the step operator (reduced driver) and of M_red (estimate driver): 64 KB crossed between 63 and 64
    assert 'sizeof(double) * 2 * N * (N | 1)' in online and 'if (lds > 64 * 1024)' in online
    assert 'launch_block_inverse(ctx, (int)S, N, Amu, Dinv, 5, 2, st)' in online
    assert 'launch_block_inverse(ctx, S, N, M_red, Minv, 1, 0, st)' in online
    assert inverse_lds(63) <= 64 * 1024 < inverse_lds(64)
    for sizes in ({N for N, _ in g.REDUCED_CELLS}, {N for N, _, _ in g.EST_CELLS} | {63}):
        assert {63, 64} <= sizes
    assert any(N < 64 for N, _, _ in g.EST_CELLS)
    # the full-order driver: panels of 16, the table rewritten per step inside the panel loop
    assert 'for (int m0 = 0; m0 < nmu; m0 += 16) {' in fom
    assert 'op.th.v[c][q] = dt * theta[(m0 + c) * th_ld + (long)(step + 1) * Q + q];' in fom
    assert [((nmu + 15) // 16, (nmu - 1) % 16 + 1) for nmu in g.FOM_PANELS] == [(3, 1), (4, 1), (4, 16)]
    assert [(nmu + 15) // 16 for nmu in g.FOM_ITERATE_NMU] == [1, 2, 3]
    # the estimate driver: coef [nmu][nt + 1][2] goes up in chunks of 256 doubles
    assert 'const long nc = (long)nmu * (nt + 1) * 2;' in online and 'for (long c0 = 0; c0 < nc; c0 += 256) {' in online
    assert 'struct PeTable { double v[256]; };' in online and 'for (int i = 0; i < 256; ++i) t.v[i] = i < n ? coef[c0 + i] : 0.0;' in online
    assert [chunks(nmu, nt) for _, nmu, nt in g.EST_CELLS] == [[96], [256, 8], [256, 234], [256, 256]]
    assert {(group_width(nmu), ksc_n(N)) for N, nmu, _ in g.EST_CELLS} == {(16, 10), (64, 10), (64, 12), (64, 16)}
    assert set(g.EST_BOTH_LAYOUTS) <= set(g.EST_CELLS) and g.EST_MAIN in g.EST_CELLS
    assert groups(g.EST_MAIN[1], 1) == 3                                    # solve_valu = 1: three groups of the time residual
    # the elliptic rows: the VALU form only with LRBMS_OPT_ESTIMATE_VALU and the dense layout (no F_side), the cell that sets the
    # option is dense and its coefficient panels fit the LDS; solve_valu moves the time residual's matvec to groups of 16
    assert 'if (Fside != nullptr || ctx->opt_estimate_valu == 0) {' in online
    assert 'lds > 160 * 1024 || ((Fside != nullptr || ctx->opt_estimate_valu == 0) && ldm > 160 * 1024)' in online
    assert 'hipLaunchKernelGGL(k_reduced_estimate_batch, dim3(ctx->S), dim3(256), lds, st' in online
    assert g.EST_VALU_LAYOUT == {'solve_valu': 'factored', 'estimate_valu': 'dense'}
    assert 8 * ((5 * g.EST_MAIN[0] + 5 * 2 * g.EST_MAIN[0]) * 16 + 8 * 16 + 4 * 3 * 16) <= 160 * 1024
    assert 'put_cols(theta + (long)k * Q);' in online                      # the source branch, one slab per launch
    assert {Q for Q, _ in g.EST_Q_CELLS} == {4, 8} and all(nmu <= 16 or Q <= 4 for Q, nmu in g.EST_Q_CELLS)
    # Python: chunks of 64 parameters
    here = os.path.dirname(os.path.abspath(__file__))
    for name, count in (('reductor.py', 2), ('discretize_parabolic_block_swipdg.py', 1)):
        with open(os.path.join(here, '..', 'pylrbms_amd', name)) as f:
            assert f.read().count('in range(0, len(mus), 64):') >= count, name


# --------------------------------------------------------------------------------------------------- 2. the faults, per cell
def _reduced(N, nmu, nt, with_U0=False):
    s = oracle_system()
    B, M, rhs = cut(N)
    th = g.tables(nmu, nt, seed=N + nmu)
    U0 = g.start_values(B, M, rhs, s['nbr'], th[0, 1], nmu) if with_U0 else None
    return s['nbr'], B, M, rhs, th, U0


@pytest.mark.parametrize('N, nmu', g.U0_CELLS)
def test_lost_start_values_miss(N, nmu):
    nt, cols = 3, 4                                                         # (the first columns: every column has its own U0)
    nbr, B, M, rhs, th, U0 = _reduced(N, nmu, nt, with_U0=True)
    th, U0 = th[:cols], U0[..., :cols]
    right = tv.dense_euler_batch_tv(B, M, nbr, th, T_END / nt, nt, rhs=rhs, U0=U0)
    assert np.array_equal(right[0], U0)
    wrong = tv.dense_euler_batch_tv(B, M, nbr, th, T_END / nt, nt, rhs=rhs)
    miss = column_errors(wrong, right)
    print('U0 dropped N={}: misses by {:.2e} .. {:.2e}'.format(N, float(miss.min()), float(miss.max())))
    assert miss.min() > FLOOR * TOL_TRAJ                                    # every step of every column


@pytest.mark.parametrize('N, nmu', [c for c in g.REDUCED_CELLS if c[0] == 40])
def test_row_k_in_place_of_row_k_plus_one_misses(N, nmu):
    nt = g.nt_of(N, nmu)
    nbr, B, M, rhs, th, _ = _reduced(N, nmu, nt)
    for m in sorted({0, nmu // 2, nmu - 1}):
        right = tv.dense_euler_tv(B, M, nbr, th[m], T_END / nt, nt, rhs=rhs)
        wrong = tv.dense_euler_tv(B, M, nbr, th[m], T_END / nt, nt, rhs=rhs, rows=th[m, :-1])
        miss = column_errors(wrong[..., None], right[..., None])
        print('row k for k + 1 N={} column {}: misses by {}'.format(N, m, miss.ravel()))
        assert miss[1:].min() > FLOOR * TOL_TRAJ                            # from the step across the switch on


@pytest.mark.parametrize('N, nmu', g.ITERATE_CELLS)
def test_a_preconditioner_at_other_rows_moves_the_second_iterate(N, nmu):
    """x_2 of the reference PCG with the preconditioner at row 1 only, and at the rows 0 .. nt, against the one at the rows 1 .. nt:
    more than MUTANT_FLOOR + TOL_X apart, so a device that passes ``check_iterates`` at TOL_X misses both by more than MUTANT_FLOOR."""
    s = oracle_system()
    B, M, rhs = cut(N)
    variants = [dict()] + ([dict(K=3), dict(with_U0=True)] if (N, nmu) == g.ITERATE_EXTRA else [])
    for kw in variants:
        inp = g.iterate_inputs(B, M, rhs, s['nbr'], nmu, **kw)
        th = inp['th']
        assert th.shape == (nmu, g.ITERATE_NT + 1, 2) and np.abs(th[:, 2, 1] / th[:, 1, 1]).max() < 0.5      # the switch lies between
        ref, P = g.iterate_reference(B, M, s['nbr'], inp)
        assert P.has_coarse
        x2, ratio = ref(2)
        assert ratio.min() > 1e-6                                           # k = 2 is inside check_iterates' range
        for what, pc in (('row 1 only', tv.step_mean(th, last=1)), ('the rows 0 .. nt', tv.step_mean(th, first=0))):
            y2, _ = g.iterate_reference(B, M, s['nbr'], inp, pc_theta=pc)[0](2)
            miss = float((np.linalg.norm(y2 - x2, axis=0) / np.linalg.norm(x2, axis=0)).max())
            print('x_2 N={} nmu={} {} misses by {:.2e} with the preconditioner at {}'.format(N, nmu, kw, miss, what))
            assert miss > MUTANT_FLOOR + TOL_X and MUTANT_FLOOR == FLOOR * TOL_X, (what, miss)


@pytest.mark.parametrize('N, nmu, nt', [c for c in g.EST_CELLS if len(chunks(c[1], c[2])) > 1])
def test_a_lost_or_shifted_second_chunk_of_the_coefficient_table_misses(N, nmu, nt):
    S = oracle_system()['nbr'].shape[0]
    rng = np.random.default_rng(N)
    raw, tr2, ncd = rng.uniform(0.1, 1.0, (3, nt + 1, S, nmu)), rng.uniform(0.1, 1.0, (nt, S, nmu)), rng.uniform(0.1, 1.0, (nt, S, nmu))
    coef = g._coef(nmu, nt)
    flat = coef.ravel()
    assert flat.size == sum(chunks(nmu, nt)) > CHUNK
    right = tv.combine_tv(raw, tr2, ncd, coef, T_END / nt)
    end = min(2 * CHUNK, flat.size)
    zero, shifted = flat.copy(), flat.copy()
    zero[CHUNK:end] = 0.0
    shifted[CHUNK:end] = flat[CHUNK - 1:end - 1]
    first = CHUNK // (2 * (nt + 1))                                         # the columns in front of it are untouched
    for what, table in (('zero', zero), ('shifted by one', shifted)):
        wrong = tv.combine_tv(raw, tr2, ncd, table.reshape(coef.shape), T_END / nt)
        assert np.array_equal(wrong['est'][:first], right['est'][:first])
        for k in ('eta', 'est'):
            miss = float((np.abs(wrong[k] - right[k]) / np.abs(right[k]).max()).max())
            print('coef chunk {} N={} nmu={} nt={}: {} misses by {:.2e}'.format(what, N, nmu, nt, k, miss))
            assert miss > FLOOR * TOL_EST, (what, k, miss)


# ------------------------------------------------------------------------------------------------ 3. a table constant in time
@pytest.mark.parametrize('N, nmu', g.U0_CELLS)
def test_a_constant_table_with_start_values_is_the_existing_reference(N, nmu):
    nt, cols = 3, 3
    nbr, B, M, rhs, th, U0 = _reduced(N, nmu, nt, with_U0=True)
    thetas = np.ascontiguousarray(th[:cols, 1])
    const = np.ascontiguousarray(np.repeat(thetas[:, None, :], nt + 1, axis=1))
    a = tv.dense_euler_batch_tv(B, M, nbr, const, T_END / nt, nt, rhs=rhs, U0=U0[..., :cols])
    b = dense_euler_batch(B, M, nbr, thetas, T_END / nt, nt, rhs=rhs, U0=U0[..., :cols])
    assert np.array_equal(a[0], U0[..., :cols]) and np.abs(a - b).max() <= 1e-13 * np.abs(b).max()
