"""k_f1w (f1_form 0) runs the third row tile (rows 32 .. N - 1) of its class-3 column tiles on the 4x4x4 f64 MFMA: two
instructions per k-step, rows 32 .. 35 and 36 .. 39.  The rows >= 32 of every array those tiles hold are compared apart from
the rows < 32, at the N where the tail can go wrong: 34 (two live rows, the second instruction all padding), 36 (the boundary
between the two instructions), 38 and 40.  Reference: k_f1u (f1_form 2) at the bound of test_f1w_forms_gpu.py, and the oracle
through common.compare_all at the tolerance of test_parity_gpu.py.  Every output is NaN before every pass."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from common import compare_all, energy_orthonormalize, make_bases, oracle_from_problem, theta_bar_of  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 1e-12            # k_f1w against k_f1u and K-split against K-split (test_f1w_forms_gpu.py)
ORACLE_TOL = 1e-11     # common.compare_all (test_parity_gpu.py)
GRIDS = [((2, 2), 2), ((3, 2), 4)]
SYS = ('B_sys', 'rhs_red', 'E_red', 'M_red')
FACTORED = ('G_nc_self', 'r_fd', 'G_rdd_self', 'G_bb_self', 'G_ab_self', 'G_aa', 'F_side', 'F_nc')
DENSE = ('G_nc', 'r_fd', 'G_rdd', 'G_bb', 'G_ab', 'G_aa')


@functools.lru_cache(maxsize=None)
def _setup(shape, kc):
    from pylrbms_amd import multiscale_problem
    from pylrbms_amd.engine import Engine
    p = multiscale_problem.init_grid_and_problem({'num_subdomains': list(shape), 'coarse_per_subdomain': kc})
    lam = p['lambda']
    eng = Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar_of(p)).assemble()
    assert eng.Q == 2
    return p, eng


@functools.lru_cache(maxsize=None)
def _oracle(shape, kc):
    return oracle_from_problem(_setup(shape, kc)[0])


def _pass(eng, V, N, form, ks=0, factored=None, buf=None, subset=None):
    """One pass with every output NaN before it (a subset pass: the rows of the subset that k_f1w writes); {name: clone}."""
    import torch
    eng.ctx.set_option('f1_form', form)
    eng.ctx.set_option('f1_ksplit', ks)
    if buf is None:
        buf = eng.alloc_reduce_buffers(N, factored=factored)
    names = SYS + (FACTORED if len(buf['grams']) == 8 else DENSE)
    out = dict(zip(names, list(buf['sys']) + list(buf['grams'])))
    if subset is None:
        for x in out.values():
            x.fill_(float('nan'))
    else:
        idx = torch.as_tensor(subset, device=out['E_red'].device)
        out['B_sys'][:, idx, 2] = float('nan')
        out['E_red'][idx] = float('nan')
        out['M_red'][idx] = float('nan')
        out['G_ab_self'][:, idx] = float('nan')
        out['G_aa'][:, :, idx] = float('nan')
    eng.ctx.kernel_timing(True)
    eng.project_and_estimate(V, buf, subset=subset)
    ran = {k for k, _ in eng.ctx.kernel_timing_read()}
    eng.ctx.kernel_timing(False)
    assert ('k_f1w' if form == 0 else 'k_f1u') in ran, (form, ks, sorted(ran))
    return buf, {k: x.clone() for k, x in out.items()}


def _reset(eng):
    eng.ctx.set_option('f1_form', 0)
    eng.ctx.set_option('f1_ksplit', 0)


def _tail_views(out, N, Q=2):
    """{label: (head, tail)} for every array k_f1w holds in class-3 tiles; the same call on the reference gives the same views.
    Rectangular groups (G_ab self blocks, G_aa[0][1] and the transpose the kernel writes with it): rows < 32 / rows >= 32.
    Symmetric groups (B_sys diagonal, E_red, M_red, G_aa[q][q]; delivered as row <= column plus the mirror image): the block
    of rows and columns < 32 / everything with a row or a column >= 32 (the packed tails and their mirrored columns)."""
    v = {}
    gab = out['G_ab_self'] if 'G_ab_self' in out else out['G_ab'][..., 2 * Q * N:3 * Q * N]      # dense: the self slot's columns
    for q in range(Q):
        for q2 in range(Q):
            x = gab[q][:, :, q2 * N:(q2 + 1) * N]
            v['G_ab[{}] self, q2 = {}'.format(q, q2)] = (x[:, :32], x[:, 32:])
    v['G_aa[0][1]'] = (out['G_aa'][0, 1][:, :32], out['G_aa'][0, 1][:, 32:])
    v['G_aa[1][0] (transpose)'] = (out['G_aa'][1, 0][:, :, :32], out['G_aa'][1, 0][:, :, 32:])
    sym = {'E_red': out['E_red'], 'M_red': out['M_red']}
    for q in range(Q):
        sym['B_sys[{}] diagonal'.format(q)] = out['B_sys'][q][:, 2]
        sym['G_aa[{0}][{0}]'.format(q)] = out['G_aa'][q, q]
    for k, x in sym.items():
        v[k] = (x[:, :32, :32], x[:, 32:, :])
        v[k + ' (mirrored columns)'] = (x[:, :32, :32], x[:, :, 32:])
    return v


def _check_against(ref, got, N, tag):
    import torch
    for k in ref:
        assert bool(torch.isfinite(got[k]).all()), (tag, k)
        assert float((ref[k] - got[k]).abs().max()) <= REL * float(ref[k].abs().max()), (tag, k)
    rv, gv = _tail_views(ref, N), _tail_views(got, N)
    for k in rv:
        scale = max(float(rv[k][0].abs().max()), float(rv[k][1].abs().max()))
        assert (N - 32) in tuple(gv[k][1].shape[-2:]) and gv[k][1].shape == rv[k][1].shape, (tag, k)
        assert float((rv[k][0] - gv[k][0]).abs().max()) <= REL * scale, (tag, k, 'rows < 32')
        assert float((rv[k][1] - gv[k][1]).abs().max()) <= REL * scale, (tag, k, 'rows 32 .. N - 1')
        # a swap of the groups 32 .. 35 / 36 .. 39 or a dropped instruction is an error of the size of the entries themselves:
        assert float(rv[k][1].abs().max()) > 1e3 * REL * scale, (tag, k, 'the tail rows of the reference are not trivial')


@pytest.mark.parametrize('N', [34, 36, 38, 40])
@pytest.mark.parametrize('shape, kc', GRIDS)
def test_tail_rows_against_k_f1u_and_the_oracle(shape, kc, N):
    p, eng = _setup(shape, kc)
    d = _oracle(shape, kc)
    V = make_bases(eng.S, eng.t.n, N, seed=29)
    Vd = eng.ctx.from_numpy(V)
    try:
        _, ref = _pass(eng, Vd, N, 2, 1)
        _, got = _pass(eng, Vd, N, 0)
        _check_against(ref, got, N, 'k_f1w against k_f1u')
    finally:
        _reset(eng)
    # the oracle: compare_all runs the unfused kernels against the oracle's reductor and the fused pass (k_f1w at this shape,
    # factored and dense layout) against the unfused kernels
    res = compare_all(p, eng, energy_orthonormalize(V, d), 0.4, do_solve=False, oracle=d)
    assert 'fused_G_ab' in res and 'fused_dense_G_ab' in res
    bad = {k: v for k, v in res.items() if not v < ORACLE_TOL}
    assert not bad, bad


@pytest.mark.parametrize('shape, kc, N', [((2, 2), 2, 36), ((2, 2), 2, 40), ((3, 2), 4, 34), ((3, 2), 4, 38)])
def test_ksplits_agree_and_repeat(shape, kc, N):
    import torch
    _, eng = _setup(shape, kc)
    Vd = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=31))
    try:
        outs = {}
        for ks in (1, 2, 4):
            buf, outs[ks] = _pass(eng, Vd, N, 0, ks)
            _, again = _pass(eng, Vd, N, 0, ks, buf=buf)
            for k in outs[ks]:
                assert bool(torch.isfinite(outs[ks][k]).all()), (ks, k)
                assert torch.equal(outs[ks][k], again[k]), (ks, k)
        for ks in (2, 4):
            _check_against(outs[1], outs[ks], N, 'K-split {} against 1'.format(ks))
        _check_against(outs[2], outs[4], N, 'K-split 4 against 2')
    finally:
        _reset(eng)


def test_dense_layout_tail_rows():
    """The dense layout's wider G_ab rows ([N, 5 Q N], the self slot in the middle) go through the same epilogue."""
    N = 40
    _, eng = _setup((2, 2), 2)
    Vd = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=37))
    try:
        _, ref = _pass(eng, Vd, N, 2, 1, factored=False)
        _, got = _pass(eng, Vd, N, 0, factored=False)
        assert tuple(got['G_ab'].shape) == (2, eng.S, N, 5 * 2 * N)
        _check_against(ref, got, N, 'dense layout')
    finally:
        _reset(eng)


def test_subset_pass_leaves_every_row_as_the_whole_pass_wrote_it():
    import torch
    N = 38
    _, eng = _setup((3, 2), 4)
    Vd = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=41))
    try:
        buf, whole = _pass(eng, Vd, N, 0)
        subset = list(range(0, eng.S, 2))
        assert 0 < len(subset) == eng.S // 2
        _, after = _pass(eng, Vd, N, 0, buf=buf, subset=subset)
        for k in whole:
            assert torch.equal(whole[k], after[k]), k
    finally:
        _reset(eng)


def test_mfma_count_prices_the_small_shape():
    """lrbms_fused_mfma_per_subdomain in units of one 16x16x4 (2 048 flop); a 4x4x4_4b is a quarter unit."""
    _, eng = _setup((3, 2), 4)
    assert eng.t.n_T == 128
    chunks = 128 // 4                       # four elements per chunk
    # projection: 150 k-steps per chunk, 34 of them (third row tile of the class-3 column tiles) as two quarter units each
    per_chunk = 150 - 34 + 17
    role_a_apply = 128 * 3 * 3              # three k-steps x three column tiles per element
    role_b_apply = 128 * 5 // 4             # five quarter units per element
    assert per_chunk == 133 and chunks * per_chunk + role_a_apply + role_b_apply == 5568
    assert eng.ctx.fused_mfma_per_subdomain(2, 40) == 5568
