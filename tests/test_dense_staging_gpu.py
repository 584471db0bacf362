"""Staging of the dense kernels of the fused pass -- runs on the MI355X box (`-m gpu`).

k_f1w (f1_form 0) does not stage the c^{qq'} Z V rows of the three G_aa groups: role A stores Z V once and the element's three
scalars into a small table, and the consumer of a G_aa tile multiplies the Z V fragment with the scalar of the K row's element
and of the column's group where it reads it; the G_ab columns moved up to the tile boundary behind G_aa[0][1].  With the
assembled c^{qq'} a swapped pair, a wrong element or a wrong table parity can hide (the pairs are multiples of one field), so
G_aa is checked with scalars that can be told apart -- random, per element and per pair -- against k_f1u (f1_form 2) at the bound
of test_f1w_forms_gpu.py, per pair and per column block; every other output of the kernel at the same bound; the K-splits; the
dense layout; a subset pass; and the oracle through common.compare_all at the tolerance of test_parity_gpu.py.

k_f2g (f2_form 0) stages its flux rows with producers that own adjacent column pairs wherever Q N is even: 16-byte loads and
LDS stores, the per-column expressions of the one-column producers.  f2_form 2 runs the one-column producers on the same inputs
(odd Q N runs them in form 0 as well), so every output of the pass has to be the same bits in both forms -- at config 3's shape,
with all 64 lanes owning a pair (Q N = 128), with one row tile, and where a pair straddles the boundary between the two
components (N odd, Q N even).  Every output is NaN before every pass."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from common import (compare_all, energy_orthonormalize, make_bases, oracle_from_problem, problem_with_q_components,  # noqa: E402
                    theta_bar_of)

pytestmark = pytest.mark.gpu

SYS = ('B_sys', 'rhs_red', 'E_red', 'M_red')
FACTORED = ('G_nc_self', 'r_fd', 'G_rdd_self', 'G_bb_self', 'G_ab_self', 'G_aa', 'F_side', 'F_nc')
DENSE = ('G_nc', 'r_fd', 'G_rdd', 'G_bb', 'G_ab', 'G_aa')


@functools.lru_cache(maxsize=None)
def _setup(Q, shape, kc):
    from pylrbms_amd.engine import Engine
    if Q == 2:
        from pylrbms_amd import multiscale_problem
        p = multiscale_problem.init_grid_and_problem({'num_subdomains': list(shape), 'coarse_per_subdomain': kc})
    else:
        p = problem_with_q_components(shape, kc, Q)
    lam = p['lambda']
    eng = Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar_of(p)).assemble()
    assert eng.Q == Q and eng.t.n_T % 8 == 0
    return eng


def _pass_f2(eng, V, N, f2_form, factored):
    """One pass with every output NaN before it; {name: clone}."""
    eng.ctx.set_option('f2_form', f2_form)
    try:
        buf = eng.alloc_reduce_buffers(N, factored=factored)
        names = SYS + (FACTORED if len(buf['grams']) == 8 else DENSE)
        out = dict(zip(names, list(buf['sys']) + list(buf['grams'])))
        for x in out.values():
            x.fill_(float('nan'))
        eng.ctx.kernel_timing(True)
        eng.project_and_estimate(V, buf)
        ran = {k for k, _ in eng.ctx.kernel_timing_read()}
        eng.ctx.kernel_timing(False)
        assert 'k_f2' in ran, (f2_form, sorted(ran))
        return {k: x.clone() for k, x in out.items()}
    finally:
        eng.ctx.set_option('f2_form', 0)


def _same_bits(eng, Q, N, factored, seed):
    import torch
    assert eng.ctx.fused_supported(Q, N, factored=factored)
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=seed))
    pairs = _pass_f2(eng, V, N, 0, factored)
    single = _pass_f2(eng, V, N, 2, factored)
    for k in single:
        assert bool(torch.isfinite(single[k]).all()), k
        assert torch.equal(pairs[k], single[k]), k
    # the arrays k_f2g writes are not trivial, and the product form k_f2 (f2_form 1) is a different kernel: same numbers to rounding
    prod = _pass_f2(eng, V, N, 1, factored)
    for k in ('G_bb_self', 'G_rdd_self') if factored else ('G_bb', 'G_rdd'):
        scale = float(prod[k].abs().max())
        assert scale > 0.0 and float((prod[k] - pairs[k]).abs().max()) <= 1e-13 * scale, k
    assert float(pairs['r_fd'].abs().max()) > 0.0 and torch.equal(prod['r_fd'], pairs['r_fd'])


# (N, subdomains, k_c) at Q = 2: Q N = 80 (config 3's kernel, 40 of 64 lanes own a pair), 68, 40, 128 (all 64 lanes), 16 (one row
# tile), 66 (N odd: the pair of lane 16 holds column 32 of component 0 and column 0 of component 1)
EVEN = [(40, (3, 2), 4), (34, (2, 2), 2), (20, (2, 2), 2), (64, (3, 2), 4), (8, (2, 2), 2), (33, (3, 2), 4)]


@pytest.mark.parametrize('factored', [True, False], ids=['factored', 'dense'])
@pytest.mark.parametrize('N, shape, kc', EVEN)
def test_pair_and_one_column_producers_give_the_same_bits(N, shape, kc, factored):
    _same_bits(_setup(2, shape, kc), 2, N, factored, seed=43)


@pytest.mark.parametrize('Q, N', [(3, 37), (1, 17)])
def test_odd_qn_runs_the_one_column_producers_in_both_forms(Q, N):
    _same_bits(_setup(Q, (3, 2), 2), Q, N, True, seed=47)


def test_non_spd_flux_mass_gives_a_non_finite_g_bb_with_pair_producers():
    """As test_f2_gram_gpu.py: a Bbb block that is not SPD gives the subdomain that holds it a NaN G_bb[self, self]; every other
    subdomain keeps the bits of the unpoisoned pass."""
    import torch
    N = 40
    eng = _setup(2, (3, 2), 4)
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=9))
    good = _pass_f2(eng, V, N, 0, True)
    keep = eng.Bbb
    try:
        Bbb = keep.clone()
        B4 = Bbb.view(eng.S, -1, 3, 3)
        s0, T0 = eng.S // 2, B4.shape[1] // 3
        B4[s0, T0, 1, 1] = -B4[s0, T0, 1, 1]           # pivot 1 of the Cholesky factor < 0
        eng.Bbb = Bbb
        eng.__dict__.pop('_bound_pass', None)
        bad = _pass_f2(eng, V, N, 0, True)
    finally:
        eng.Bbb = keep
        eng.__dict__.pop('_bound_pass', None)
    assert bool(torch.isnan(bad['G_bb_self'][s0]).all())
    others = [s for s in range(eng.S) if s != s0]
    assert torch.equal(bad['G_bb_self'][others], good['G_bb_self'][others])
    assert np.isfinite(float(good['G_bb_self'].abs().max()))


# ---------------------------------------------------------------------------------------------------------- k_f1w
REL = 1e-12            # k_f1w against k_f1u and K-split against K-split (test_f1w_forms_gpu.py)
ORACLE_TOL = 1e-11     # common.compare_all (test_parity_gpu.py)
GRIDS = [((2, 2), 2), ((3, 2), 4)]


@functools.lru_cache(maxsize=None)
def _problem(shape, kc):
    from pylrbms_amd import multiscale_problem
    return multiscale_problem.init_grid_and_problem({'num_subdomains': list(shape), 'coarse_per_subdomain': kc})


@functools.lru_cache(maxsize=None)
def _oracle(shape, kc):
    return oracle_from_problem(_problem(shape, kc))


class _distinct_caa:
    """eng.caa replaced by positive random scalars that vary with the element and differ between the pairs; [0][1] mirrored into
    [1][0] (k_f1u reads the latter, k_f1w writes the transpose of the former)."""

    def __init__(self, eng, seed):
        self.eng, self.seed = eng, seed

    def __enter__(self):
        eng = self.eng
        self.keep = eng.caa
        assert eng.caa.numel() == 4 * eng.S * eng.t.n_T
        c = np.random.default_rng(self.seed).uniform(0.5, 2.0, size=(2, 2, eng.S, eng.t.n_T)) * np.array([1.0, 3.0, 3.0, 7.0]).reshape(2, 2, 1, 1)
        c[1, 0] = c[0, 1]
        eng.caa = eng.ctx.from_numpy(c.reshape(tuple(self.keep.shape)))
        eng.__dict__.pop('_bound_pass', None)
        return c

    def __exit__(self, *exc):
        self.eng.caa = self.keep
        self.eng.__dict__.pop('_bound_pass', None)
        self.eng.ctx.set_option('f1_form', 0)
        self.eng.ctx.set_option('f1_ksplit', 0)


def _pass_f1(eng, V, N, form, ks=0, factored=None, buf=None, subset=None):
    """One pass with every output NaN before it (a subset pass: the rows of the subset that k_f1w writes); buffers, {name: clone}."""
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


def _gaa_blocks(out, N):
    """{label: block} of G_aa per pair and per column block of the kernel's tiles (columns < 16, 16 .. 31, >= 32; of the transpose
    G_aa[1][0] that k_f1w writes beside G_aa[0][1]: the rows)."""
    G, v = out['G_aa'], {}
    for lo, hi in ((0, 16), (16, 32), (32, N)):
        for q, q2 in ((0, 0), (1, 1), (0, 1)):
            v['G_aa[{}][{}] columns {} .. {}'.format(q, q2, lo, hi - 1)] = G[q, q2][:, :, lo:hi]
        v['G_aa[1][0] rows {} .. {}'.format(lo, hi - 1)] = G[1, 0][:, lo:hi, :]
    return v


def _check_f1(ref, got, N, tag):
    """Every output of the pass at REL of its own scale (k_f1w's: the B_sys diagonal, E_red, M_red, G_ab_self, rhs_red, G_aa);
    then the G_aa blocks, each non-trivial in the reference."""
    import torch
    for k in ref:
        assert bool(torch.isfinite(got[k]).all()), (tag, k)
        assert float((ref[k] - got[k]).abs().max()) <= REL * float(ref[k].abs().max()), (tag, k)
    diag_r, diag_g = ref['B_sys'][:, :, 2], got['B_sys'][:, :, 2]
    assert float(diag_r.abs().max()) > 0.0 and float((diag_r - diag_g).abs().max()) <= REL * float(diag_r.abs().max()), (tag, 'B_sys diagonal')
    rb, gb = _gaa_blocks(ref, N), _gaa_blocks(got, N)
    scale = float(ref['G_aa'].abs().max())
    for k in rb:
        assert rb[k].shape == gb[k].shape and (N - 32 if '32' in k else 16) in tuple(rb[k].shape[-2:]), (tag, k)
        assert float((rb[k] - gb[k]).abs().max()) <= REL * scale, (tag, k)
        assert float(rb[k].abs().max()) > 1e3 * REL * scale, (tag, k, 'the block of the reference is not trivial')
    assert torch.equal(got['G_aa'][1, 0], got['G_aa'][0, 1].transpose(1, 2)), (tag, 'G_aa[1][0] is the transpose of G_aa[0][1]')


@pytest.mark.parametrize('N', [34, 36, 38, 40])
@pytest.mark.parametrize('shape, kc', GRIDS)
def test_g_aa_with_scalars_that_can_be_told_apart(shape, kc, N):
    eng = _setup(2, shape, kc)
    Vd = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=53))
    with _distinct_caa(eng, seed=59) as c:
        assert float(np.abs(c[0, 0] - c[1, 1]).min()) > 0.0 and float(np.abs(c[0, 0] - c[0, 1]).min()) > 0.0
        _, ref = _pass_f1(eng, Vd, N, 2, 1)
        _, got = _pass_f1(eng, Vd, N, 0)
        _check_f1(ref, got, N, 'k_f1w against k_f1u')
        # the three pairs differ by more than the bound in the reference: a swapped pair cannot pass
        G = ref['G_aa']
        for x, y in ((G[0, 0], G[1, 1]), (G[0, 0], G[0, 1]), (G[1, 1], G[0, 1])):
            assert float((x - y).abs().max()) > 1e6 * REL * float(G.abs().max())


@pytest.mark.parametrize('shape, kc, N', [((2, 2), 2, 34), ((3, 2), 4, 40)])
def test_ksplits_agree_and_repeat_with_distinct_scalars(shape, kc, N):
    import torch
    eng = _setup(2, shape, kc)
    Vd = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=61))
    with _distinct_caa(eng, seed=67):
        outs = {}
        for ks in (1, 2, 4):
            buf, outs[ks] = _pass_f1(eng, Vd, N, 0, ks)
            _, again = _pass_f1(eng, Vd, N, 0, ks, buf=buf)
            for k in outs[ks]:
                assert torch.equal(outs[ks][k], again[k]), (ks, k)
        for ks in (2, 4):
            _check_f1(outs[1], outs[ks], N, 'K-split {} against 1'.format(ks))


@pytest.mark.parametrize('N', [34, 40])
def test_dense_layout_with_distinct_scalars(N):
    """The dense layout's wider G_ab rows ([N, 5 Q N], the self slot in the middle) go through the same epilogue."""
    eng = _setup(2, (2, 2), 2)
    Vd = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=71))
    with _distinct_caa(eng, seed=73):
        _, ref = _pass_f1(eng, Vd, N, 2, 1, factored=False)
        _, got = _pass_f1(eng, Vd, N, 0, factored=False)
        assert tuple(got['G_ab'].shape) == (2, eng.S, N, 5 * 2 * N)
        _check_f1(ref, got, N, 'dense layout')
        _, split = _pass_f1(eng, Vd, N, 0, 2, factored=False)
        _check_f1(got, split, N, 'dense layout, K-split 2')


def test_subset_pass_leaves_every_row_as_the_whole_pass_wrote_it():
    import torch
    N = 38
    eng = _setup(2, (3, 2), 4)
    Vd = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=79))
    with _distinct_caa(eng, seed=83):
        buf, whole = _pass_f1(eng, Vd, N, 0)
        subset = list(range(0, eng.S, 2))
        assert 0 < len(subset) == eng.S // 2
        _, after = _pass_f1(eng, Vd, N, 0, buf=buf, subset=subset)
        for k in whole:
            assert torch.equal(whole[k], after[k]), k


@pytest.mark.parametrize('shape, kc, N', [((3, 2), 4, 40), ((2, 2), 2, 34)])
def test_the_oracle_with_the_assembled_scalars(shape, kc, N):
    """compare_all runs the unfused kernels against the oracle's reductor and the fused pass (k_f1w at this shape, factored and
    dense layout) against the unfused kernels."""
    p, eng, d = _problem(shape, kc), _setup(2, shape, kc), _oracle(shape, kc)
    V = make_bases(eng.S, eng.t.n, N, seed=89)
    res = compare_all(p, eng, energy_orthonormalize(V, d), 0.4, do_solve=False, oracle=d)
    assert 'fused_G_ab' in res and 'fused_dense_G_ab' in res and 'fused_G_aa' in res
    bad = {k: v for k, v in res.items() if not v < ORACLE_TOL}
    assert not bad, bad
