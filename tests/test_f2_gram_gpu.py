"""LRBMS_OPT_F2_FORM: the Gram form of the flux-Gram kernel (k_f2g, default) against the R~^T B R~ form (k_f2) on the same
inputs -- runs on the MI355X box (`-m gpu`).

The Gram form refactors the sums behind G_bb[self, self] and G_rdd[self, self] (B_T = C_T^T C_T, |T| = sqrt|T|^2), so those two
arrays agree with k_f2 to rounding; every other output of the pass is the same bits.  One cell per k_f2g<NR> instantiation
(NR = ceil(Q N / 16) = 1 .. 8), in both output layouts."""
import numpy as np
import pytest

from common import make_bases, problem_with_q_components, theta_bar_of

pytestmark = pytest.mark.gpu

# (Q, N, subdomains, k_c): NR in the comment
CELLS = [
    (2, 40, (6, 5), 4),     # NR 5: config 3's kernel shape
    (2, 20, (4, 4), 2),     # NR 3
    (2, 33, (3, 2), 2),     # NR 5, odd N
    (2, 64, (2, 2), 4),     # NR 8, QN = 128
    (1, 40, (3, 2), 2),     # NR 3, Q = 1
    (1, 16, (3, 2), 2),     # NR 1
    (1, 17, (3, 2), 2),     # NR 2
    (2, 32, (3, 2), 2),     # NR 4
    (2, 48, (3, 3), 4),     # NR 6
    (3, 37, (3, 2), 2),     # NR 7
]


def _engine(Q, shape, kc):
    from pylrbms_amd.engine import Engine
    if Q == 2:
        from pylrbms_amd import multiscale_problem
        p = multiscale_problem.init_grid_and_problem({'num_subdomains': list(shape), 'coarse_per_subdomain': kc})
    else:
        p = problem_with_q_components(shape, kc, Q)
    lam = p['lambda']
    return Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'],
                  theta_bar_of(p)).assemble()


def _pass(eng, V, N, factored, form):
    eng.ctx.set_option('f2_form', form)
    try:
        buf = eng.project_and_estimate(V, eng.alloc_reduce_buffers(N, factored=factored))
        return [x.clone() for x in buf['sys']] + [x.clone() for x in buf['grams']]
    finally:
        eng.ctx.set_option('f2_form', 0)


def _self_blocks(outs, factored):
    """G_rdd[self, self], G_bb[self, self]: [S, QN, QN] (block 0 of the dense block-compact layout)."""
    G_rdd, G_bb = outs[4 + 2], outs[4 + 3]
    return (G_rdd, G_bb) if factored else (G_rdd[:, 0], G_bb[:, 0])


@pytest.mark.parametrize('factored', [True, False], ids=['factored', 'dense'])
@pytest.mark.parametrize('Q, N, shape, kc', CELLS)
def test_gram_form_agrees_with_the_product_form(Q, N, shape, kc, factored):
    import torch
    eng = _engine(Q, shape, kc)
    assert eng.Q == Q and eng.ctx.fused_supported(Q, N, factored=factored)
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=5))
    ref = _pass(eng, V, N, factored, 1)
    out = _pass(eng, V, N, factored, 0)
    gram = {4 + 2, 4 + 3}                      # G_rdd, G_bb: whole arrays (the side blocks come from the thin kernels: same bits)
    for i, (a, b) in enumerate(zip(ref, out)):
        if i in gram:
            continue
        assert torch.equal(a, b), 'output {} differs'.format(i)
    for a, b in zip(_self_blocks(ref, factored), _self_blocks(out, factored)):
        assert bool(torch.isfinite(b).all())
        scale = float(a.abs().max())
        assert float((a - b).abs().max()) <= 1e-13 * scale
        assert float((b - b.transpose(1, 2)).abs().max()) <= 1e-14 * scale
    if not factored:                           # the blocks outside [self, self] are k_f2's business in neither form
        for k in (4 + 2, 4 + 3):
            assert torch.equal(ref[k][:, 1:], out[k][:, 1:])


@pytest.mark.parametrize('Q, N, shape, kc', [CELLS[0], CELLS[3], CELLS[4]])
def test_non_spd_flux_mass_gives_a_non_finite_g_bb(Q, N, shape, kc):
    """k_f2g factors B_T by Cholesky: a Bbb block that is not SPD must not come out as finite wrong numbers.  The subdomain that
    holds it gets a NaN G_bb[self, self]; every other subdomain keeps the bits of the unpoisoned pass."""
    import torch
    eng = _engine(Q, shape, kc)
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=9))
    good = _pass(eng, V, N, True, 0)
    Bbb = eng.Bbb.clone()
    B4 = Bbb.view(eng.S, -1, 3, 3)
    s0, T0 = eng.S // 2, B4.shape[1] // 3
    B4[s0, T0, 1, 1] = -B4[s0, T0, 1, 1]           # pivot 1 of the Cholesky factor < 0
    eng.Bbb = Bbb
    eng.__dict__.pop('_bound_pass', None)
    bad = _pass(eng, V, N, True, 0)
    G_bb, G_bb_good = bad[4 + 3], good[4 + 3]
    assert bool(torch.isnan(G_bb[s0]).all())
    others = [s for s in range(eng.S) if s != s0]
    assert torch.equal(G_bb[others], G_bb_good[others])
    assert np.isfinite(float(G_bb_good.abs().max()))
