"""k_f1w (the rank-2 projection kernel, f1_form 0) against k_f1u (f1_form 2) at every N of its shape range that the bench
configs use, over the K-splits 1 / 2 / 4, with every output poisoned before each pass.  The chunk loops of k_f1w request the
scalars of the next chunk a whole stage ahead; short parts (two chunks per workgroup at K-split 4) run the clamped tail of
that rotation."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from common import make_bases, theta_bar_of  # noqa: E402

pytestmark = pytest.mark.gpu


def _engine(p):
    from pylrbms_amd.engine import Engine
    lam = p['lambda']
    return Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'],
                  theta_bar_of(p)).assemble()


def _pass(eng, V, N, form, ks):
    eng.ctx.set_option('f1_form', form)
    eng.ctx.set_option('f1_ksplit', ks)
    buf = eng.alloc_reduce_buffers(N)
    for x in list(buf['sys']) + list(buf['grams']):
        x.fill_(float('nan'))
    eng.ctx.kernel_timing(True)
    buf = eng.project_and_estimate(V, buf)
    ran = {k for k, _ in eng.ctx.kernel_timing_read()}
    eng.ctx.kernel_timing(False)
    return ran, [x.clone() for x in buf['sys']] + [x.clone() for x in buf['grams']]


@pytest.mark.parametrize('shape, kc, N', [((3, 3), 4, 34), ((4, 3), 4, 38), ((3, 2), 4, 40), ((2, 2), 2, 40)])
def test_f1w_matches_k_f1u_over_ksplits(shape, kc, N):
    import torch
    from pylrbms_amd import multiscale_problem
    p = multiscale_problem.init_grid_and_problem({'num_subdomains': list(shape), 'coarse_per_subdomain': kc})
    eng = _engine(p)
    assert eng.Q == 2
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=17))
    try:
        ran, ref = _pass(eng, V, N, 2, 1)
        assert 'k_f1u' in ran, sorted(ran)
        for ks in (1, 2, 4):
            ran, got = _pass(eng, V, N, 0, ks)
            assert 'k_f1w' in ran, (ks, sorted(ran))
            for i, (a, b) in enumerate(zip(ref, got)):
                assert bool(torch.isfinite(b).all()), (ks, i)
                assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max()), (ks, i)
            if ks > 1:
                _, again = _pass(eng, V, N, 0, ks)
                for a, b in zip(got, again):
                    assert torch.equal(a, b), ks
    finally:
        eng.ctx.set_option('f1_form', 0)
        eng.ctx.set_option('f1_ksplit', 0)
    assert np.isfinite(float(ref[0].abs().max()))
