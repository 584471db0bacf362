"""Role B of k_f1w (f1_form 0) forms the flux applies Y^{q,q2} = W'^q_T R_T^{q2} on the 4x4x4 f64 MFMA: four independent
blocks per instruction, a lane standing for (block, k, j).  A wrong lane map swaps (q, q2) blocks or columns of the G_ab self
blocks and nothing else, so they are compared with k_f1u (f1_form 2) per (q, q2) block and per group of 16 columns, at every
even N of the kernel's range, over the K-splits 1 / 2 / 4 (long parts with coarse_per_subdomain 4, parts of two chunks at
K-split 4 with coarse_per_subdomain 2), with every output filled with NaN before each pass.  make_bases gives every subdomain
N distinct seeded columns, so all 2 N flux columns of a row differ and no swap goes unseen."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from common import make_bases, theta_bar_of  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12          # times the largest entry of the reference array (the figure of test_f1w_forms_gpu.py)
NAMES = ('B_sys', 'rhs_red', 'E_red', 'M_red', 'G_nc_self', 'r_fd', 'G_rdd_self', 'G_bb_self', 'G_ab_self', 'G_aa', 'F_side', 'F_nc')
I_GAB = NAMES.index('G_ab_self')      # [Q][S][N][Q N]: row of V, column q2 N + j of the flux basis


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


def _check_gab_blocks(ref, got, Q, N, ks):
    """Every entry of G_ab_self, per (q, q2) block and group of 16 columns; the message names the worst failing cell."""
    assert ref.shape == got.shape == (Q, ref.shape[1], N, Q * N), (ref.shape, got.shape)
    bound = TOL * float(ref.abs().max())
    failed = []
    for q in range(Q):
        for q2 in range(Q):
            for g in range((N + 15) // 16):
                lo, hi = q2 * N + 16 * g, q2 * N + min(16 * g + 16, N)
                d = (ref[q, :, :, lo:hi] - got[q, :, :, lo:hi]).abs()
                d = d.nan_to_num(nan=float('inf'))                  # an entry that was never written fails its cell
                worst = float(d.max())
                print('N {} ksplit {} block (q {}, q2 {}) columns {}..{}: max |diff| {:.3e} (bound {:.3e})'.format(
                    N, ks, q, q2, 16 * g, hi - q2 * N - 1, worst, bound))
                if not worst <= bound:
                    col = int(d.amax(dim=(0, 1)).argmax())
                    failed.append('block (q {}, q2 {}) columns {}..{}: max |diff| {:.3e} at column {}'.format(
                        q, q2, 16 * g, hi - q2 * N - 1, worst, 16 * g + col))
    assert not failed, 'G_ab_self, N {} ksplit {}, bound {:.3e}: {}'.format(N, ks, bound, '; '.join(failed))


@pytest.mark.parametrize('kc', [4, 2])
@pytest.mark.parametrize('N', [34, 36, 38, 40])
def test_f1w_role_b_apply_matches_k_f1u(N, kc):
    import torch
    from pylrbms_amd import multiscale_problem
    p = multiscale_problem.init_grid_and_problem({'num_subdomains': [3, 2], 'coarse_per_subdomain': kc})
    eng = _engine(p)
    assert eng.Q == 2
    V = eng.ctx.from_numpy(make_bases(eng.S, eng.t.n, N, seed=29))
    try:
        ran, ref = _pass(eng, V, N, 2, 1)
        assert 'k_f1u' in ran and 'k_f1w' not in ran, sorted(ran)
        assert len(ref) == len(NAMES), len(ref)
        for name, a in zip(NAMES, ref):
            assert bool(torch.isfinite(a).all()), name
        for ks in (1, 2, 4):
            ran, got = _pass(eng, V, N, 0, ks)
            assert 'k_f1w' in ran and 'k_f1u' not in ran, (ks, sorted(ran))
            _check_gab_blocks(ref[I_GAB], got[I_GAB], eng.Q, N, ks)
            for i, (name, a, b) in enumerate(zip(NAMES, ref, got)):
                assert a.shape == b.shape, (ks, name)
                assert bool(torch.isfinite(b).all()), (ks, name)
                worst, bound = float((a - b).abs().max()), TOL * float(a.abs().max())
                print('N {} ksplit {} {}: max |diff| {:.3e} (bound {:.3e})'.format(N, ks, name, worst, bound))
                assert worst <= bound, (ks, name, worst, bound)
            _, again = _pass(eng, V, N, 0, ks)
            for name, a, b in zip(NAMES, got, again):
                assert torch.equal(a, b), (ks, name)
    finally:
        eng.ctx.set_option('f1_form', 0)
        eng.ctx.set_option('f1_ksplit', 0)
