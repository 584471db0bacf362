"""Times the batched neighbourhood corrector solves of the 3D / P2 path (config 5 by default: 8x8x8 subdomains, k_c 4) by HIP
events around calls that end in a synchronise, after a warm-up call: 16 marked subdomains and all of them, against one
full-order solve (block-Jacobi alone) of the same session, whose matvec streams the same operator.
usage: enrichment3d_time.py [P] [kc] [rtol]"""
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from pylrbms_amd import multiscale_problem3d  # noqa: E402
from pylrbms_amd.engine3d import Engine3D  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 8
kc = int(sys.argv[2]) if len(sys.argv) > 2 else 4
rtol = float(sys.argv[3]) if len(sys.argv) > 3 else 1e-10
p = multiscale_problem3d.init_grid_and_problem({'num_subdomains': (P, P, P), 'cubes_per_subdomain': kc})
eng = Engine3D(p['grid'], p['lambda']['functions'], p['f'], p['lambda_bar'], p['lambda_hat']).assemble(online_enrichment=True)
c, t, ops = eng.ctx, eng.t, eng.ops
S, n, nT, ncf = eng.S, t.n, t.n_T, t.ncf
th = np.array([1.0, 0.5])
print('S', S, 'n', n, 'n_T', nT, 'ncf', ncf, 'Q', eng.Q, 'rtol', rtol, flush=True)


def event_ms(fn, reps=3):
    fn()                                                    # warm-up
    best, out = 1e30, None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return out, best


# ---- one full-order solve without the coarse level: the iteration the corrector iteration is set against
c.fom_coarse_space(None)
(U, info), ms = event_ms(lambda: c.fom_solve(eng.Q, th, ops['A_diag'], ops['A_cpl'], ops['b'], rtol=rtol))
op_bytes = 8.0 * (S * nT * 500 + S * 6 * ncf * 100)
fom_vec = 8.0 * S * n * (3 + 2 + 7 + 5.6)                   # dir 3, matvec 2, update 7 doubles per DoF + the packed block inverses
fom_it = ms / max(int(info[0]), 1)
print('fom_solve (block-Jacobi): {:.1f} ms, {} iterations, {:.1f} us per iteration; bytes per iteration from shapes: operator {:.0f} MB '
      '+ vectors and block inverses {:.0f} MB'.format(ms, int(info[0]), 1e3 * fom_it, op_bytes / 1e6, fom_vec / 1e6), flush=True)

# ---- corrector solves
slots = np.asarray(p['grid'].neighbor_slots)
for label, marked in (('16 marked', list(range(0, S, max(S // 16, 1)))[:16]), ('all marked', list(range(S)))):
    nmark = len(marked)
    work = c.empty(c.local_correction_work_size(nmark))
    (corr, inf), ms = event_ms(lambda: c.local_correction_solve(eng.Q, th, marked, ops['A_diag'], ops['A_cpl'], ops['D_corr'], ops['b'],
                                                                rtol=rtol, work=work))
    its = int(inf[:, 0].max())
    nslot = int((slots[marked] >= 0).sum())                 # member (problem, slot) pairs: the vectors that exist
    members = len({int(v) for v in slots[marked].ravel() if v >= 0})
    opb = 8.0 * members * (nT * 500 + 2 * 6 * ncf * 100)      # Amu, Cmu and Dmu of the member subdomains, once
    vecb = 8.0 * nslot * n * (3 + 2 + 7 + 5.6)               # per (problem, slot): as above, the block inverses once per slot
    print('{}: nmark {}, {:.1f} ms per call, iterations {} .. {}, {:.1f} local solves/s, {:.1f} us per iteration; work {:.0f} MB; bytes per '
          'iteration from shapes: operator {:.0f} MB (once, {} member subdomains) + vectors and block inverses {:.0f} MB ({} slots); '
          'iteration / fom iteration = {:.2f}'.format(label, nmark, ms, int(inf[:, 0].min()), its, nmark / ms * 1e3, 1e3 * ms / its,
                                                      8.0 * work.numel() / 1e6, opb / 1e6, members, vecb / 1e6, nslot,
                                                      ms / its / fom_it), flush=True)
    del work
