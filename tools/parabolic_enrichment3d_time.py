"""Times the corrector trajectories of the parabolic enrichment on the 3D / P2 path (``lrbms3_local_correction_euler``, DESIGN.md
9.19) at config 5's shape (8 x 8 x 8 subdomains, k_c 4: 3 840 DoFs each, Q = 2) with nt = 10 steps, for 16 and 512 marked subdomains:

* one ``lrbms3_local_correction_euler`` call against ``nt`` calls of ``lrbms3_local_correction_solve`` on the same neighbourhoods (the
  only other native solver of those systems; the step operator M + dt A is better conditioned than A, but every step pays one extra
  matvec and at least one poll of the scalars), with the iteration counts of both;
* one enrichment round (``ParabolicLRBMSReductor3D.enrich_local_batch`` + ``reduce(touched=)``) split into the corrector call, the
  local POD and the incremental re-projection.

Host clock around calls that end in a device synchronise; untimed passes first, then the median of ``reps`` alternating passes.
The per-kernel split is not taken here.
usage: parabolic_enrichment3d_time.py [P] [kc] [nt] [reps] [out]"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from pylrbms_amd import multiscale_problem3d  # noqa: E402
from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D, discretize  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 8
kc = int(sys.argv[2]) if len(sys.argv) > 2 else 4
nt = int(sys.argv[3]) if len(sys.argv) > 3 else 10
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
out_path = sys.argv[5] if len(sys.argv) > 5 else None
T, mu, rtol = 0.05, 0.37, 1e-10
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


p = multiscale_problem3d.init_grid_and_problem({'num_subdomains': (P, P, P), 'cubes_per_subdomain': kc})
d, _ = discretize(p, T, nt, online_enrichment=True)
eng = d.engine
S, n = eng.S, eng.t.n
dt = T / nt
theta = d.theta(mu)
say('S {} n {} n_T {} Q {} nt {} dt {:g} rtol {:g}, {} ({}), median of {} passes after 2 untimed ones'.format(
    S, n, eng.t.n_T, eng.Q, nt, dt, rtol, torch.cuda.get_device_name(0), time.strftime('%Y-%m-%d'), reps))

rng = np.random.default_rng(0)
for nmark in (16, 512):
    marked = sorted(rng.choice(S, size=min(nmark, S), replace=False).tolist())

    def euler():
        return eng.local_corrections_euler(theta, dt, nt, marked, rtol=rtol)

    def stationary():
        for _ in range(nt):
            out = eng.local_corrections(theta, marked, rtol=rtol)
        return out
    for _ in range(2):
        euler(), stationary()
    te, ts = [], []
    for _ in range(reps):                                       # alternating: both see the same clocks
        (_, ie), ms = clock(euler)
        te.append(ms)
        (_, is_), ms = clock(stationary)
        ts.append(ms)
    me, ms_ = float(np.median(te)), float(np.median(ts))
    say('{:4d} marked: euler (1 call, {} steps) {:.3f} ms [{:.3f} .. {:.3f}], iterations per neighbourhood {:.0f} .. {:.0f} summed over the '
        'steps; stationary x {} calls {:.3f} ms [{:.3f} .. {:.3f}], iterations per call {:.0f} .. {:.0f}; euler / stationary = {:.2f}'.format(
            len(marked), nt, me, min(te), max(te), ie[:, 0].min(), ie[:, 0].max(), nt, ms_, min(ts), max(ts), is_[:, 0].min(),
            is_[:, 0].max(), me / ms_))

# ---- one enrichment round: corrector call, local POD, incremental re-projection
reductor = ParabolicLRBMSReductor3D(d)
U0 = d.solve(1.0)
reductor.extend_basis(U0[:, :, [1, nt // 2, nt]])
del U0
reductor.reserve(reductor.basis_size() + 2)
rd = reductor.reduce()
say('enrichment round at N = {} (slab width), pod_modes 2:'.format(reductor.basis_size()))
for nmark in (16, 512):
    marked = sorted(rng.choice(S, size=min(nmark, S), replace=False).tolist())
    tc, tr, tt = [], [], []
    for k in range(reps + 2):
        _, c_ms = clock(lambda: d.solve_for_local_correction_trajectories(marked, mu))          # (the defaults enrich_local_batch uses)
        _, e_ms = clock(lambda: reductor.enrich_local_batch(marked, None, mu, pod_modes=2))     # (its own corrector call included)
        _, r_ms = clock(lambda: reductor.reduce(touched=marked))
        if k >= 2:
            tc.append(c_ms), tt.append(e_ms), tr.append(r_ms)
    c_ms, e_ms, r_ms = (float(np.median(x)) for x in (tc, tt, tr))
    total = e_ms + r_ms
    say('{:4d} marked: round {:.3f} ms = correctors (rtol 1e-12) {:.3f} ms ({:.0f} %) + scatter and local POD {:.3f} ms ({:.0f} %) + '
        'reduce(touched=) {:.3f} ms ({:.0f} %, {}); local sizes now {} .. {}'.format(
            len(marked), total, c_ms, 100 * c_ms / total, e_ms - c_ms, 100 * (e_ms - c_ms) / total, r_ms, 100 * r_ms / total,
            reductor.last_reduce_info, min(reductor.local_sizes()), max(reductor.local_sizes())))
if out_path:
    with open(out_path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
