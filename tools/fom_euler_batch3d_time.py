"""Times batched full-order trajectories on the 3D / P2 path at config 5 (8 x 8 x 8 subdomains, k_c = 4, 1.97 M DoFs):
d.solve_batch(mus) -- one lrbms3_fom_implicit_euler_batch call, four panels of 16 columns, panels outermost -- against the loop of
64 d.solve(mu) (lrbms3_fom_implicit_euler) in the same process, 64 parameters uniform in [0.1, 1], nt = 10 steps, rtol 1e-10 as
tools/parabolic3d_time.py.  Untimed calls of both first, then 5 alternated rounds, median and spread.  Prints the iterations of
every panel beside the slowest single solve of the same columns, the true residual
|(M + dt A(mu)) u_{k+1} - M u_k - dt b| / |M u_k + dt b| of the worst step of both paths (lrbms3_fom_apply, the mass from the
table TM), their agreement relative to max |u|, and writes the report.
usage: fom_euler_batch3d_time.py [REPORT [P [kc [ROUNDS [NT]]]]]   (default profiles/fom_euler_batch3d_time.txt 8 4 5 10)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pylrbms_amd import multiscale_problem3d  # noqa: E402
from pylrbms_amd.discretize_parabolic_block_swipdg_3d import discretize  # noqa: E402

report = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'fom_euler_batch3d_time.txt')
P = int(sys.argv[2]) if len(sys.argv) > 2 else 8
kc = int(sys.argv[3]) if len(sys.argv) > 3 else 4
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
NT = int(sys.argv[5]) if len(sys.argv) > 5 else 10
NMU, RTOL, GATE, T_END = 64, 1e-10, 2.0, 0.1
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


p = multiscale_problem3d.init_grid_and_problem({'num_subdomains': (P, P, P), 'cubes_per_subdomain': kc})
d, _ = discretize(p, T_END, NT)
eng, c = d.engine, d.engine.ctx
say('{} x {} x {} subdomains, k_c {}: S {}  DoFs {}  parameters {} uniform in [0.1, 1] (seed 7)  T {:g}  nt {}  rtol {:g}'.format(
    P, P, P, kc, eng.S, eng.S * eng.t.n, NMU, T_END, NT, RTOL))
mus = [float(m) for m in np.random.default_rng(7).uniform(0.1, 1.0, size=NMU)]
single_its = []


def loop():
    out = []
    single_its.clear()
    for mu in mus:
        U, info = d.solve(mu, rtol=RTOL, return_info=True)
        out.append(U)
        single_its.append(info[0])
    return out


def batch():
    return d.solve_batch(mus, rtol=RTOL)


TM = torch.as_tensor(eng.t.tables(eng.spec)['TM'].reshape(6, 10, 10)[eng.t.elem_type], device=eng.ops['b'].device)      # [n_T, 10, 10]


def worst_step_residual(U, mu):
    """max over the steps of |(M + dt A) u_{k+1} - (M u_k + dt b)| / |M u_k + dt b| for a trajectory U [S, n, nt + 1]."""
    U = U.contiguous()
    S, n, L = U.shape
    MU = torch.einsum('eij,sejl->seil', TM, U.reshape(S, -1, 10, L)).reshape(S, n, L)
    AU = c.fom_apply(d.Q, d.theta(mu), eng.ops['A_diag'], eng.ops['A_cpl'], U[:, :, 1:].contiguous())
    f = MU[:, :, :-1] + d.dt * eng.ops['b'][:, :, None]
    r = MU[:, :, 1:] + d.dt * AU - f
    return float((torch.linalg.norm(r.reshape(-1, L - 1), dim=0) / torch.linalg.norm(f.reshape(-1, L - 1), dim=0)).max())


U_loop, _ = once(loop)                                        # untimed
U_batch, _ = once(batch)
t_loop, t_batch = [], []
for rnd in range(ROUNDS):
    U_loop = None
    U_loop, tl = once(loop)
    U_batch = None
    U_batch, tb = once(batch)
    t_loop.append(tl)
    t_batch.append(tb)
    say('round {}  loop of {} d.solve  s {:.3f}   d.solve_batch  s {:.3f}   ratio {:.2f}'.format(rnd, NMU, tl, tb, tl / tb))
its_b, rel_b = d.last_solve_info
_, info_b = c.fom_implicit_euler_batch(np.stack([d.theta(mu) for mu in mus]), d.dt, NT, eng.ops['A_diag'], eng.ops['A_cpl'],
                                       eng.ops['b'].reshape(1, eng.S, eng.t.n), np.ones((NMU, NT + 1, 1)), rtol=RTOL)
say('iterations per panel over the {} steps (16 columns each, one preconditioner at the mean theta): {}   sum {}'.format(
    NT, info_b['panel_iterations'], info_b['iterations']))
its = np.array(single_its)
say('iterations of the single trajectories (own element inverses and coarse level): min {}  median {:.0f}  max {}   slowest per panel '
    'of the same columns: {}'.format(its.min(), np.median(its), its.max(), [int(its[i:i + 16].max()) for i in range(0, NMU, 16)]))
r_loop = np.array([worst_step_residual(U, mu) for U, mu in zip(U_loop, mus)])
r_batch = np.array([worst_step_residual(U, mu) for U, mu in zip(U_batch, mus)])
say('true residual of the worst step |(M + dt A) u_k+1 - f| / |f|: loop max {:.2e}   batch max {:.2e}   (recurrence ratio of the batch '
    '{:.2e})'.format(r_loop.max(), r_batch.max(), rel_b))
umax = max(float(U.abs().max()) for U in U_loop)
diff = max(float((a - b).abs().max()) for a, b in zip(U_loop, U_batch)) / umax
say('max |u_loop - u_batch| / max |u|  {:.2e}'.format(diff))
ml, mb = float(np.median(t_loop)), float(np.median(t_batch))
say('loop s: median {:.3f}  min {:.3f}  max {:.3f}    batch s: median {:.3f}  min {:.3f}  max {:.3f}'.format(
    ml, min(t_loop), max(t_loop), mb, min(t_batch), max(t_batch)))
say('median of {}: loop {:.1f} ms per trajectory   batch {:.1f} ms per trajectory, {:.1f} us per panel iteration   speedup {:.2f}x   '
    'gate >= {:.1f}x: {}'.format(ROUNDS, ml / NMU * 1e3, mb / NMU * 1e3, mb / max(1, info_b['iterations']) * 1e6, ml / mb, GATE,
                                 'met' if ml / mb >= GATE else 'MISSED'))
ok = bool(r_loop.max() <= 10 * RTOL and r_batch.max() <= 10 * RTOL and rel_b <= RTOL)
say('both paths meet rtol (recurrence ratio <= rtol, true residual within 10 rtol): {}'.format(ok))
os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
with open(report, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
sys.exit(0 if ok else 1)
