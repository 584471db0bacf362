"""Times batched full-order trajectories at config 3 (32 x 32 subdomains, 393 k DoFs): d.solve_batch(mus) of the parabolic
discretization -- one lrbms_fom_implicit_euler_batch call, four panels of 16 columns, every panel its whole trajectory --
against the loop of 64 d.solve(mu) (lrbms_fom_implicit_euler) in the same process.  64 parameters uniform in [0.1, 1], T = 0.05,
10 steps (as tools/parabolic_batch_time.py), rtol 1e-10.  Untimed calls of both first, then the median of 5 alternated rounds.
Prints the iteration count of every panel (summed over the steps) beside the counts of the single solves, the iterations per step
of the slowest single solve, checks on the device that every step and column of both paths meets rtol
(|(M + dt A(mu)) u_{k+1} - M u_k - dt b| / |M u_k + dt b| through lrbms_fom_apply), and writes the report.
usage: fom_euler_batch_time.py [REPORT]   (default profiles/fom_euler_batch_time.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench import CONFIGS  # noqa: E402
from pylrbms_amd import multiscale_problem  # noqa: E402
from pylrbms_amd.discretize_parabolic_block_swipdg import discretize  # noqa: E402
from pylrbms_amd.parameters import parse_parameter  # noqa: E402

report = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'fom_euler_batch_time.txt')
ROUNDS, NMU, RTOL, T_END, NT = 5, 64, 1e-10, 0.05, 10
cfg = CONFIGS['cfg3']
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


p = multiscale_problem.init_grid_and_problem({'num_subdomains': cfg['num_subdomains'], 'coarse_per_subdomain': cfg['coarse_per_subdomain']})
d, _ = discretize(p, T_END, NT)
eng, c = d.engine, d.engine.ctx
dt = T_END / NT
say('config 3: S {}  DoFs {}  parameters {} uniform in [0.1, 1] (seed 7)  T {:g}  steps {}  rtol {:g}'.format(
    eng.S, eng.S * eng.t.n, NMU, T_END, NT, RTOL))
mus = [parse_parameter([m], p['parameter_type']) for m in np.random.default_rng(7).uniform(0.1, 1.0, size=NMU)]
opts = {'precision': RTOL}
single_its = []


def loop():
    """-> [S, n, nt + 1, NMU]"""
    cols = []
    single_its.clear()
    for mu in mus:
        cols.append(d.solve(mu, inverse_options=opts).tensor)
        single_its.append(d.last_solve_info['iterations'])
    return torch.stack(cols, dim=3)


def batch():
    return torch.stack([u.tensor for u in d.solve_batch(mus, inverse_options=opts)], dim=3)


area = c.from_numpy(np.asarray(eng.t.area, dtype=np.float64))


def mass_apply(u):
    """M u for u [S, n, L]: |T| / 12 (1 + delta_ij) per element."""
    v = u.reshape(eng.S, eng.t.n // 3, 3, -1)
    return (area[None, :, None, None] / 12.0 * (v.sum(dim=2, keepdim=True) + v)).reshape(u.shape)


def residual_ratios(U):
    """The worst step of every column of U [S, n, nt + 1, NMU], on the device."""
    out = []
    b = eng.b.reshape(eng.S, eng.t.n, 1)
    for m, mu in enumerate(mus):
        u = U[..., m].contiguous()
        rhs = mass_apply(u[:, :, :-1]) + dt * b
        new = u[:, :, 1:].contiguous()
        lhs = mass_apply(new) + dt * c.fom_apply(d.theta(mu), eng.A_diag, eng.A_cpl, new)
        out.append(float((torch.linalg.norm((lhs - rhs).reshape(-1, NT), dim=0) / torch.linalg.norm(rhs.reshape(-1, NT), dim=0)).max()))
    return np.array(out)


U_loop, _ = once(loop)                                        # untimed
U_batch, _ = once(batch)
t_loop, t_batch = [], []
for rnd in range(ROUNDS):
    U_loop, tl = once(loop)
    U_batch, tb = once(batch)
    t_loop.append(tl)
    t_batch.append(tb)
    say('round {}  loop of {} d.solve  s {:.4f}   d.solve_batch  s {:.4f}   ratio {:.2f}'.format(rnd, NMU, tl, tb, tl / tb))
info = d.last_solve_info
info_b = c.fom_implicit_euler_batch(np.stack([d.theta(mu) for mu in mus]), dt, NT, eng.A_diag, eng.A_cpl, eng.b.reshape(1, eng.S, eng.t.n),
                                    np.ones((NMU, NT + 1, 1)), rtol=RTOL)[1]
say('iterations per panel, summed over the {} steps (16 columns each, one coarse level at the mean theta): {}'.format(
    NT, info_b['panel_iterations']))
its = np.array(single_its)
say('iterations of the single solves over the {} steps (own coarse level each): min {}  median {:.0f}  max {}   per panel of the same '
    'columns (max): {}'.format(NT, its.min(), np.median(its), its.max(), [int(its[i:i + 16].max()) for i in range(0, NMU, 16)]))
slow = int(its.argmax())
per_step, u = [], None
for k in range(NT):                                           # the same trajectory one step per call: its iterations per step
    Uk, ik = c.fom_implicit_euler(d.theta(mus[slow]), dt, 1, eng.A_diag, eng.A_cpl, eng.b, U0=u, rtol=RTOL)
    per_step.append(ik['iterations'])
    u = Uk[1]
say('iterations per step of the slowest single solve (column {}): {}'.format(slow, per_step))
r_loop, r_batch = residual_ratios(U_loop), residual_ratios(U_batch)
say('true residual ratio of the worst step: loop max {:.2e}   batch max {:.2e}   (recurrence ratio of the batch {:.2e})'.format(
    r_loop.max(), r_batch.max(), info['relative_residual']))
diff = float((U_loop - U_batch).abs().max() / U_loop.abs().max())
say('max |u_loop - u_batch| / max |u|  {:.2e}'.format(diff))
ml, mb = float(np.median(t_loop)), float(np.median(t_batch))
spread = max(max(t_loop) - min(t_loop), max(t_batch) - min(t_batch))
say('median of {}: loop s {:.4f} ({:.2f} ms per trajectory)   batch s {:.4f} ({:.2f} ms per trajectory, {:.1f} us per panel iteration)   '
    'speedup {:.2f}x   spread between rounds s {:.4f}   batch faster by more than the spread: {}'.format(
        ROUNDS, ml, ml / NMU * 1e3, mb, mb / NMU * 1e3, mb / max(1, sum(info_b['panel_iterations'])) * 1e6, ml / mb, spread,
        ml - mb > spread))
ok = bool(r_loop.max() <= 10 * RTOL and r_batch.max() <= 10 * RTOL and info['relative_residual'] <= RTOL)
say('both paths meet rtol (recurrence ratio <= rtol, true residual within 10 rtol): {}'.format(ok))
os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
with open(report, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
sys.exit(0 if ok else 1)
