"""Times batched snapshot generation at config 3 (32 x 32 subdomains, 393 k DoFs): d.solve_batch(mus) -- one
lrbms_fom_solve_batch call, four panels of 16 columns -- against the loop of 64 d.solve(mu) (lrbms_fom_solve) in the same
process, 64 parameters uniform in [0.1, 1], rtol 1e-10.  Untimed calls of both first, then the median of 5 alternated rounds.
Prints the iteration count of every panel beside the counts of the single solves, checks on the device that every column of
both paths meets rtol (|b - A(mu) x| / |b| through lrbms_fom_apply), and writes the report.
usage: fom_batch_time.py [REPORT]   (default profiles/fom_batch_time.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench import CONFIGS  # noqa: E402
from pylrbms_amd import multiscale_problem  # noqa: E402
from pylrbms_amd.discretize_elliptic_block_swipdg import discretize  # noqa: E402
from pylrbms_amd.parameters import parse_parameter  # noqa: E402

report = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'fom_batch_time.txt')
ROUNDS, NMU, RTOL, GATE = 5, 64, 1e-10, 2.0
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
d, _ = discretize(p)
eng, c = d.engine, d.engine.ctx
say('config 3: S {}  DoFs {}  parameters {} uniform in [0.1, 1] (seed 7)  rtol {:g}'.format(eng.S, eng.S * eng.t.n, NMU, RTOL))
mus = [parse_parameter([m], p['parameter_type']) for m in np.random.default_rng(7).uniform(0.1, 1.0, size=NMU)]
opts = {'precision': RTOL}
single_its = []


def loop():
    cols = []
    single_its.clear()
    for mu in mus:
        cols.append(d.solve(mu, inverse_options=opts).tensor)
        single_its.append(d.last_solve_info['iterations'])
    return torch.cat(cols, dim=2)


def batch():
    return d.solve_batch(mus, inverse_options=opts).tensor


def residual_ratios(X):
    """|b - A(mu_m) x_m| / |b| per column, on the device."""
    out = []
    bn = float(torch.linalg.norm(eng.b))
    for m, mu in enumerate(mus):
        x = X[:, :, m:m + 1].contiguous()
        y = c.fom_apply(d.theta(mu), eng.A_diag, eng.A_cpl, x)
        out.append(float(torch.linalg.norm(eng.b.reshape(-1) - y.reshape(-1))) / bn)
    return np.array(out)


X_loop, _ = once(loop)                                        # untimed
X_batch, _ = once(batch)
t_loop, t_batch = [], []
for rnd in range(ROUNDS):
    X_loop, tl = once(loop)
    X_batch, tb = once(batch)
    t_loop.append(tl)
    t_batch.append(tb)
    say('round {}  loop of {} d.solve  s {:.4f}   d.solve_batch  s {:.4f}   ratio {:.2f}'.format(rnd, NMU, tl, tb, tl / tb))
panels = d.last_solve_info
info_b = c.fom_solve_batch(np.stack([d.theta(mu) for mu in mus]), eng.A_diag, eng.A_cpl, np.ones((NMU, 1)),
                           eng.b.reshape(1, eng.S, eng.t.n), rtol=RTOL)[1]
say('iterations per panel (16 columns each, one coarse level at the mean theta): {}'.format(info_b['panel_iterations']))
its = np.array(single_its)
say('iterations of the single solves (own coarse level each): min {}  median {:.0f}  max {}   per panel of the same columns (max): {}'.format(
    its.min(), np.median(its), its.max(), [int(its[i:i + 16].max()) for i in range(0, NMU, 16)]))
r_loop, r_batch = residual_ratios(X_loop), residual_ratios(X_batch)
say('true residual ratio |b - A x| / |b|: loop max {:.2e}   batch max {:.2e}   (recurrence ratio of the batch {:.2e})'.format(
    r_loop.max(), r_batch.max(), panels['relative_residual']))
diff = float((X_loop - X_batch).abs().max() / X_loop.abs().max())
say('max |x_loop - x_batch| / max |x|  {:.2e}'.format(diff))
ml, mb = float(np.median(t_loop)), float(np.median(t_batch))
say('median of {}: loop s {:.4f} ({:.2f} ms per snapshot)   batch s {:.4f} ({:.2f} ms per snapshot, {:.1f} us per panel iteration)   '
    'speedup {:.2f}x   gate >= {:.1f}x: {}'.format(ROUNDS, ml, ml / NMU * 1e3, mb, mb / NMU * 1e3,
                                                 mb / max(1, sum(info_b['panel_iterations'])) * 1e6, ml / mb, GATE,
                                                 'met' if ml / mb >= GATE else 'MISSED'))
ok = bool(r_loop.max() <= 10 * RTOL and r_batch.max() <= 10 * RTOL and panels['relative_residual'] <= RTOL)
say('both paths meet rtol (recurrence ratio <= rtol, true residual within 10 rtol): {}'.format(ok))
os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
with open(report, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
sys.exit(0 if ok else 1)
