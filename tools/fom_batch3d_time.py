"""Times batched snapshot generation on the 3D / P2 path at config 5 (8 x 8 x 8 subdomains, k_c = 4, 1.97 M DoFs):
d.solve_batch(mus) -- one lrbms3_fom_solve_batch call, four panels of 16 columns -- against the loop of 64 d.solve(mu)
(lrbms3_fom_solve with its kept coarse inverse) in the same process, 64 parameters uniform in [0.1, 1], rtol 1e-8 as
tools/fom3d_time.py.  Untimed calls of both first, then 5 alternated rounds, median and spread.  Prints the iteration count of
every panel beside the counts of the single solves of the same columns, and the true residual |b - A(mu) x| / |b| of every
column of both paths (lrbms3_fom_apply), and writes the report.
usage: fom_batch3d_time.py [REPORT [P [kc [ROUNDS]]]]   (default profiles/fom_batch3d_time.txt 8 4 5)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pylrbms_amd import multiscale_problem3d  # noqa: E402
from pylrbms_amd.discretize_elliptic_block_swipdg_3d import discretize  # noqa: E402

report = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'fom_batch3d_time.txt')
P = int(sys.argv[2]) if len(sys.argv) > 2 else 8
kc = int(sys.argv[3]) if len(sys.argv) > 3 else 4
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
NMU, RTOL, GATE = 64, 1e-8, 2.0
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
d, _ = discretize(p)
eng, c = d.engine, d.engine.ctx
say('{} x {} x {} subdomains, k_c {}: S {}  DoFs {}  parameters {} uniform in [0.1, 1] (seed 7)  rtol {:g}'.format(
    P, P, P, kc, eng.S, eng.S * eng.t.n, NMU, RTOL))
mus = [float(m) for m in np.random.default_rng(7).uniform(0.1, 1.0, size=NMU)]
single_its = []
batch_info = []


def loop():
    cols = []
    single_its.clear()
    for mu in mus:
        U, info = d.solve(mu, rtol=RTOL, return_info=True)
        cols.append(U[:, :, None])
        single_its.append(info[0])
    return torch.cat(cols, dim=2)


def batch():
    X, info = c.fom_solve_batch(np.stack([d.theta(mu) for mu in mus]), eng.ops['A_diag'], eng.ops['A_cpl'], np.ones((NMU, 1)),
                                eng.ops['b'].reshape(1, eng.S, eng.t.n), rtol=RTOL)
    batch_info[:] = [info]
    return X


def batch_api():
    return d.solve_batch(mus, rtol=RTOL)


def residual_ratios(X):
    """|b - A(mu_m) x_m| / |b| per column, on the device."""
    out = []
    b = eng.ops['b'].reshape(-1)
    bn = float(torch.linalg.norm(b))
    for m, mu in enumerate(mus):
        x = X[:, :, m:m + 1].contiguous()
        y = c.fom_apply(d.Q, d.theta(mu), eng.ops['A_diag'], eng.ops['A_cpl'], x)
        out.append(float(torch.linalg.norm(b - y.reshape(-1))) / bn)
    return np.array(out)


X_loop, _ = once(loop)                                        # untimed
X_batch, _ = once(batch_api)
t_loop, t_batch = [], []
for rnd in range(ROUNDS):
    X_loop, tl = once(loop)
    X_batch, tb = once(batch_api)
    t_loop.append(tl)
    t_batch.append(tb)
    say('round {}  loop of {} d.solve  s {:.4f}   d.solve_batch  s {:.4f}   ratio {:.2f}'.format(rnd, NMU, tl, tb, tl / tb))
once(batch)
info_b = batch_info[0]
say('iterations per panel (16 columns each, one preconditioner at the mean theta): {}'.format(info_b['panel_iterations']))
its = np.array(single_its)
say('iterations of the single solves (own element inverses, kept coarse inverse): min {}  median {:.0f}  max {}   per panel of the same '
    'columns (max): {}'.format(its.min(), np.median(its), its.max(), [int(its[i:i + 16].max()) for i in range(0, NMU, 16)]))
r_loop, r_batch = residual_ratios(X_loop), residual_ratios(X_batch)
say('true residual ratio |b - A x| / |b|: loop max {:.2e}   batch max {:.2e}   (recurrence ratio of the batch {:.2e})'.format(
    r_loop.max(), r_batch.max(), info_b['relative_residual']))
diff = float((X_loop - X_batch).abs().max() / X_loop.abs().max())
say('max |x_loop - x_batch| / max |x|  {:.2e}'.format(diff))
ml, mb = float(np.median(t_loop)), float(np.median(t_batch))
say('loop s: median {:.4f}  min {:.4f}  max {:.4f}    batch s: median {:.4f}  min {:.4f}  max {:.4f}'.format(
    ml, min(t_loop), max(t_loop), mb, min(t_batch), max(t_batch)))
say('median of {}: loop {:.2f} ms per snapshot   batch {:.2f} ms per snapshot, {:.1f} us per panel iteration   speedup {:.2f}x   '
    'gate >= {:.1f}x: {}'.format(ROUNDS, ml / NMU * 1e3, mb / NMU * 1e3, mb / max(1, sum(info_b['panel_iterations'])) * 1e6, ml / mb, GATE,
                                 'met' if ml / mb >= GATE else 'MISSED'))
ok = bool(r_loop.max() <= 10 * RTOL and r_batch.max() <= 10 * RTOL and info_b['relative_residual'] <= RTOL)
say('both paths meet rtol (recurrence ratio <= rtol, true residual within 10 rtol): {}'.format(ok))
os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
with open(report, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
sys.exit(0 if ok else 1)
