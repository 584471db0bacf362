"""Times the POD basis extension (extend_basis(method='pod'): lrbms_local_pod / lrbms3_local_pod) against the Gram-Schmidt loop
(extend_basis of the parabolic reductors) on the same input in the same process:
  config 3 (parabolic shape): 32 x 32 subdomains, k_c = 4 (n = 384), the 41-vector trajectory of 40 implicit Euler steps into the
                              order-0 basis, 16 modes;
  config 5:                   8 x 8 x 8 subdomains, k_c = 4 (n = 3840, P2), the 11-vector trajectory of 10 steps into the order-0
                              basis, 8 modes.
The loop is timed twice: to the same number of new vectors (max_vectors = 1 + modes: it stops after the first few time steps), and
over the whole trajectory.  Untimed calls first, then 5 timed repetitions of each, alternated; every repetition starts from the
same order-0 slab.  Reports median, minimum and the spread (max - min) and whether the loop's minimum lies above POD's maximum.
Then one POD call under lrbms(3)_kernel_timing: the time per kernel.  Writes profiles/local_pod_time.txt.
usage: local_pod_time.py [2d|3d|both]"""
import os
import statistics
import sys
import time
sys.path.insert(0, '.')
import numpy as np
import torch

WARM, REPS = 2, 5
lines = []


def say(*a):
    line = ' '.join(str(x) for x in a)
    print(line, flush=True)
    lines.append(line)


def run(tag, red, U, modes, desc):
    eng = red.d.engine
    V0, n0 = red._V.clone(), red._nloc.copy()

    def reset():
        red._V, red._nloc = V0.clone(), n0.copy()

    def pod():
        return red.extend_basis(U, method='pod', pod_modes=modes)

    def gs_same():
        red.extend_basis(U, max_vectors=1 + modes)

    def gs_all():
        red.extend_basis(U)

    cases = (('pod', pod), ('gram_schmidt to {} vectors'.format(1 + modes), gs_same), ('gram_schmidt, whole trajectory', gs_all))
    times = {name: [] for name, _ in cases}
    sizes = {}
    for rep in range(WARM + REPS):
        for name, fn in cases:                                   # alternated
            reset()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if rep >= WARM:
                times[name].append(dt)
            sizes[name] = (red.basis_size(), int(red._nloc.min()), int(red._nloc.max()))
    say('{}: {}'.format(tag, desc))
    for name, _ in cases:
        ts = times[name]
        say('  {:38s} median ms {:9.3f}  min ms {:9.3f}  max ms {:9.3f}  spread ms {:8.3f}  slab width {} (local sizes {} .. {})'.format(
            name, 1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts), 1e3 * (max(ts) - min(ts)), *sizes[name]))
    for name in [c[0] for c in cases[1:]]:
        ratio = statistics.median(times[name]) / statistics.median(times['pod'])
        clear = min(times[name]) > max(times['pod'])
        say('  {} / pod (medians) {:.2f}; the slowest pod repetition is {} the fastest of the loop'.format(
            name, ratio, 'faster than' if clear else 'NOT faster than'))
    reset()
    eng.ctx.kernel_timing(True)
    pod()
    per = {}
    for k, ms in eng.ctx.kernel_timing_read():
        per.setdefault(k, [0, 0.0])
        per[k][0] += 1
        per[k][1] += ms
    eng.ctx.kernel_timing(False)
    say('  one pod call, per kernel (events on the stream; the product applies and the copies are not bracketed):')
    for k, (cnt, ms) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        say('    {:24s} launches {:3d}  total ms {:8.3f}'.format(k, cnt, ms))
    reset()


def config3():
    from pylrbms_amd import multiscale_problem
    from pylrbms_amd.discretize_parabolic_block_swipdg import discretize
    from pylrbms_amd.reductor import ParabolicLRBMSReductor
    p = multiscale_problem.init_grid_and_problem({'num_subdomains': [32, 32], 'coarse_per_subdomain': 4})
    d, data = discretize(p, 0.05, 40)
    U = d.solve(d.parse_parameter(0.5))
    red = ParabolicLRBMSReductor(
        d, products=[d.operators['local_energy_dg_product_{}'.format(ii)] for ii in range(data['block_space'].num_blocks)])
    run('config 3', red, U, 16, 'S {} n {} snapshots {} modes 16 (2D, P1)'.format(d.engine.S, d.engine.t.n, U.tensor.shape[2]))


def config5():
    from pylrbms_amd import multiscale_problem3d
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D, discretize
    p = multiscale_problem3d.init_grid_and_problem({'num_subdomains': (8, 8, 8), 'cubes_per_subdomain': 4})
    d, _ = discretize(p, 0.1, 10)
    U = d.solve(0.5)
    red = ParabolicLRBMSReductor3D(d)
    run('config 5', red, U, 8, 'S {} n {} snapshots {} modes 8 (3D, P2)'.format(d.engine.S, d.engine.t.n, U.shape[2]))


which = sys.argv[1] if len(sys.argv) > 1 else 'both'
say('# python tools/local_pod_time.py {}: {} untimed and {} timed repetitions of each, alternated'.format(which, WARM, REPS))
if which in ('2d', 'both'):
    config3()
if which in ('3d', 'both'):
    config5()
os.makedirs('profiles', exist_ok=True)
out = os.path.join('profiles', 'local_pod_time.txt' if which == 'both' else 'local_pod_time_{}.txt'.format(which))
with open(out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
