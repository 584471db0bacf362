"""Times the streamed POD basis extension (extend_basis(method='hapod'): lrbms_local_pod_stream_* / lrbms3_local_pod_stream_*) on
the training sets the batched full-order solvers produce, in the same process as the only route the single-call POD has for the
same columns:
  config 3 (parabolic shape): 32 x 32 subdomains, k_c = 4 (n = 384), 64 parameters x 40 implicit Euler steps: 40 slabs of 64
                              columns from d.solve_batch(mus, as_snapshots='slabs'), into the order-0 basis, 16 modes;
  config 5:                   8 x 8 x 8 subdomains, k_c = 4 (n = 3840, P2), 64 parameters x 10 steps: 10 slabs, 8 modes.
Variants, alternated, untimed calls first, then 5 timed repetitions of each, every repetition from the same order-0 slab:
  hapod keep 64 / keep 32 (pieces of 64 / 96 columns), each with the rotation on the MFMA kernel (k_pod_stream_rotate, option
  pod_rotate_valu 0) and on the k_pod_xt route (two launches into a second buffer and the copy back, option 1);
  pod: extend_basis_pod on the stacked set (torch.cat of the slabs, timed with it and reported apart), consecutive 128-column calls.
Reports per variant the median / min / max of a whole extension, the time per push, the device-to-host copies it makes (every
.cpu() of the call), the vectors appended and the squared projection error of the whole set onto the basis, in the local product.
Then one short stream (4 pushes and finish) per route under lrbms(3)_kernel_timing: the time per kernel.
The two routes compute different things (k modes of the set / k modes per 128 columns), so both sides are reported, no ratio.
Writes profiles/local_pod_stream_time.txt.
usage: local_pod_stream_time.py [2d|3d|both]"""
import os
import statistics
import sys
import time
sys.path.insert(0, '.')
import numpy as np
import torch

WARM, REPS = 1, 5
lines = []


def say(*a):
    line = ' '.join(str(x) for x in a)
    print(line, flush=True)
    lines.append(line)


class CopyCounter:
    """Counts the device-to-host copies of a call: every Tensor.cpu() of a device tensor."""

    def __enter__(self):
        self.count, self._cpu = 0, torch.Tensor.cpu
        counter, orig = self, self._cpu

        def cpu(t, *a, **kw):
            if t.is_cuda:
                counter.count += 1
            return orig(t, *a, **kw)
        torch.Tensor.cpu = cpu
        return self

    def __exit__(self, *exc):
        torch.Tensor.cpu = self._cpu


def projection_error2(red, slabs):
    """sum_j |u_j - Pi u_j|_P^2 over all columns of all slabs and all subdomains, Pi the P-projection onto the local bases."""
    S = red.d.engine.S
    V = red._V[:S].contiguous()
    total = 0.0
    for U in slabs:
        U = U.contiguous()
        E = U - torch.einsum('snk,skl->snl', V, torch.einsum('snk,snl->skl', V, red._product_apply(U)))
        total += float((E * red._product_apply(E)).sum())
    return total


def run(tag, red, slabs, modes, desc):
    eng = red.d.engine
    ctx = eng.ctx
    V0, n0 = red._V.clone(), red._nloc.copy()
    columns = sum(int(u.shape[2]) for u in slabs)

    def reset():
        red._V, red._nloc = V0.clone(), n0.copy()

    def hapod(keep, valu):
        def fn():
            ctx.set_option('pod_rotate_valu', valu)
            try:
                return red.extend_basis_hapod(slabs, modes=modes, keep=keep)
            finally:
                ctx.set_option('pod_rotate_valu', 0)
        return fn

    cat_times = []

    def pod():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        stacked = torch.cat(list(slabs), dim=2)
        torch.cuda.synchronize(); cat_times.append(time.perf_counter() - t0)
        return red.extend_basis_pod(stacked, modes=modes)

    cases = [('hapod keep {} {}'.format(keep, 'k_pod_xt route' if valu else 'MFMA rotate'), hapod(keep, valu))
             for keep in (64, 32) for valu in (0, 1)] + [('pod, stacked, 128-column calls', pod)]
    times = {name: [] for name, _ in cases}
    facts = {}
    for rep in range(WARM + REPS):
        for name, fn in cases:                                   # alternated
            reset()
            with CopyCounter() as cc:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                sv, added = fn()
                torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if rep >= WARM:
                times[name].append(dt)
            if name not in facts:
                pushes = red.last_pod_info['nodes'] if name.startswith('hapod') else -(-columns // 128)
                facts[name] = dict(copies=cc.count, added=(int(added.min()), int(added.max())), width=red.basis_size(), pushes=pushes,
                                   error=projection_error2(red, slabs),
                                   lost=float(red.last_pod_info['lost'].sum()) if name.startswith('hapod') else None)
    say('{}: {}'.format(tag, desc))
    for name, _ in cases:
        ts, f = times[name], facts[name]
        say('  {:34s} median ms {:9.3f}  min ms {:9.3f}  max ms {:9.3f}  per push / call ms {:8.3f} ({} of them)  device-to-host copies {}'
            '  vectors appended {} .. {} (slab width {})  projection error^2 of the set {:.6e}{}'.format(
                name, 1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts), 1e3 * statistics.median(ts) / f['pushes'], f['pushes'],
                f['copies'], f['added'][0], f['added'][1], f['width'], f['error'],
                '' if f['lost'] is None else '  (reported bound, sum of lost: {:.6e}; on the deflated set)'.format(f['lost'])))
    say('  torch.cat of the {} columns for the pod route: median ms {:.3f} (inside its time above)'.format(
        columns, 1e3 * statistics.median(cat_times[WARM:])))
    for keep in (64, 32):
        a, b = times['hapod keep {} MFMA rotate'.format(keep)], times['hapod keep {} k_pod_xt route'.format(keep)]
        say('  keep {}: MFMA rotate / k_pod_xt route (medians) {:.3f}; the slowest MFMA repetition is {} the fastest of the k_pod_xt route'.format(
            keep, statistics.median(a) / statistics.median(b), 'faster than' if max(a) < min(b) else 'NOT faster than'))
    # per kernel: a short stream under the event timing
    P = red._pod_product()
    for keep in (64, 32):
        for valu in (0, 1):
            reset()
            pad = torch.nn.functional.pad(red._V, (0, max(0, red._pod_width(1 + modes) - red._V.shape[2]))).contiguous()
            nloc = torch.as_tensor(np.ascontiguousarray(red._nloc[:eng.S], dtype=np.int32)).to(pad.device)
            ctx.set_option('pod_rotate_valu', valu)
            stream = ctx.local_pod_stream(P, pad, nloc, keep=keep, cmax=128 - keep)
            for u in slabs[:2]:                                  # warm: fill the carried panel
                stream.push(u)
            torch.cuda.synchronize()
            ctx.kernel_timing(True)
            for u in slabs[2:6]:
                stream.push(u)
            nodes = stream.nodes
            per = {}
            for k, ms in ctx.kernel_timing_read(2048):
                per.setdefault(k, [0, 0.0])
                per[k][0] += 1
                per[k][1] += ms
            stream.finish(modes)
            fin = {}
            for k, ms in ctx.kernel_timing_read(2048):
                fin.setdefault(k, [0, 0.0])
                fin[k][0] += 1
                fin[k][1] += ms
            ctx.kernel_timing(False)
            ctx.set_option('pod_rotate_valu', 0)
            pushes = nodes - 2
            say('  keep {} {}: per push, per kernel (events on the stream over {} pushes of {} columns; the product applies and the '
                'copies are not bracketed):'.format(keep, 'k_pod_xt route' if valu else 'MFMA rotate', pushes, int(slabs[2].shape[2])))
            for k, (cnt, ms) in sorted(per.items(), key=lambda kv: -kv[1][1]):
                say('    {:24s} launches per push {:5.1f}  ms per push {:8.3f}'.format(k, cnt / pushes, ms / pushes))
            say('    finish: ' + ', '.join('{} x{} {:.3f} ms'.format(k, cnt, ms) for k, (cnt, ms) in sorted(fin.items(), key=lambda kv: -kv[1][1])))
    reset()


def config3():
    from pylrbms_amd import multiscale_problem
    from pylrbms_amd.discretize_parabolic_block_swipdg import discretize
    from pylrbms_amd.reductor import ParabolicLRBMSReductor
    p = multiscale_problem.init_grid_and_problem({'num_subdomains': [32, 32], 'coarse_per_subdomain': 4})
    d, data = discretize(p, 0.05, 40)
    mus = [d.parse_parameter(float(v)) for v in np.random.default_rng(7).uniform(0.1, 1.0, 64)]
    torch.cuda.synchronize(); t0 = time.perf_counter()
    slabs = d.solve_batch(mus, as_snapshots='slabs')
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    red = ParabolicLRBMSReductor(
        d, products=[d.operators['local_energy_dg_product_{}'.format(ii)] for ii in range(data['block_space'].num_blocks)])
    run('config 3', red, slabs, 16, 'S {} n {} slabs {} x {} columns (solve_batch {:.1f} s) modes 16 (2D, P1)'.format(
        d.engine.S, d.engine.t.n, len(slabs), int(slabs[0].shape[2]), dt))


def config5():
    from pylrbms_amd import multiscale_problem3d
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D, discretize
    p = multiscale_problem3d.init_grid_and_problem({'num_subdomains': (8, 8, 8), 'cubes_per_subdomain': 4})
    d, _ = discretize(p, 0.1, 10)
    mus = [float(v) for v in np.random.default_rng(7).uniform(0.1, 1.0, 64)]
    torch.cuda.synchronize(); t0 = time.perf_counter()
    slabs = d.solve_batch(mus, as_snapshots='slabs')
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    red = ParabolicLRBMSReductor3D(d)
    run('config 5', red, slabs, 8, 'S {} n {} slabs {} x {} columns (solve_batch {:.1f} s) modes 8 (3D, P2)'.format(
        d.engine.S, d.engine.t.n, len(slabs), int(slabs[0].shape[2]), dt))


which = sys.argv[1] if len(sys.argv) > 1 else 'both'
say('# python tools/local_pod_stream_time.py {}: {} untimed and {} timed repetitions of each, alternated'.format(which, WARM, REPS))
if which in ('2d', 'both'):
    config3()
if which in ('3d', 'both'):
    config5()
os.makedirs('profiles', exist_ok=True)
out = os.path.join('profiles', 'local_pod_stream_time.txt' if which == 'both' else 'local_pod_stream_time_{}.txt'.format(which))
with open(out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
