"""Times the incremental re-projection of the 3D / P2 path against the whole project+estimate pass of the same
session (config 5 by default: 8x8x8 subdomains, k_c 4, N = 30 real vectors on the slab width the enrichment loop reserves).

Cases: the whole pass; the pass restricted (lrbms3_pass_set_subset) to 16 scattered changed subdomains, to 16 changed subdomains
forming one 2 x 2 x 4 block, to 1 changed subdomain, and to all of them (which must cost what the whole pass costs); the whole
pass again at the end (drift of the session).  Per case: own and side counts, the K-split the library chooses per kernel (the rule
of lrbms3_project_estimate_phase restated below), milliseconds per pass by device events around a window of passes after warm-up
passes (best of 3 windows, and the slowest), the same for one ``Engine3D.project_and_estimate(subset=)`` call -- which also sets
and lifts the restriction, what a round of the loop pays --, and the per-kernel times of one serial pass.
usage: reproject3d_time.py [P] [kc] [N] [reserve] [output file]"""
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from pylrbms_amd import multiscale_problem3d  # noqa: E402
from pylrbms_amd.engine3d import Engine3D  # noqa: E402
from pylrbms_amd.grid3d import side_targets  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 8
kc = int(sys.argv[2]) if len(sys.argv) > 2 else 4
N = int(sys.argv[3]) if len(sys.argv) > 3 else 30
reserve = int(sys.argv[4]) if len(sys.argv) > 4 else 8          # AdaptiveEnrichment.solve without a step limit reserves 8
path = sys.argv[5] if len(sys.argv) > 5 else None
WARMUP, WINDOW, REPS = 3, 50, 3

p = multiscale_problem3d.init_grid_and_problem({'num_subdomains': (P, P, P), 'cubes_per_subdomain': kc})
eng = Engine3D(p['grid'], p['lambda']['functions'], p['f'], p['lambda_bar'], p['lambda_hat']).assemble()
c, S, Q = eng.ctx, eng.S, eng.Q
width = min(N + reserve + ((N + reserve) & 1), 64 // Q)         # LRBMSReductor3D.reserve: even, at most 64 // Q
lines = []


def say(*a):
    line = ' '.join(str(x) for x in a)
    print(line, flush=True)
    lines.append(line)


say('S', S, 'n', eng.t.n, 'Q', Q, 'N', N, 'real vectors on a slab of width', width, '| windows of', WINDOW, 'passes after', WARMUP,
    'warm-up passes, best / slowest of', REPS)
gen = torch.Generator(device='cuda').manual_seed(1)
V = torch.zeros(eng.S_ext, eng.t.n, width, dtype=torch.float64, device='cuda')
V[:, :, :N] = torch.randn(eng.S_ext, eng.t.n, N, dtype=torch.float64, device='cuda', generator=gen)
out, work = eng.alloc_outputs(width), eng.alloc_work(width)


def ksplit(nblocks, target):
    """``ksplit_of`` of lrbms3_project_estimate_phase (csrc/lrbms3d.hip) at LRBMS3_OPT_KSPLIT 0."""
    if nblocks <= 0 or nblocks >= 384:
        return 1
    return max(1, min(8, (target + nblocks - 1) // nblocks))


def ksplits(n_own, n_side):
    npair = Q * (Q + 1) // 2
    return dict(SYS=ksplit(Q * n_own, 512), AAA=ksplit(npair * n_own, 768), NC=ksplit(n_own, 256), AB=ksplit(Q * n_own, 512),
                BB=ksplit(n_own, 256), CPL=ksplit(6 * Q * n_side, 512))


def windows(fn, per_window):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_window):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / per_window)
    return min(ms), max(ms)


def measure(label, changed):
    own = S if changed is None else len(changed)
    side = S if changed is None else len(side_targets(eng.nbr, changed))
    c.pass_set_subset(changed)
    try:
        best, worst = windows(lambda: c.project_estimate(Q, V, eng.ops, work, out), WINDOW)
        c.kernel_timing(True)
        c.project_estimate(Q, V, eng.ops, work, out)
        kern = c.kernel_timing_read()
        c.kernel_timing(False)
    finally:
        c.pass_set_subset(None)
    call = windows(lambda: eng.project_and_estimate(V, out, work, subset=changed), 1) if changed is not None else (best, worst)
    say('{:<28} own {:>3} side {:>3} | pass {:.3f} ms (slowest window {:.3f}) | one call with set / lift {:.3f} ms (slowest {:.3f}) | '
        'K-split {}'.format(label, own, side, best, worst, call[0], call[1], ' '.join('{} {}'.format(k, v) for k, v in
                                                                                     ksplits(own, side).items())))
    say('    serial pass, us per kernel: ' + ', '.join('{} {:.0f}'.format(k, 1e3 * v) for k, v in kern))
    return best


idx = np.arange(S).reshape(P, P, P)                              # [z, y, x]: subdomain = x + P (y + P z)
step = max(S // 16, 1)
whole = measure('whole pass', None)
res = {
    '16 scattered': measure('16 scattered', list(range(0, S, step))[:16]),
    '16 as one 2x2x4 block': measure('16 as one 2x2x4 block', sorted(int(v) for v in idx[2:6, 2:4, 2:4].ravel()) if P >= 6 else
                                     sorted(int(v) for v in idx[:4, :2, :2].ravel())),
    '1 changed': measure('1 changed', [int(idx[P // 2, P // 2, P // 2])]),
    'all {} changed'.format(S): measure('all {} changed'.format(S), list(range(S))),
}
again = measure('whole pass (again)', None)
say('whole pass at the start / at the end of the session: {:.3f} / {:.3f} ms'.format(whole, again))
for k, v in res.items():
    say('{:<28} {:.3f} ms = {:.3f} of the whole pass'.format(k, v, v / whole))
if width != N:                                                   # the whole pass on the slab without the reserved columns
    Vn = V[:, :, :N].contiguous()
    on, wn = eng.alloc_outputs(N), eng.alloc_work(N)
    best, worst = windows(lambda: c.project_estimate(Q, Vn, eng.ops, wn, on), WINDOW)
    say('whole pass at width {} (no reserved columns): {:.3f} ms (slowest window {:.3f})'.format(N, best, worst))
if path:
    with open(path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
