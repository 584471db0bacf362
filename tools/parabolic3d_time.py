"""Times the parabolic 3D / P2 path (config 5 by default: 8x8x8 subdomains, k_c 4, N 30, nt 10): full-order implicit Euler,
reduced implicit Euler, both estimates, and the two streaming kernels (project_mass, mass_inverse_norm2) by HIP events.
usage: parabolic3d_time.py [P] [kc] [N] [NT]"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from pylrbms_amd import multiscale_problem3d  # noqa: E402
from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D, discretize  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 8
kc = int(sys.argv[2]) if len(sys.argv) > 2 else 4
N = int(sys.argv[3]) if len(sys.argv) > 3 else 30
nt = int(sys.argv[4]) if len(sys.argv) > 4 else 10
p = multiscale_problem3d.init_grid_and_problem({'num_subdomains': (P, P, P), 'cubes_per_subdomain': kc})
d, _ = discretize(p, 0.1, nt)
eng = d.engine
mu = 0.5
print('S', eng.S, 'n', eng.t.n, 'Q', d.Q, 'nt', nt, flush=True)


def timed(fn, reps=2):
    best, out = 1e9, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return out, best


def kernel_ms(fn, reps=10):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


U, t = timed(lambda: d.solve(mu))
it, res = d.last_solve_info
print('FOM implicit Euler: {:.4f} s, {:.1f} steps/s, {:.1f} CG iterations per step, worst residual {:.1e}'.format(
    t, nt / t, it / nt, res), flush=True)
(est, parts), t = timed(lambda: d.estimate(U, mu), reps=1)
print('FOM parabolic estimate: {:.4f} s, est {:.6e}'.format(t, est), flush=True)
reductor = ParabolicLRBMSReductor3D(d)
reductor.extend_basis(U[:, :, 1:])
g = torch.Generator(device=U.device).manual_seed(0)
while reductor.basis_size() < N:           # fill up with random vectors so that the reduced model has the bench size
    reductor.extend_basis(torch.randn(eng.S, eng.t.n, 1, dtype=torch.float64, device=U.device, generator=g))
rd, t = timed(lambda: reductor.reduce())
print('N', reductor.basis_size(), 'reduce (pass + project_mass): {:.4f} s'.format(t), flush=True)
u, t = timed(lambda: rd.solve(mu))
it, res = rd.last_solve_info
print('reduced implicit Euler: {:.5f} s, {:.1f} trajectories/s, {:.1f} PCG iterations per step, worst residual {:.1e}'.format(
    t, 1.0 / t, it / nt, res), flush=True)
(est_r, parts_r), t = timed(lambda: rd.estimate(u, mu))
print('reduced parabolic estimate: {:.5f} s, est {:.6e}'.format(t, est_r), flush=True)
V = reductor.bases.contiguous()
ms = kernel_ms(lambda: eng.ctx.project_mass(V))
nbytes = V.numel() * 8 + eng.S * N * N * 8
print('project_mass: {:.4f} ms, {:.1f} MB -> {:.2f} TB/s = {:.2f} of 6.3 TB/s'.format(ms, nbytes / 1e6, nbytes / ms / 1e9,
                                                                                    nbytes / ms / 1e9 / 6.3), flush=True)
Y = torch.randn(eng.S, eng.t.n, nt, dtype=torch.float64, device=U.device, generator=g)
ms = kernel_ms(lambda: eng.ctx.mass_inverse_norm2(Y))
nbytes = Y.numel() * 8 + eng.S * nt * 8
print('mass_inverse_norm2 (L = {}): {:.4f} ms, {:.1f} MB -> {:.2f} TB/s = {:.2f} of 6.3 TB/s'.format(
    nt, ms, nbytes / 1e6, nbytes / ms / 1e9, nbytes / ms / 1e9 / 6.3), flush=True)
