"""Bench leg of BASELINE.json config 5 (3D diffusion, 8 x 8 x 8 subdomains, SWIPDG p = 2, local basis dim 30) -- used by
bench.py (`--config cfg5` prints its line; a `--full` run of config 3 carries it as the `config5` object).

A step is one pass of the 3D project+estimate path (lrbms3_project_estimate) over all subdomains of this rank on synthetic
data (pylrbms_amd/multiscale_problem3d.py, constant + seeded random basis columns resident in HBM).  One GPU holds the whole
8 x 8 x 8 configuration (0.47 GB of bases, 2.6 GB of assembled element blocks).

`run(full=False)` (a plain bench run) does only what the headline figure needs; `full=True` adds the per-kernel table, the
roofline and the assembly time (the CPU baseline and the online legs have switches of their own).

Roofline of the dominant kernel: executed fp64-MFMA flops (padding included, counted from the kernel's own tile shapes) over
its HIP-event duration against 78.6 TFLOP/s; compulsory HBM bytes of the pass (inputs once + outputs once) beside it."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CONFIGS3D = {
    'cfg5': {'num_subdomains': (8, 8, 8), 'cubes_per_subdomain': 4, 'N': 30},
    'cfg5_tile8': {'num_subdomains': (4, 4, 4), 'cubes_per_subdomain': 4, 'N': 30},   # what one rank of the 8-GPU run holds
}
PEAK_HBM_GBS = 8000.0
PEAK_FP64_MFMA_TFLOPS = 78.6
MFMA_FLOPS = 2 * 16 * 16 * 4


def mfma_counts(t, N, Q):
    """Executed v_mfma_f64_16x16x4 per subdomain and kernel of the pass (k3_pg<KIND>: per item KS * CT apply steps +
    RT * KR * CT projection steps; csrc/lrbms3d.hip)."""
    tn, tq = (N + 15) // 16, (Q * N + 15) // 16
    n_T, ncf = t.n_T, t.ncf
    nsl = 1 + (t.up_face >= 0).sum(axis=1)                                  # slots read per element in the symmetric form of B_sys
    sys_steps = int((2 * nsl + (nsl + 1) // 2).sum())
    per = {'k3_pg<SYS>': (sys_steps * tn + tn * 3 * tn * n_T) * Q,
           'k3_pg<CPL>': (3 * tn + tn * 3 * tn) * ncf * 6 * Q,
           'k3_pg<AAA>': (3 * tn + tn * 3 * tn) * n_T * (Q * (Q + 1) // 2),      # pairs q <= q', mirrored at the store
           'k3_pg<NC>': (3 * tn + tn * 3 * tn) * n_T,
           'k3_pg<AB>': (3 * tn + tn * tq) * n_T * Q,                              # contracted through the four faces
           'k3_pg<BB>': 2 * (tq + tq * (tq + 1) // 2) * n_T}                     # G_bb and G_rdd: apply + upper tile triangle each
    return per


def compulsory_bytes(t, S, N, Q):
    """Every input of the pass once and every output once (bytes)."""
    QN = Q * N
    inputs = S * 8 * (t.n * N + t.n_T * (Q * 500 + 100 + Q * Q * 100 + Q * 40 + 16 + 1 + Q * 40) + Q * 6 * t.ncf * 100 + t.n)
    outputs = S * 8 * (Q * 7 * N * N + N + N * N + 2 * QN * QN + Q * N * QN + Q * Q * N * N + QN + 3 * t.nbf * QN + Q * t.nbf * N +
                       6 * t.nvs * N + t.nb * N)
    return inputs, outputs


_POOL3 = {}


def _pool_reduce3(chunk):
    from oracle.lrbms3d import Reductor3D
    Reductor3D(_POOL3['d'], _POOL3['V']).reduce(subdomains=chunk)
    return len(chunk)


def cpu_baseline3d(N):
    """The 3D oracle's Reductor3D.reduce() (NumPy / SciPy) on a 2 x 2 x 2 sample of the same problem (k_c = 4, N as config 5),
    timed before the process touches the GPU: one process, and the target subdomains farmed over a fork()ed pool on the host cores
    the process may use (as bench.py does for config 3).  Why not 4 x 4 x 4: the oracle ASSEMBLES its global sparse operators in
    Python (21 s for 2 x 2 x 2, 76 s for 3 x 3 x 3, ~3 min for 4 x 4 x 4: untimed, but inside a --full bench run), and its
    rate per target subdomain barely depends on the sample (1.4 / s at 2 x 2 x 2, 1.0 / s at 3 x 3 x 3 on one core here)."""
    import multiprocessing as mp
    from threadpoolctl import threadpool_limits
    from bench import host_cores
    from oracle.lrbms3d import Discretization3D, Reductor3D
    from oracle.mesh3d import KuhnMesh3D
    from pylrbms_amd import multiscale_problem3d
    P = (2, 2, 2)
    p = multiscale_problem3d.init_grid_and_problem({'num_subdomains': P, 'cubes_per_subdomain': 4})
    lam = p['lambda']
    t0 = time.perf_counter()
    d = Discretization3D(KuhnMesh3D(np.array(P) * 4, P), lam['functions'], lam['coefficients'], np.eye(3), p['f'], p['lambda_bar'],
                         p['lambda_hat'], 1.0, 1.0)
    t_asm = time.perf_counter() - t0
    rng = np.random.default_rng(0)
    V = [np.hstack([np.ones((d.n, 1)), rng.standard_normal((d.n, N - 1))]) for _ in range(d.S)]
    hc = host_cores()
    workers = max(1, min(hc['cores'], d.S))
    with threadpool_limits(limits=1):
        t0 = time.perf_counter()
        Reductor3D(d, V).reduce()
        one = d.S / (time.perf_counter() - t0)
        _POOL3['d'], _POOL3['V'] = d, V
        chunks = [[ii] for ii in range(d.S)]
        with mp.get_context('fork').Pool(workers) as pool:
            pool.map(_pool_reduce3, chunks[:workers])                     # start-up of the workers is not timed
            t0 = time.perf_counter()
            pool.map(_pool_reduce3, chunks)
            allc = d.S / (time.perf_counter() - t0)
    _POOL3.clear()
    return {'value': allc, 'unit': 'subdomains/s', 'cores': workers, 'kind': 'port', 'value_1core': one,
            'assemble_subdomains_per_s_1core': d.S / t_asm,
            'sample': 'oracle.lrbms3d.Reductor3D.reduce() (NumPy/SciPy fp64) on 2x2x2 subdomains of the same synthetic 3D problem '
                      '(k_c = 4, n = 3840, N = {}): value = the 8 target subdomains farmed over a {}-process pool (1 BLAS thread '
                      'each), value_1core = one process; timed before the GPU is touched.  A 4x4x4 sample would add ~3 min of '
                      'untimed oracle assembly (Python) to a --full bench run; the per-subdomain rate barely depends on the '
                      'sample size'.format(N, workers),
            'os_cpu_count': hc['os_cpu_count'], 'affinity': hc['affinity'], 'cgroup_quota': hc['cgroup_quota']}


def run(config='cfg5', steps=10, warmup=2, device_index=0, cpu=True, online=True, world=1, rank=0, backend='nccl', options=None,
        full=True):
    """One rank of the config-5 bench.  world > 1 (launched by torch.distributed.run): the 8 x 8 x 8 subdomains are cut into
    one 3D tile per rank (strong scaling, as BASELINE.json config 5 asks for 8 GPUs), every step = one halo exchange of the
    neighbour rows (all_to_all_single over RCCL, point to point) + one pass; rank 0 returns the line, the others None."""
    cfg = CONFIGS3D[config]
    N = cfg['N']
    base = cpu_baseline3d(N) if (cpu and world == 1) else None
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    import torch
    import torch.distributed as dist
    from pylrbms_amd import multiscale_problem3d
    from pylrbms_amd.engine3d import Engine3D
    torch.cuda.set_device(device_index)
    if world > 1:
        if backend == 'nccl':
            from pylrbms_amd.parallel import init_rccl
            init_rccl(torch.device('cuda', device_index))
        else:
            dist.init_process_group(backend)
    pcfg = {'num_subdomains': cfg['num_subdomains'], 'cubes_per_subdomain': cfg['cubes_per_subdomain']}
    p = multiscale_problem3d.init_grid_and_problem(pcfg, rank=rank, world_size=world)
    lam = p['lambda']
    t0 = time.perf_counter()
    eng = Engine3D(p['grid'], lam['functions'], p['f'], p['lambda_bar'], p['lambda_hat'], data_degree=p['data_degree'],
                   device_index=device_index)
    setup_s = time.perf_counter() - t0
    for name, value in (options or {}).items():
        eng.ctx.set_option(name, value)
    eng.assemble()
    torch.cuda.synchronize()
    if full:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.assemble()
        e1.record()
        torch.cuda.synchronize()
        assemble_ms = e0.elapsed_time(e1)
    t, S, Q = eng.t, eng.S, eng.Q
    S_total = p['grid'].num_subdomains
    g = torch.Generator(device='cuda').manual_seed(rank)
    V = torch.zeros(eng.S_ext, t.n, N, dtype=torch.float64, device='cuda')
    V[:S] = torch.randn(S, t.n, N, dtype=torch.float64, device='cuda', generator=g)
    V[:S, :, 0] = 1.0
    halo = None
    if world > 1:
        from pylrbms_amd.grid3d import DDSubdomainsGrid3D
        from pylrbms_amd.parallel import HaloExchange, HaloPlan
        gr = p['grid']
        plan = HaloPlan(lambda r: DDSubdomainsGrid3D(gr.lower_left, gr.upper_right, gr.K, gr.P, rank=r, world_size=world), world, rank)
        halo = HaloExchange(plan, N, V.device)
    out, work = eng.alloc_outputs(N), eng.alloc_work(N)

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # an untimed loop of the same passes runs FIRST (with `full`, its last K passes are the per-kernel timing leg): after the
    # host-side setup above the device needs ~18 ms of work to reach its steady clocks (tools/ramp_time.py); the timed region is
    # W warm-up + exactly K passes behind it
    for _ in range(max(0, 10 - steps)):
        eng.project_and_estimate(V, out, work, halo=halo)
    if full:
        eng.ctx.kernel_timing(True)
    for _ in range(steps):
        eng.project_and_estimate(V, out, work)
    if full:
        rows = eng.ctx.kernel_timing_read()
        eng.ctx.kernel_timing(False)
    fence()
    for _ in range(warmup):
        eng.project_and_estimate(V, out, work, halo=halo)
    fence()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        eng.project_and_estimate(V, out, work, halo=halo)
    e1.record()
    fence()
    elapsed = time.perf_counter() - t0
    dev_ms = e0.elapsed_time(e1) / steps
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=V.device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    # the timed passes left their results in `out`: every array finite, one checksum per run on record (same seed => same value)
    bad = [k for k, v in out.items() if not bool(torch.isfinite(v).all())]
    if bad:
        raise RuntimeError('config-5 pass produced non-finite values in {}'.format(bad))
    checksum = {k: float(v.sum()) for k, v in out.items()}
    checksum['all'] = float(sum(checksum.values()))
    roofline = None
    if full:
        agg = {}
        for name, v in rows:
            agg.setdefault(name, []).append(v)
        counts = mfma_counts(t, N, Q)
        table = []
        for name, v in sorted(agg.items(), key=lambda kv: -np.mean(kv[1])):
            us = 1e3 * float(np.mean(v))
            row = {'name': name, 'us': us}
            if name in counts:
                fl = counts[name] * S * MFMA_FLOPS
                row.update(mfma_flops=fl, mfma_TFLOPs=fl / (us * 1e-6) / 1e12, mfma_frac=fl / (us * 1e-6) / 1e12 / PEAK_FP64_MFMA_TFLOPS)
            table.append(row)
        inputs, outputs = compulsory_bytes(t, S, N, Q)
        dense_us = sum(r['us'] for r in table if 'mfma_flops' in r)
        dense_fl = sum(r['mfma_flops'] for r in table if 'mfma_flops' in r)
        dom = table[0]
        roofline = {'bound': 'mfma' if 'mfma_frac' in dom else 'hbm', 'unit': 'TFLOP/s' if 'mfma_frac' in dom else 'GB/s',
                    'achieved': dom.get('mfma_TFLOPs'), 'peak': PEAK_FP64_MFMA_TFLOPS, 'frac': dom.get('mfma_frac'), 'traffic': None,
                    'kernel': dom['name'], 'kernel_us': dom['us'],
                    'basis': 'executed fp64-MFMA flops of the dominant kernel (padding included) / its HIP-event duration',
                    'dense_kernels': {'us': dense_us, 'mfma_flops': dense_fl, 'TFLOPs': dense_fl / (dense_us * 1e-6) / 1e12,
                                      'frac': dense_fl / (dense_us * 1e-6) / 1e12 / PEAK_FP64_MFMA_TFLOPS},
                    'compulsory_bytes': inputs + outputs, 'compulsory_input_bytes': inputs, 'compulsory_output_bytes': outputs,
                    'compulsory_GBps': (inputs + outputs) / (dev_ms * 1e-3) / 1e9,
                    'compulsory_frac_of_hbm_peak': (inputs + outputs) / (dev_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                    'device_ms_per_step': dev_ms, 'kernels': table, 'kernels_sum_us': sum(r['us'] for r in table)}
        # measured HBM traffic per launch from the committed rocprofv3 PMC passes of this configuration (FETCH_SIZE x 2 + WRITE_SIZE as the
        # guide prescribes for gfx950; separate --pmc runs, tools/cfg5_pmc.sh): profiles/rNN_cfg5_pmc_traffic.json
        if world == 1:
            import glob
            import json as _json
            for path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', 'r*_pmc_traffic.json')), reverse=True):
                try:
                    doc = _json.load(open(path))
                except (OSError, ValueError):
                    continue
                if doc.get('config') != config:
                    continue
                from pylrbms_amd._build import source_sha
                if doc.get('csrc_sha') != source_sha():       # a profile speaks for the kernels it was taken from: look for this build's
                    roofline.setdefault('traffic_source', '{} (withheld: the kernel sources changed since that profile was taken)'.format(
                        os.path.join('profiles', os.path.basename(path))))
                    continue
                for r in table:
                    if r['name'] in doc['per_kernel']:
                        r['pmc_bytes'] = doc['per_kernel'][r['name']]['bytes']
                if dom['name'] in doc['per_kernel']:
                    roofline['traffic'] = doc['per_kernel'][dom['name']]['bytes']
                    roofline['traffic_GBps'] = roofline['traffic'] / (dom['us'] * 1e-6) / 1e9
                    roofline['traffic_frac_of_hbm_peak'] = roofline['traffic_GBps'] / PEAK_HBM_GBS
                roofline['traffic_per_pass'] = doc['per_pass_bytes']
                roofline['traffic_over_compulsory'] = doc['per_pass_bytes'] / (inputs + outputs)
                roofline['traffic_source'] = os.path.join('profiles', os.path.basename(path))
                break
    mine = [float(S), float(len(eng.halo)), float(halo.send_bytes if halo is not None else 0), float(halo.recv_bytes if halo is not None else 0)]
    if world > 1:
        gathered = [torch.zeros(4, dtype=torch.float64, device=V.device) for _ in range(world)]
        dist.all_gather(gathered, torch.tensor(mine, dtype=torch.float64, device=V.device))
        rows_d = [x.cpu().tolist() for x in gathered]
    else:
        rows_d = [mine]
    dist_info = {'backend': backend if world > 1 else None, 'world_size': dist.get_world_size() if world > 1 else 1,
                 'subdomains_per_rank': [int(r[0]) for r in rows_d], 'halo_subdomains_per_rank': [int(r[1]) for r in rows_d],
                 'halo_bytes_sent_per_rank_per_step': [int(r[2]) for r in rows_d],
                 'halo_bytes_received_per_rank_per_step': [int(r[3]) for r in rows_d]}
    if world > 1:
        online = False
    res = {'metric': 'offline project+estimate throughput', 'value': S_total * steps / elapsed, 'unit': 'subdomains/s', 'n_gpus': world,
           'steps': steps, 'warmup': warmup, 'ms_per_step': 1e3 * elapsed / steps, 'higher_is_better': True,
           'scaling': 'strong' if world > 1 else 'weak',
           'vs_baseline': None, 'dtype': 'f64', 'data': 'synthetic',
           'config': {'workload': 'BASELINE.json config 5{}: 3D diffusion, {}x{}x{} subdomains, SWIPDG p=2 on Kuhn tetrahedra, k_c={} '
                                  '(n={} DG DoFs, n_rt={} RT0 DoFs per subdomain), Q={}, local basis dim {}'.format(
                                      '' if config == 'cfg5' else ' (per-rank tile of the 8-GPU run)', *cfg['num_subdomains'],
                                      cfg['cubes_per_subdomain'], t.n, t.n_rt, Q, N),
                      'subdomains': S_total, 'N': N, 'Q': Q,
                      'parallelism': 'one rank holds every subdomain' if world == 1 else '3D subdomain tiles x{}'.format(world)},
           'distributed': dist_info, 'output_checksum': checksum}
    if full:
        res['roofline'] = roofline
        res['assemble'] = {'ms': assemble_ms, 'value': S / (1e-3 * assemble_ms), 'unit': 'subdomains/s', 'host_sampling_and_upload_s': setup_s}
    if online:
        # online phase on the same reduced model: 256 parameters in batches of 16, then their estimates one by one
        mus = np.random.default_rng(7).uniform(0.1, 1.0, size=256)
        thetas = np.stack([np.array([1.0, float(m)]) for m in mus])
        nper = 64      # parameters per native call (groups of 16 on the caller's + the side streams)
        eng.ctx.reduced_precond_use(eng.ctx.reduced_precond_build(Q, np.array([1.0, 0.55]), out['B_sys']))    # warm-up (rocSOLVER, too)
        eng.ctx.reduced_solve_batch(Q, thetas[:nper], out['B_sys'], out['rhs_red'], rtol=1e-12)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        iters, worst = 0, 0.0
        pc = eng.ctx.reduced_precond_build(Q, np.array([1.0, 0.55]), out['B_sys'])       # once per reduced model: inside the timed region
        eng.ctx.reduced_precond_use(pc)
        torch.cuda.synchronize()
        t_pc = time.perf_counter() - t0
        for b0 in range(0, len(mus), nper):
            ub, binfo = eng.ctx.reduced_solve_batch(Q, thetas[b0:b0 + nper], out['B_sys'], out['rhs_red'], rtol=1e-12)
            iters, worst = max(iters, binfo[0]), max(worst, binfo[1])
        torch.cuda.synchronize()
        t_batch = time.perf_counter() - t0
        eng.ctx.reduced_precond_use(None)
        th = np.array([1.0, 0.5])
        u, info = eng.reduced_solve(th, out, rtol=1e-12, max_iter=20000)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nrep = 8
        for k in range(nrep):
            u, info = eng.reduced_solve(np.array([1.0, 0.1 + 0.1 * k]), out, rtol=1e-12, max_iter=20000)
        torch.cuda.synchronize()
        t_solve = (time.perf_counter() - t0) / nrep
        t0 = time.perf_counter()
        for k in range(nrep):
            eng.reduced_estimate(th, u, out)
        torch.cuda.synchronize()
        t_est = (time.perf_counter() - t0) / nrep
        ub = ub[:, :, :16].contiguous() if ub.shape[2] >= 16 else ub.repeat(1, 1, 16)[:, :, :16].contiguous()
        eng.ctx.reduced_estimate_batch(Q, thetas[:16], ub, out, eng.ops, eng.hdiam)                      # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b0 in range(0, len(mus), 16):       # the solutions of the last batch stand in for all (same work)
            eng.ctx.reduced_estimate_batch(Q, thetas[b0:b0 + 16], ub, out, eng.ops, eng.hdiam)
        torch.cuda.synchronize()
        t_estb = time.perf_counter() - t0
        res['online'] = {'metric': 'online reduced solves (O1)', 'value': len(mus) / t_batch, 'unit': 'mu-solves/s',
                         'parameters': len(mus), 'batch': nper, 'single_parameter_solves_per_s': 1.0 / t_solve,
                         'estimates_per_s': len(mus) / t_estb, 'single_parameter_estimates_per_s': 1.0 / t_est,
                         'solve_plus_estimate_per_s': len(mus) / (t_batch + t_estb), 'reduced_dim': S * N, 'cg_iterations_max': iters,
                         'relative_residual_max': worst,
                         'preconditioner_build_ms': 1e3 * t_pc,
                         'solver': 'PCG on the 7-slot block-sparse reduced system, rtol 1e-12, 64 parameters per call (four groups of 16 on four streams) '
                                   '(lrbms3_reduced_solve_batch: every projected block read once per iteration for the batch), '
                                   'preconditioner = inverse diagonal blocks + coarse level on the first local basis vectors, built '
                                   'once at mu = 0.55 (time included in value)'}
    if online:
        # snapshot generation: one full-order solve (two-level CG on the never-assembled block operator: element blocks + P1 per subdomain)
        try:
            fwork = eng.ctx.empty(int(eng.ctx.lib.lrbms3_fom_solve_work_size(eng.ctx.handle)))
            fms = []
            for rep, mu_s in enumerate((0.55, 0.55, 0.5)):
                # 0: warm-up (creates the rocBLAS handle, loads rocSOLVER's kernels); 1: a solve that factorises its coarse matrix and
                # keeps the inverse (d.solve does that for the first snapshot); 2: another parameter with the kept inverse
                if rep == 1:
                    eng.ctx.fom_precond_keep(True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, finfo = eng.ctx.fom_solve(Q, np.array([1.0, mu_s]), eng.ops['A_diag'], eng.ops['A_cpl'], eng.ops['b'], rtol=1e-8,
                                             max_iter=20000, work=fwork)
                torch.cuda.synchronize()
                fms.append(1e3 * (time.perf_counter() - t0))
            eng.ctx.fom_precond_keep(False)
            del fwork
            res['snapshot'] = {'metric': 'full-order solve (d.solve)', 'ms': fms[2], 'first_snapshot_ms': fms[1], 'dofs': S * t.n,
                               'cg_iterations': finfo[0], 'relative_residual': finfo[1], 'rtol': 1e-8,
                               'preconditioner': 'inverse 10x10 element blocks + Galerkin coarse level on P1 per subdomain; the dense '
                                                 'coarse inverse is factorised by the first snapshot (first_snapshot_ms) and kept for '
                                                 'the others (ms: another parameter)'}
        except Exception as exc:                      # reported, not fatal for the bench line
            res['snapshot'] = {'error': str(exc)}
    if base is not None:
        res['cpu_baseline'] = base
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return res if rank == 0 else None


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='cfg5', choices=sorted(CONFIGS3D))
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--full', action='store_true', help='also the CPU baseline, the per-kernel table, the roofline, assembly and the online legs')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='skip the CPU baseline of a --full run')
    a = ap.parse_args()
    print(json.dumps(run(a.config, a.steps, a.warmup, cpu=a.full and not a.no_cpu_baseline, online=a.full, full=a.full)), flush=True)
