"""bench.py --dump-outputs: the outputs of the last timed step as .npy files, so that two builds run with the same arguments
can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_buffers(S, Q, N, ncf, nvs, seed=5):
    """CPU tensors in the factored layout of ``Engine.alloc_outputs``, every entry distinct."""
    g = torch.Generator().manual_seed(seed)
    QN, C = Q * N, 5 * Q * N
    shapes = {'sys': [(Q, S, 5, N, N), (S, N), (S, N, N), (S, N, N)],
              'grams': [(S, N, N), (S, C), (S, QN, QN), (S, QN, QN), (Q, S, N, QN), (Q, Q, S, N, N), (S, 4, ncf, 4 * QN + 4),
                        (S, 4, nvs, 2 * N + 4 * nvs)]}
    return {k: tuple(torch.randn(*s, generator=g, dtype=torch.float64) for s in v) for k, v in shapes.items()}


def test_dump_keeps_the_rows_of_one_seeded_sample_of_subdomains(tmp_path, monkeypatch):
    S, Q, N = 48, 2, 6
    buf = _fake_buffers(S, Q, N, ncf=4, nvs=5)
    total = sum(v.numel() * 8 for k in ('sys', 'grams') for v in buf[k])
    monkeypatch.setattr(bench, 'DUMP_BYTES', total // 3)
    info = bench.dump_outputs(str(tmp_path / 'a'), buf, S)
    assert info['of'] == S and 0 < info['subdomains'] < S // 3 + 1 and info['bytes'] <= total // 3
    again = bench.dump_outputs(str(tmp_path / 'b'), buf, S)
    assert again['subdomains'] == info['subdomains']
    names = bench.DUMP_NAMES['sys'] + bench.DUMP_NAMES[8]
    assert sorted(os.listdir(str(tmp_path / 'a'))) == sorted(n + '.npy' for n in names)
    # every array cut along its own subdomain axis at the same subdomains
    full = dict(zip(names, buf['sys'] + buf['grams']))
    gid = {name: torch.zeros_like(v) for name, v in full.items()}
    for name, v in gid.items():
        ax = bench.DUMP_S_AXIS.get(name, 0)
        v.copy_(torch.arange(S, dtype=torch.float64).reshape([-1 if d == ax else 1 for d in range(v.dim())]).expand_as(v))
    ids = bench.dump_outputs(str(tmp_path / 'ids'), {'sys': tuple(gid[n] for n in bench.DUMP_NAMES['sys']),
                                                     'grams': tuple(gid[n] for n in bench.DUMP_NAMES[8])}, S)
    rows = None
    for name in names:
        a = np.load(str(tmp_path / 'a' / (name + '.npy')))
        assert a.dtype == np.float64
        assert np.array_equal(a, np.load(str(tmp_path / 'b' / (name + '.npy'))))
        ax = bench.DUMP_S_AXIS.get(name, 0)
        got = np.unique(np.load(str(tmp_path / 'ids' / (name + '.npy'))).swapaxes(0, ax).reshape(ids['subdomains'], -1), axis=1)
        assert got.shape[1] == 1
        rows = got[:, 0] if rows is None else rows
        assert np.array_equal(got[:, 0], rows) and np.all(np.diff(rows) > 0)
        assert np.array_equal(a, full[name].numpy().take(rows.astype(np.int64), axis=ax))


@pytest.mark.gpu
def test_bench_dumps_what_the_timed_pass_computed(tmp_path):
    """The arrays bench.py writes are the outputs of the pass on its seeded inputs: the same pass, run here, gives them."""
    dump = str(tmp_path / 'dump')
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--config', 'cfg2',
           '--no-cpu-baseline', '--no-online', '--dump-outputs', dump]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out['steps'] == 2 and out['ms_per_step'] > 0
    info = out['dumped_outputs']
    files = sorted(os.listdir(dump))
    assert files == sorted(n + '.npy' for n in info['arrays'])
    assert sum(os.path.getsize(os.path.join(dump, f)) for f in files) <= 64 * 10 ** 6

    from pylrbms_amd import multiscale_problem
    from pylrbms_amd.engine import Engine
    cfg = bench.CONFIGS['cfg2']
    p = multiscale_problem.init_grid_and_problem({'num_subdomains': cfg['num_subdomains'],
                                                  'coarse_per_subdomain': cfg['coarse_per_subdomain']})
    lam = p['lambda']
    theta_bar = np.array([c.evaluate(p['mu_bar']) for c in lam['coefficients']])
    eng = Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar)
    eng.assemble()
    V = eng.ctx.zeros(eng.S_ext, p['grid'].template.n, cfg['N'])
    V[:eng.S] = eng.ctx.from_numpy(bench.make_bases_host(eng.local, p['grid'].template.n, cfg['N']))
    buf = eng.project_and_estimate(V, eng.alloc_reduce_buffers(cfg['N']))
    torch.cuda.synchronize()
    assert info['subdomains'] == info['of'] == eng.S                  # config 2 fits whole
    for name, v in zip(info['arrays'], buf['sys'] + buf['grams']):
        want, got = v.cpu().numpy(), np.load(os.path.join(dump, name + '.npy'))
        assert got.dtype == np.float64 and got.shape == want.shape, name
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), name
