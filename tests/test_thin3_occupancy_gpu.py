"""The merged thin side kernel k_thin3 (csrc/fused.hip) after the register diet of ``thin_ncf_body`` -- runs on the MI355X box
(`-m gpu`).

The diet moved loads and stores of the F_nc body (the M_ab rows and the neighbour's vertex averages are copied behind the first
barrier, the touch tables are requested together, the rows of a batch are addressed by 32-bit lane offsets, the first batch stands
outside its loop) without touching an expression or a summation order.  On 3 x 3 subdomains (one interior subdomain with four
neighbours, edges and corners for the sides without neighbour, both side orientations), Q = 2, over

    k_c = 4, N = 40   config 3's per-subdomain shape: NTX = 3, 16-byte items, one batch
    k_c = 4, N = 39   odd N: 8-byte items, five per batch
    k_c = 4, N = 20   NTX = 2
    k_c = 2, N = 34   fewer touching elements than threads in a batch

each with the Oswald vertex patch off and on:

- F_nc, F_side, r_fd and the off-diagonal blocks of B_sys of the factored pass against the oracle (1e-11, the tolerance
  tests/test_dispatch_parity_gpu.py applies to these arrays; the factors through the blocks they stand for).  With the vertex patch
  F_nc carries the diagonal subdomains and has no dense block form: it is checked through the local nonconformity terms of a
  reduced model against the oracle's reductor with ``oswald_patch='vertex'`` (1e-10, as tests/test_parity_gpu.py does);
- the same bits in all twelve outputs with the side tables kept and rebuilt (LRBMS_OPT_SIDE_TABLES 1 / 0), and from the merged
  launch and the separate k_thin_ncf / k_thin_rt / k_coupling launches (LRBMS_OPT_THIN_MERGE 1 / 0), whole pass and by phases;
- a subset pass over the interior subdomain's neighbourhood: its rows are the whole pass's bits, every other row stays as it was."""
import numpy as np
import pytest

from common import (compact_blocks, energy_orthonormalize, expand_cols, expand_square, make_bases, oracle_from_problem, rel_err,
                    slots_of, theta_bar_of, theta_of)

pytestmark = pytest.mark.gpu

TOL = 1e-11            # tests/test_dispatch_parity_gpu.py: every array against the oracle
ETA_TOL = 1e-10        # ... and the estimates of a reduced model (tests/test_parity_gpu.py: the vertex patch against the oracle)
SHAPE, Q = (3, 3), 2
CASES = [(4, 40), (4, 39), (4, 20), (2, 34)]
PARAMS = [(kc, N, patch) for patch in (False, True) for kc, N in CASES]
IDS = ['kc{}-N{}-{}'.format(kc, N, 'patch' if patch else 'head') for kc, N, patch in PARAMS]
NEIGHBOURHOOD = [1, 3, 4, 5, 7]      # the interior subdomain of the 3 x 3 grid and its four neighbours

_SETUPS, _REDUCED = {}, {}


def _setup(kc, patch):
    """(problem, engine, oracle) of a template and a patch setting: built once, shared by every test that needs them."""
    if (kc, patch) not in _SETUPS:
        from pylrbms_amd import multiscale_problem
        from pylrbms_amd.engine import Engine
        p = multiscale_problem.init_grid_and_problem({'num_subdomains': list(SHAPE), 'coarse_per_subdomain': kc})
        lam = p['lambda']
        eng = Engine(p['grid'], lam['functions'], p['kappa'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar_of(p),
                     conventions={'oswald_vertex_patch': True} if patch else None).assemble()
        d = oracle_from_problem(p, oswald_patch='vertex') if patch else oracle_from_problem(p)
        assert eng.S == 9 and eng.Q == Q and d.Q == Q
        _SETUPS[kc, patch] = (p, eng, d)
    return _SETUPS[kc, patch]


def _reduced(kc, N, patch):
    """(bases on the host, on the device, the oracle's reduced data): computed once per case and left unchanged."""
    if (kc, N, patch) not in _REDUCED:
        from oracle.lrbms import OracleReductor
        p, eng, d = _setup(kc, patch)
        V = energy_orthonormalize(make_bases(d.S, d.n, N, seed=5 + N), d)
        rd = OracleReductor(d, [V[ii] for ii in range(d.S)]).reduce()
        _REDUCED[kc, N, patch] = (V, eng.ctx.from_numpy(V), rd)
    return _REDUCED[kc, N, patch]


def _host(x):
    return x.detach().cpu().numpy()


@pytest.mark.parametrize('kc, N, patch', PARAMS, ids=IDS)
def test_factored_outputs_of_the_thin_kernels_match_the_oracle(kc, N, patch):
    from pylrbms_amd.engine import expand_factored_grams
    p, eng, d = _setup(kc, patch)
    grid = p['grid']
    V, Vd, rd = _reduced(kc, N, patch)
    assert eng.ctx.fused_supported(Q, N, factored=True)
    S, QN, nvs = eng.S, Q * N, eng.ctx.nvs
    eng.ctx.kernel_timing(True)
    try:
        buf = eng.project_and_estimate(Vd, eng.alloc_reduce_buffers(N), fused=True)
        ran = {k for k, _ in eng.ctx.kernel_timing_read()}
    finally:
        eng.ctx.kernel_timing(False)
    assert 'k_thin3' in ran, sorted(ran)
    grams = buf['grams']
    assert len(grams) == 8 and grams[7].shape == (S, 4, nvs, (3 if patch else 2) * N + 4 * nvs)
    # the dense blocks the factors stand for (F_nc without the diagonal subdomains' column block; its G_nc is used for HEAD only)
    dense = expand_factored_grams(tuple(grams[:7]) + (grams[7][..., :2 * N + 4 * nvs].contiguous(),))
    G_nc, r_fd, G_rdd, G_bb = [_host(x) for x in dense[:4]]
    B_sys = _host(buf['sys'][0])
    errs = {'B_sys_offdiag': 0.0, 'r_fd': 0.0, 'F_side:G_rdd': 0.0, 'F_side:G_bb': 0.0}
    sys_scale = max(np.abs(rd.op[ii][ii][q]).max() for ii in range(S) for q in range(Q))
    for ii in range(S):
        for q in range(Q):
            for k, jj in enumerate(slots_of(grid, ii)):
                if k == 2:
                    continue
                ref = rd.op[ii][jj][q] if jj >= 0 else np.zeros((N, N))
                errs['B_sys_offdiag'] = max(errs['B_sys_offdiag'], float(np.abs(B_sys[q, ii, k] - ref).max() / sys_scale))
        errs['r_fd'] = max(errs['r_fd'], rel_err(r_fd[ii], expand_cols(rd.r_fd[ii], grid, ii, QN)))
        for name, got, ref in (('F_side:G_rdd', G_rdd[ii], rd.r_dd[ii]), ('F_side:G_bb', G_bb[ii], rd.df_bb[ii])):
            blocks, _ = compact_blocks(expand_square(ref, grid, ii, None, QN), QN)
            errs[name] = max(errs[name], rel_err(got, blocks))
        if not patch:
            errs['F_nc:G_nc'] = max(errs.get('F_nc:G_nc', 0.0), rel_err(G_nc[ii], expand_square(rd.nc[ii], grid, ii, None, N)))
    print('thin kernels vs oracle, k_c {} N {} patch {}: {}'.format(kc, N, patch, errs))
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad
    # F_nc as the estimate kernels read it: the local nonconformity terms of a reduced model (with the patch the only form the
    # diagonal subdomains' block has)
    rng = np.random.default_rng(3)
    mus = [0.15, 1.0]
    U = rng.standard_normal((S, N, len(mus)))
    thetas = np.stack([theta_of(p, mu) for mu in mus])
    eta_b = _host(eng.ctx.reduced_estimate_batch(thetas, eng.ctx.from_numpy(U), grams, eng.f2, eng.ceps, eng.hdiam))
    for m, mu in enumerate(mus):
        um = np.ascontiguousarray(U[:, :, m])
        eta_s = _host(eng.reduced_estimate(thetas[m], eng.ctx.from_numpy(um), grams))
        _, (nc, r, df), _ = rd.estimate([um[ii] for ii in range(S)], mu, decompose=True)
        for row, want in enumerate((nc, r, df)):
            scale = max(np.abs(want).max(), 1e-300)
            e_s, e_b = np.abs(eta_s[row] - want).max() / scale, np.abs(eta_b[row, :, m] - want).max() / scale
            print('  estimate row {} mu {}: single {:.2e} batched {:.2e}'.format(row, mu, e_s, e_b))
            assert e_s < ETA_TOL and e_b < ETA_TOL, (m, row, e_s, e_b)


def _outputs(buf):
    return list(buf['sys']) + list(buf['grams'])


def _run(eng, V, buf, phases=(0,)):
    """The pass into NaN-filled outputs and work; -> (clones of the twelve outputs, timing names of the kernels that ran)."""
    for x in _outputs(buf) + [buf['work']]:
        x.fill_(float('nan'))
    args = (V, eng.F, eng.A_diag, eng.A_cpl, eng.P_diag, eng.b, eng.ebar, eng.caa, eng.Aab, eng.Bbb, buf['work'], buf['sys'],
            buf['grams'])
    eng.ctx.kernel_timing(True)
    try:
        for ph in phases:
            eng.ctx.project_estimate_fused(*args, phase=ph)
        ran = {k for k, _ in eng.ctx.kernel_timing_read()}
    finally:
        eng.ctx.kernel_timing(False)
    return [x.clone() for x in _outputs(buf)], ran


def _assert_equal(got, want, tag):
    import torch
    assert len(got) == len(want) == 12
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(b).all()), (tag, i)
        assert torch.equal(a, b), '{}: output {} differs (max |diff| {})'.format(
            tag, i, float((a - b).abs().nan_to_num(float('inf')).max()))


SEPARATE = {'k_thin_ncf', 'k_thin_rt', 'k_coupling'}


@pytest.mark.parametrize('kc, N, patch', PARAMS, ids=IDS)
def test_launch_forms_give_the_same_bits_and_a_subset_pass_leaves_the_rest(kc, N, patch):
    import torch
    _, eng, _ = _setup(kc, patch)
    _, Vd, _ = _reduced(kc, N, patch)
    buf = eng.alloc_reduce_buffers(N, factored=True)
    opts = {'side_tables': 1, 'thin_merge': 1, 'streams': -1}
    try:
        _run(eng, Vd, buf)
        want, ran = _run(eng, Vd, buf)                      # merged launch, tables kept, forked (9 subdomains)
        assert 'k_thin3' in ran and 'k_side_tables' not in ran and not (SEPARATE & ran), sorted(ran)
        eng.ctx.set_option('side_tables', 0)
        got, ran = _run(eng, Vd, buf)
        assert 'k_side_tables' in ran and 'k_thin3' in ran, sorted(ran)
        _assert_equal(got, want, 'side tables rebuilt')
        eng.ctx.set_option('side_tables', 1)
        eng.ctx.set_option('streams', 0)
        got, ran = _run(eng, Vd, buf)
        assert 'k_thin3' in ran and not (SEPARATE & ran), sorted(ran)
        _assert_equal(got, want, 'merged, one stream')
        eng.ctx.set_option('thin_merge', 0)
        for phases in ((0,), (1, 2)):
            got, ran = _run(eng, Vd, buf, phases=phases)
            assert SEPARATE <= ran and 'k_thin3' not in ran, (phases, sorted(ran))
            _assert_equal(got, want, ('separate launches', phases))
        eng.ctx.set_option('side_tables', 0)
        got, ran = _run(eng, Vd, buf)
        assert SEPARATE <= ran and 'k_side_tables' in ran, sorted(ran)
        _assert_equal(got, want, 'separate launches, side tables rebuilt')
    finally:
        for k, v in opts.items():
            eng.ctx.set_option(k, v)
    # a subset pass over the interior subdomain's neighbourhood, into buffers that hold a sentinel
    sub = torch.tensor(NEIGHBOURHOOD, device=Vd.device)
    rest = torch.tensor([i for i in range(eng.S) if i not in NEIGHBOURHOOD], device=Vd.device)
    for x in _outputs(buf):
        x.fill_(7.0)
    buf['work'].fill_(float('nan'))
    eng.ctx.kernel_timing(True)
    try:
        eng.project_and_estimate(Vd, buf, subset=NEIGHBOURHOOD)
        ran = {k for k, _ in eng.ctx.kernel_timing_read()}
    finally:
        eng.ctx.kernel_timing(False)
    assert 'k_thin3' in ran, sorted(ran)
    for i, (a, b) in enumerate(zip(want, _outputs(buf))):
        sdim = 1 if (a.dim() >= 2 and a.shape[0] == eng.Q and a.shape[1] == eng.S) else 0
        if a.dim() >= 3 and a.shape[0] == eng.Q and a.shape[1] == eng.Q and a.shape[2] == eng.S:
            sdim = 2
        assert torch.equal(a.index_select(sdim, sub), b.index_select(sdim, sub)), i
        assert bool((b.index_select(sdim, rest) == 7.0).all()), i
