"""Sharded views (S_ext > S) of the 3D / P2 path on the GPU against the CPU oracle on the GLOBAL mesh, per split axis
(the contract of include/lrbms3d_hip.h: neighbours through ``nbr [S][7]`` into the S_ext ordering, ``lam``, ``Cf``,
``phys`` of halo subdomains, and of a halo slab of ``V`` only the cube layer next to the shared side).

Every rank of every tiling of tests/sharded3d_ref.py:CASES is emulated in this process, one ``Engine3D`` after the other (released
before the next); ``V`` is the view ``fill_view`` builds from the production exchange plan, NaN in every halo row the exchange does
not move.  Nothing here starts a process or touches ``torch.distributed``.

The module-scoped fixture ``run`` does the device work of one (case, world) once and keeps plain numbers per rank; the tests assert
on them, each printing its figures first.

Tolerances (none of them fitted to the outcome): 1e-11 relative in the max norm for every assembled and projected array and for
``fom_apply`` -- ``TOL`` and ``rel`` of tests/test_parity3d_gpu.py --, 1e-10 for the estimator terms (the same file), 1e-12 between
the two forms of the batched estimate (test_batched_estimate_matches_single_estimates there) and between a restricted and a whole
pass at the automatic K-split, bit for bit at a forced one.  ``rel`` is taken over the local part of an array,
for ``A_cpl`` also per side and for ``B_sys`` per slot, so that a halo side is not hidden under the maximum of the others."""
import functools

import numpy as np
import pytest

import common3d as c3
import sharded3d_ref as sr

pytestmark = pytest.mark.gpu

TOL = 1e-11
TOL_ETA = 1e-10
TOL_FORMS = 1e-12
ASSEMBLED = ('A_diag', 'A_cpl', 'b', 'f2', 'ceps', 'bdiv', 'ebar', 'Aaa', 'Aab', 'Bbb', 'P_diag', 'Cf')
NMU = (3, 9)                                                  # the batched estimate works in passes of 8: a partial pass; 8 + 1
RESTRICTED = {('z2', 2), ('z4_line', 4), ('cube8', 8), ('cube8', 2)}      # cube8 at 2 ranks: S = 4, rows that must NOT change
# subdomain axis of every output of the pass; what phase 2 writes (include/lrbms3d_hip.h: lrbms3_pass_set_subset)
AXIS = dict(B_sys=1, rhs_red=0, G_nc=0, G_bb=0, G_rdd=0, G_ab=1, G_aa=2, r_fd=0, Rb=0, Yb=0, Dp=0, Xab=1, As=0, Cn=0)
SIDE_ARRAYS = ('Rb', 'As', 'B_cpl_lo', 'B_cpl_hi')
NAN = float('nan')


def worse(a, b):
    """max that keeps a NaN (the builtin drops it)."""
    if a != a or b != b:
        return NAN
    return max(a, b)


@functools.lru_cache(maxsize=None)
def global_case(name):
    """Problem, oracle, global bases and the oracle's reduced model of a case; the inputs and references of the online checks."""
    p = sr.problem_of(name)
    d = c3.oracle_of(p)
    N = p['N']
    Vg = c3.make_bases3d(d.S, d.n, N, seed=3)
    rd = c3.reduce_with_oracle(p, d, Vg)
    rng = np.random.default_rng(5)
    u = rng.standard_normal((d.S, N))
    ref = dict(u=u, eta=np.stack(rd.local_terms([u[ii] for ii in range(d.S)], p['mu'])), batch={})
    for nmu in NMU:
        mus = rng.uniform(0.1, 1.3, size=nmu)
        U = rng.standard_normal((d.S, N, nmu))
        eta = np.stack([np.stack(rd.local_terms([U[ii, :, m] for ii in range(d.S)], mus[m])) for m in range(nmu)], axis=2)
        ref['batch'][nmu] = dict(thetas=np.stack([c3.theta_of(p, mu) for mu in mus]), U=U, eta=eta)        # eta [3, S, nmu]
    x = rng.standard_normal((d.S, d.n, 3))
    ref['x'], ref['Ax'] = x, (d.system_matrix(p['mu']) @ x.reshape(d.ndof, 3)).reshape(d.S, d.n, 3)
    return p, d, Vg, rd, ref


def make_engine(p, grid):
    from pylrbms_amd.engine3d import Engine3D
    return Engine3D(grid, p['lambdas'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar=c3.theta_of(p, p['mu_bar'])).assemble()


def release(eng):
    import torch
    torch.cuda.synchronize()
    eng.ctx.close()


def fresh(eng, N):
    out, work = eng.alloc_outputs(N), eng.alloc_work(N)
    for x in list(out.values()) + [work]:
        x.fill_(NAN)
    return out, work


def views(eng, out, work, N):
    """name -> view with the subdomain axis first of everything a pass writes: the outputs (B_sys as its diagonal slot and the two
    groups of coupling slots) and the three parts of the work buffer."""
    S, t, Q = eng.S, eng.t, eng.Q
    v = {k: out[k].movedim(AXIS[k], 0) for k in out if k != 'B_sys'}
    B = out['B_sys'].movedim(1, 0)
    v['B_diag'], v['B_cpl_lo'], v['B_cpl_hi'] = B[:, :, 3], B[:, :, 0:3], B[:, :, 4:7]
    n0, n1, n2 = S * t.n_rt * Q * N, S * t.n_nodes * N, S * t.nbd * N
    assert work.numel() == n0 + n1 + n2
    v['Rs'], v['Avg'], v['Zb'] = work[:n0].view(S, -1), work[n0:n0 + n1].view(S, -1), work[n0 + n1:].view(S, -1)
    return v


# ------------------------------------------------------------------------------------------------------------ measurements
def measure_assembled(eng, view):
    from pylrbms_amd.grid3d import SIDE_TO_SLOT
    got = {k: eng.ops[k].cpu().numpy().reshape(view['ops'][k].shape) for k in ASSEMBLED}
    rels = {k: c3.rel(got[k], view['ops'][k]) for k in ASSEMBLED}
    per_side = [c3.rel(got['A_cpl'][:, :, a], view['ops']['A_cpl'][:, :, a]) for a in range(6)]
    # a coupling side towards a halo subdomain carries blocks (a vanishing reference would make its rel an exact-zero check)
    halo_sides_nonzero = all(float(np.abs(view['ops']['A_cpl'][:, i, a]).max()) > 0.0
                             for i in range(eng.S) for a in range(6) if eng.nbr[i, SIDE_TO_SLOT[a]] >= eng.S)
    return dict(rels=rels, A_cpl_side=per_side, halo_sides_nonzero=halo_sides_nonzero)


def dense_rels(eng, out, view, Q, N):
    from pylrbms_amd.engine3d import expand_factored
    got = {k: v.cpu().numpy() for k, v in expand_factored(eng, out, Q, N).items()}
    worst, slot = {}, [0.0] * 7
    for i, ref in enumerate(view['dense']):
        pairs = [(k, got[k][i], ref[k]) for k in ('G_nc', 'G_bb', 'G_rdd', 'r_fd')]
        pairs += [('G_ab', got['G_ab'][:, i], ref['G_ab']), ('G_aa', got['G_aa'][:, :, i], ref['G_aa']),
                  ('B_sys', got['B_sys'][:, i], ref['B_sys']), ('rhs_red', got['rhs_red'][i], view['rhs'][i])]
        for k, a, b in pairs:
            worst[k] = worse(worst.get(k, 0.0), c3.rel(a, b))
        for s in range(7):
            slot[s] = worse(slot[s], c3.rel(got['B_sys'][:, i, s], ref['B_sys'][:, s]))
    return worst, slot


def measure_pass(eng, Vd, view, Q, N):
    """The whole pass and the two phases on the NaN-poisoned view into NaN-filled buffers, at K-split 0, 1 and 2.  Returns the
    figures per K-split and the outputs of the automatic one."""
    import torch
    res, keep = {}, None
    try:
        for ks in (0, 1, 2):
            eng.ctx.set_option('ksplit', ks)
            out, work = fresh(eng, N)
            eng.project_and_estimate(Vd, out, work)
            o2, w2 = fresh(eng, N)
            eng.ctx.project_estimate(Q, Vd, eng.ops, w2, o2, phase=1)
            eng.ctx.project_estimate(Q, Vd, eng.ops, w2, o2, phase=2)
            torch.cuda.synchronize()
            worst, slot = dense_rels(eng, out, view, Q, N)
            res[ks] = dict(not_finite=[k for k, v in out.items() if not bool(torch.isfinite(v).all())],
                           phased_differs=[k for k in out if not torch.equal(out[k], o2[k])] + ([] if torch.equal(work, w2) else ['work']),
                           worst=worst, slot=slot)
            if ks == 0:
                keep = out
    finally:
        eng.ctx.set_option('ksplit', 0)
    return res, keep


def measure_estimates(eng, out, p, d, ref):
    ctx, loc, ext = eng.ctx, list(eng.local), list(eng.ext)
    th = c3.theta_of(p, p['mu'])
    eta = eng.reduced_estimate(th, ctx.from_numpy(ref['u'][ext]), out).cpu().numpy()
    res = dict(single=[c3.rel(eta[k], ref['eta'][k][loc]) for k in range(3)], batch={})
    for nmu, b in ref['batch'].items():
        U = ctx.from_numpy(b['U'][ext])
        got = {}
        try:
            for form in (0, 1):
                ctx.set_option('estimate_valu', form)
                got[form] = ctx.reduced_estimate_batch(d.Q, b['thetas'], U, out, eng.ops, eng.hdiam).cpu().numpy()      # [3, S, nmu]
        finally:
            ctx.set_option('estimate_valu', 0)
        want = b['eta'][:, loc]
        cols = {form: max((c3.rel(got[form][k, :, m], want[k, :, m]) for k in range(3) for m in range(nmu)), key=_nan_first)
                for form in (0, 1)}
        res['batch'][nmu] = dict(mfma=cols[0], valu=cols[1],
                                 forms=max((c3.rel(got[0][k, :, m], got[1][k, :, m]) for k in range(3) for m in range(nmu)), key=_nan_first))
    return res


def _nan_first(x):
    return float('inf') if x != x else x


def measure_fom_apply(eng, plan, plans, p, d, ref):
    x = eng.ctx.from_numpy(sr.fill_view(plan, plans, ref['x'], 3))           # halo slabs: the exchanged layer, NaN elsewhere
    y = eng.ctx.fom_apply(d.Q, c3.theta_of(p, p['mu']), eng.ops['A_diag'], eng.ops['A_cpl'], x).cpu().numpy()
    return c3.rel(y, ref['Ax'][list(eng.local)])


def changed_basis(Vg, ids):
    V2 = Vg.copy()
    rng = np.random.default_rng(23)
    for g in ids:
        V2[g, :, -1] = rng.standard_normal(Vg.shape[1])
    return V2


def measure_restricted(eng, plan, plans, Vg, N):
    """Whole pass on the view of ``Vg``; the basis of some subdomains replaced in ``Vg``, the view rebuilt, and the restricted pass on
    their S_ext indices into the same buffers -- against a whole pass on the new view into fresh buffers.  Variants: the first local
    subdomain together with the last halo subdomain, and every halo subdomain alone."""
    import torch
    from pylrbms_amd.grid3d import side_targets
    S, ctx = eng.S, eng.ctx
    V_old = ctx.from_numpy(sr.fill_view(plan, plans, Vg, N))
    variants = [('local+halo', [0, eng.S_ext - 1])] + [('halo {}'.format(h), [h]) for h in range(S, eng.S_ext)]
    res = []
    try:
        for ks in (0, 1, 2):
            ctx.set_option('ksplit', ks)
            for label, subset in variants:
                V_new = ctx.from_numpy(sr.fill_view(plan, plans, changed_basis(Vg, [eng.ext[i] for i in subset]), N))
                out, work = fresh(eng, N)
                eng.project_and_estimate(V_old, out, work)
                mine = views(eng, out, work, N)
                before = {k: x.clone() for k, x in mine.items()}
                eng.project_and_estimate(V_new, out, work, subset=subset)
                ref_out, ref_work = fresh(eng, N)
                eng.project_and_estimate(V_new, ref_out, ref_work)
                torch.cuda.synchronize()
                ref = views(eng, ref_out, ref_work, N)
                own, side = [i for i in subset if i < S], side_targets(eng.nbr, subset)
                moved = {k: not torch.equal(before[k][side], ref[k][side]) for k in SIDE_ARRAYS}      # the new basis matters
                rec = dict(ks=ks, label=label, own=own, side=side, rows_changed=[], differs=[], worst=0.0, worst_at=None,
                           side_moved=moved['Rb'] and moved['As'] and (moved['B_cpl_lo'] or moved['B_cpl_hi']))
                for k, x in mine.items():
                    rows = side if k in SIDE_ARRAYS else own
                    keep = torch.ones(S, dtype=torch.bool, device=x.device)
                    if rows:
                        keep[torch.as_tensor(rows, device=x.device)] = False
                    if not torch.equal(x[keep], before[k][keep]):
                        rec['rows_changed'].append(k)
                    if not torch.equal(x, ref[k]):
                        rec['differs'].append(k)
                        scale = float(ref[k].abs().max())
                        err = float((x - ref[k]).abs().max()) / max(scale, 1e-300)
                        if rec['worst'] == rec['worst'] and (err != err or err > rec['worst']):      # a NaN stays
                            rec['worst'], rec['worst_at'] = err, k
                res.append(rec)
    finally:
        ctx.set_option('ksplit', 0)
    return res


@pytest.fixture(scope='module', params=sr.RUNS, ids=['{}-w{}'.format(*nw) for nw in sr.RUNS])
def run(request):
    import torch
    from pylrbms_amd.grid3d import tile_grid3d
    name, world = request.param
    case = sr.CASES[name]
    tiling = tile_grid3d(world, list(case['P']))
    p, d, Vg, rd, ref = global_case(name)
    grids, plans = sr.rank_grids(case['domain'], case['P'], case['kc'], world, case['kappa'])
    Q, N = d.Q, p['N']
    ranks = []
    for r in range(world):
        eng = make_engine(p, grids[r])
        try:
            view = sr.oracle_view(p, d, rd, eng)
            rec = dict(rank=r, S=eng.S, S_ext=eng.S_ext, local=list(eng.local), halo=list(eng.halo))
            rec['assembled'] = measure_assembled(eng, view)
            Vd = eng.ctx.from_numpy(sr.fill_view(plans[r], plans, Vg, N))
            rec['V_has_nan'] = bool(torch.isnan(Vd).any())
            rec['pass'], out = measure_pass(eng, Vd, view, Q, N)
            rec['estimate'] = measure_estimates(eng, out, p, d, ref)
            rec['fom_apply'] = measure_fom_apply(eng, plans[r], plans, p, d, ref)
            if (name, world) in RESTRICTED:
                rec['restricted'] = measure_restricted(eng, plans[r], plans, Vg, N)
            ranks.append(rec)
        finally:
            release(eng)                                    # one context at a time
            del eng
    return dict(name=name, world=world, tiling=tiling, want_tiling=case['worlds'][world], Q=Q, N=N, ranks=ranks)


# ------------------------------------------------------------------------------------------------------------------- tests
def tag(run, rec):
    return '{} world {} rank {} (S {} S_ext {})'.format(run['name'], run['world'], rec['rank'], rec['S'], rec['S_ext'])


def test_every_rank_is_a_view_with_halo(run):
    assert run['tiling'] == run['want_tiling']
    assert len(run['ranks']) == run['world']
    for rec in run['ranks']:
        assert rec['S_ext'] > rec['S'] >= 1, tag(run, rec)
    if run['name'] == 'cube8' and run['world'] == 8:
        assert all((rec['S'], rec['S_ext']) == (1, 4) for rec in run['ranks'])
    if run['name'] == 'z4_line':
        assert [(rec['S'], rec['S_ext']) for rec in run['ranks']] == [(1, 2), (1, 3), (1, 3), (1, 2)]
    if run['name'] != 'x2_thin':
        assert any(rec['V_has_nan'] for rec in run['ranks'])       # rows the exchange does not move: poisoned


def test_assembled_operators_of_the_view_match_the_oracle(run):
    for rec in run['ranks']:
        a = rec['assembled']
        print(tag(run, rec), 'assembled worst', max(a['rels'].values(), key=_nan_first), 'A_cpl per side', a['A_cpl_side'])
    bad = []
    for rec in run['ranks']:
        a = rec['assembled']
        assert a['halo_sides_nonzero'], tag(run, rec)
        bad += [(tag(run, rec), k, v) for k, v in a['rels'].items() if not v < TOL]
        bad += [(tag(run, rec), 'A_cpl side {}'.format(s), v) for s, v in enumerate(a['A_cpl_side']) if not v < TOL]
    assert bad == []


def test_pass_on_the_poisoned_view_matches_the_oracle_at_every_ksplit(run):
    for rec in run['ranks']:
        for ks, m in rec['pass'].items():
            print(tag(run, rec), 'ksplit', ks, 'pass worst', max(m['worst'].values(), key=_nan_first), 'B_sys per slot', m['slot'])
    bad = []                                                  # every miss of every rank in one report
    for rec in run['ranks']:
        for ks, m in rec['pass'].items():
            if m['not_finite']:
                bad.append((tag(run, rec), ks, 'not finite', m['not_finite']))
            bad += [(tag(run, rec), ks, k, v) for k, v in m['worst'].items() if not v < TOL]
            bad += [(tag(run, rec), ks, 'B_sys slot {}'.format(s), v) for s, v in enumerate(m['slot']) if not v < TOL]
    assert bad == []


def test_phase_1_then_2_is_the_whole_pass_bit_for_bit(run):
    for rec in run['ranks']:
        for ks, m in rec['pass'].items():
            assert m['phased_differs'] == [], (tag(run, rec), ks)


def test_single_estimate_of_the_view_matches_the_oracle(run):
    for rec in run['ranks']:
        print(tag(run, rec), 'estimate nc / r / df', rec['estimate']['single'])
    for rec in run['ranks']:
        assert all(v < TOL_ETA for v in rec['estimate']['single']), (tag(run, rec), rec['estimate']['single'])


def test_batched_estimate_of_the_view_matches_the_oracle_in_both_forms(run):
    for rec in run['ranks']:
        print(tag(run, rec), 'batched estimate', rec['estimate']['batch'])
    for rec in run['ranks']:
        for nmu, b in rec['estimate']['batch'].items():
            assert b['mfma'] < TOL_ETA and b['valu'] < TOL_ETA and b['forms'] < TOL_FORMS, (tag(run, rec), nmu, b)


def test_full_order_apply_of_the_view_is_the_global_operator(run):
    for rec in run['ranks']:
        print(tag(run, rec), 'fom_apply', rec['fom_apply'])
    for rec in run['ranks']:
        assert rec['fom_apply'] < TOL, (tag(run, rec), rec['fom_apply'])


def test_restricted_pass_with_a_changed_halo_slab(run):
    """A changed halo slab re-projects the side arrays of its local neighbours and nothing else; together with a changed local
    subdomain: the whole pass on the new view -- bit for bit at K-split 1 and 2, to 1e-12 max|array| at the automatic one."""
    if (run['name'], run['world']) not in RESTRICTED:
        return
    for rec in run['ranks']:
        for m in rec['restricted']:
            if m['ks'] == 0:
                print(tag(run, rec), m['label'], 'restricted vs whole at ksplit 0: worst', m['worst'], m['worst_at'])
    for rec in run['ranks']:
        assert len(rec['restricted']) == 3 * (1 + rec['S_ext'] - rec['S'])
        for m in rec['restricted']:
            where = (tag(run, rec), m['ks'], m['label'])
            assert len(m['side']) >= 1 and m['side_moved'], where                  # the change reaches a local subdomain
            if m['label'] != 'local+halo':
                assert m['own'] == [], where                                       # halo alone: no own array is written at all
            assert m['rows_changed'] == [], where
            if m['ks'] == 0:
                assert m['worst'] <= 1e-12, (where, m['worst'], m['worst_at'])
            else:
                assert m['differs'] == [], where


def test_exports_that_need_all_subdomains_refuse_a_view(monkeypatch):
    """LRBMS_E_INVALID with "needs all subdomains on this rank", no output written, and the context goes on: the next pass gives
    the bits of the one before.  On both ranks of z2."""
    import torch
    from pylrbms_amd._native import NativeError
    p, d, Vg, rd, ref = global_case('z2')
    case = sr.CASES['z2']
    grids, plans = sr.rank_grids(case['domain'], case['P'], case['kc'], 2, case['kappa'])
    Q, N = d.Q, p['N']
    SENTINEL = -7.25
    for r in range(2):
        eng = make_engine(p, grids[r])
        try:
            ctx, ops, S, t = eng.ctx, eng.ops, eng.S, eng.t
            assert eng.S_ext > S
            Vd = ctx.from_numpy(sr.fill_view(plans[r], plans, Vg, N))
            out, work = fresh(eng, N)
            eng.project_and_estimate(Vd, out, work)
            th = c3.theta_of(p, p['mu'])
            thetas = np.stack([th, 0.5 * th])
            b_K, bdiv_K = ops['b'][None].contiguous(), ops['bdiv'][None].contiguous()
            D_corr = torch.zeros_like(ops['A_cpl'])
            Y = ctx.from_numpy(np.ones((S, t.n, 2)))
            calls = {
                'reduced_solve': lambda: eng.reduced_solve(th, out),
                'reduced_solve_batch': lambda: ctx.reduced_solve_batch(Q, thetas, out['B_sys'], out['rhs_red']),
                'reduced_precond_build': lambda: ctx.reduced_precond_build(Q, th, out['B_sys']),
                'fom_solve': lambda: ctx.fom_solve(Q, th, ops['A_diag'], ops['A_cpl'], ops['b']),
                'project_mass': lambda: ctx.project_mass(Vd),
                'mass_inverse_norm2': lambda: ctx.mass_inverse_norm2(Y),
                'project_sources': lambda: ctx.project_sources(Q, b_K, bdiv_K, Vd, work),
                'local_correction_solve': lambda: ctx.local_correction_solve(Q, th, [0], ops['A_diag'], ops['A_cpl'], D_corr, ops['b']),
            }
            made = []
            plain_empty = ctx.empty

            def marked_empty(*shape):
                x = plain_empty(*shape)
                x.fill_(SENTINEL)
                made.append(x)
                return x
            for name, call in calls.items():
                del made[:]
                monkeypatch.setattr(ctx, 'empty', marked_empty)
                with pytest.raises(NativeError, match=r'\(-1\): {}: needs all subdomains on this rank'.format(name)):
                    call()
                monkeypatch.setattr(ctx, 'empty', plain_empty)
                torch.cuda.synchronize()
                assert len(made) >= 1, name                                  # the wrapper allocated the output it would have returned
                assert all(bool((x == SENTINEL).all()) for x in made), name
                o2, w2 = fresh(eng, N)
                eng.project_and_estimate(Vd, o2, w2)
                torch.cuda.synchronize()
                assert torch.equal(w2, work) and all(torch.equal(o2[k], out[k]) for k in out), name
        finally:
            release(eng)
            del eng
