"""Incremental re-projection on the 3D / P2 path on the GPU: the restricted pass (``lrbms3_pass_set_subset``)
against the whole pass -- bit for bit at a forced K-split, to summation-order rounding at the automatic one, rows outside the
lists untouched --, its phases, its error paths, and ``LRBMSReductor3D.reserve`` / ``reduce(touched=)`` up to the
``AdaptiveEnrichment`` loop.  Problems and bases are those of tests/common3d.py; a changed basis has its last column replaced.

Tolerances: 1e-12 max|array| between two passes whose K-splits may differ (the summation-order bound of
tests/test_dispatch_parity3d_gpu.py::test_forced_launch_shapes_match_the_oracle), 1e-11 against the oracle's dense blocks (the parity
tolerance there), 1e-7 against the oracle's ragged reduced model (tests/test_enrichment3d_gpu.py)."""
import functools

import numpy as np
import pytest

import common3d as c3

pytestmark = pytest.mark.gpu

TOL = 1e-11
# subdomain axis of every output of the pass
AXIS = dict(B_sys=1, rhs_red=0, G_nc=0, G_bb=0, G_rdd=0, G_ab=1, G_aa=2, r_fd=0, Rb=0, Yb=0, Dp=0, Xab=1, As=0, Cn=0)
SIDE_ARRAYS = ('Rb', 'As', 'B_cpl_lo', 'B_cpl_hi')          # what phase 2 writes; everything else (work included) is an own array


@functools.lru_cache(maxsize=None)
def engine_case(name):
    """(problem, engine, old basis, new bases per changed set) of a common3d problem, built once per module."""
    from pylrbms_amd.engine3d import Engine3D
    p = c3.make_problem(name)
    eng = Engine3D(p['grid'], p['lambdas'], p['f'], p['lambda_bar'], p['lambda_hat'], theta_bar=c3.theta_of(p, p['mu_bar'])).assemble()
    V = c3.make_bases3d(eng.S, eng.t.n, p['N'], seed=3)
    return p, eng, V


def changed_basis(V, changed):
    V2 = V.copy()
    rng = np.random.default_rng(23)
    for ii in changed:
        V2[ii, :, -1] = rng.standard_normal(V.shape[1])
    return V2


def views(eng, out, work, N):
    """name -> view with the subdomain axis first, of every array a pass writes: the outputs (B_sys split into the diagonal slot
    and the six coupling slots) and the three parts of the work buffer."""
    S, t, Q = eng.S, eng.t, eng.Q
    v = {k: out[k].movedim(AXIS[k], 0) for k in out if k != 'B_sys'}
    B = out['B_sys'].movedim(1, 0)                    # [S, Q, 7, N, N]
    v['B_diag'], v['B_cpl_lo'], v['B_cpl_hi'] = B[:, :, 3], B[:, :, 0:3], B[:, :, 4:7]          # views, not copies
    n0, n1, n2 = S * t.n_rt * Q * N, S * t.n_nodes * N, S * t.nbd * N
    assert work.numel() == n0 + n1 + n2
    v['Rs'], v['Avg'], v['Zb'] = work[:n0].view(S, -1), work[n0:n0 + n1].view(S, -1), work[n0 + n1:].view(S, -1)
    return v


def whole_pass(eng, Vd, fill=float('nan')):
    N = Vd.shape[2]
    out, work = eng.alloc_outputs(N), eng.alloc_work(N)
    for x in list(out.values()) + [work]:
        x.fill_(fill)
    eng.project_and_estimate(Vd, out, work)
    return out, work


def restricted_against_whole(name, changed, ksplit, exact=True, poison=None, phases=False):
    """Whole pass on the old basis, NaN into the rows the restricted pass has to write (``poison``: only these arrays), restricted pass
    on the new basis: every array equals the whole pass on the new basis, rows outside the lists keep their bits.  Returns
    (engine, new basis on the device, the updated outputs)."""
    import torch
    from pylrbms_amd.grid3d import side_targets
    p, eng, V = engine_case(name)
    N = p['N']
    own = [c for c in changed if c < eng.S]
    side = side_targets(eng.nbr, changed)
    Vd_old, Vd_new = eng.ctx.from_numpy(V), eng.ctx.from_numpy(changed_basis(V, changed))
    try:
        eng.ctx.set_option('ksplit', ksplit)
        out, work = whole_pass(eng, Vd_old)
        ref_out, ref_work = whole_pass(eng, Vd_new)
        mine, ref = views(eng, out, work, N), views(eng, ref_out, ref_work, N)
        for k, x in mine.items():
            rows = side if k in SIDE_ARRAYS else own
            if rows and (poison is None or k in poison):
                x[torch.as_tensor(rows, device=x.device)] = float('nan')
        before = {k: x.clone() for k, x in mine.items()}
        if phases:
            eng.ctx.pass_set_subset(changed)
            try:
                eng.ctx.project_estimate(eng.Q, Vd_new, eng.ops, work, out, phase=1)
                eng.ctx.project_estimate(eng.Q, Vd_new, eng.ops, work, out, phase=2)
            finally:
                eng.ctx.pass_set_subset(None)
        else:
            eng.project_and_estimate(Vd_new, out, work, subset=changed)
        torch.cuda.synchronize()
    finally:
        eng.ctx.set_option('ksplit', 0)
    for k, x in mine.items():
        rows = side if k in SIDE_ARRAYS else own
        keep = torch.ones(eng.S, dtype=torch.bool, device=x.device)
        if rows:
            keep[torch.as_tensor(rows, device=x.device)] = False
        assert torch.equal(x[keep], before[k][keep]), (k, 'rows outside the list changed')
        if exact:
            assert torch.equal(x, ref[k]), (k, changed, ksplit)
        else:
            assert torch.equal(x[keep], ref[k][keep]), k
            err, scale = float((x - ref[k]).abs().max()), float(ref[k].abs().max())
            print(name, k, 'max deviation', err, 'scale', scale)
            assert err <= 1e-12 * max(scale, 1e-300), (k, err, scale)
    return eng, Vd_new, out


@pytest.mark.parametrize('ksplit', [1, 2, 8])
@pytest.mark.parametrize('changed', [[0, 13, 26], [13], list(range(27))], ids=['three', 'centre', 'all'])
def test_restricted_pass_is_the_whole_pass_bit_for_bit_and_leaves_other_rows_alone(changed, ksplit):
    """[0, 13, 26]: own list 3, side list 15 (two XCD chunks of positions); partial tiles by position at K-split 2 and 8."""
    from pylrbms_amd.grid3d import side_targets
    _, eng, _ = engine_case('interior_3x3x3')
    assert len(side_targets(eng.nbr, changed)) == {3: 15, 1: 7, 27: 27}[len(changed)]
    restricted_against_whole('interior_3x3x3', changed, ksplit)


@functools.lru_cache(maxsize=None)
def oracle_blocks(name, changed):
    p, eng, V = engine_case(name)
    d = c3.oracle_of(p)
    rd = c3.reduce_with_oracle(p, d, changed_basis(V, changed))
    return d, rd, [c3.oracle_dense_blocks(p, d, rd, ii) for ii in range(d.S)]


def test_automatic_ksplit_follows_the_list_lengths():
    """Option 0: the restricted pass picks its K-split from 3 own / 15 side subdomains, the whole pass from 27 -- summation-order
    rounding apart they agree, and the dense blocks are the oracle's."""
    from pylrbms_amd.engine3d import expand_factored
    changed = (0, 13, 26)
    eng, Vd, out = restricted_against_whole('interior_3x3x3', list(changed), 0, exact=False)
    p = engine_case('interior_3x3x3')[0]
    d, rd, refs = oracle_blocks('interior_3x3x3', changed)
    got = {k: v.cpu().numpy() for k, v in expand_factored(eng, out, d.Q, p['N']).items()}
    worst = {}
    for ii, ref in enumerate(refs):
        for k in ('G_nc', 'G_bb', 'G_rdd', 'r_fd'):
            worst[k] = max(worst.get(k, 0.0), c3.rel(got[k][ii], ref[k]))
        worst['G_ab'] = max(worst.get('G_ab', 0.0), c3.rel(got['G_ab'][:, ii], ref['G_ab']))
        worst['G_aa'] = max(worst.get('G_aa', 0.0), c3.rel(got['G_aa'][:, :, ii], ref['G_aa']))
        worst['B_sys'] = max(worst.get('B_sys', 0.0), c3.rel(got['B_sys'][:, ii], ref['B_sys']))
        worst['rhs_red'] = max(worst.get('rhs_red', 0.0), c3.rel(got['rhs_red'][ii], rd.rhs[ii]))
    print('worst deviation from the oracle', worst)
    assert all(w < TOL for w in worst.values()), worst


def test_padded_side_tables_are_cleared_per_listed_subdomain():
    """kc_3x1x2: sides with fewer faces than the padded tables hold.  The listed rows of Yb, Dp and Xab start as NaN: the padded rows
    come out as the zeros the whole pass's memset gives, the other subdomains' rows are not touched."""
    p, eng, _ = engine_case('kc_3x1x2')
    assert eng.S == 8 and bool((np.asarray(eng.t.side_elem) < 0).any())
    restricted_against_whole('kc_3x1x2', [0, 7], 1, poison=('Yb', 'Dp', 'Xab'))
    restricted_against_whole('kc_3x1x2', [0, 7], 1)


def test_three_components():
    """Q = 3: six A_aa pairs and 18 coupling operators per listed subdomain."""
    p, eng, _ = engine_case('q3_2x1x2')
    assert eng.Q == 3
    restricted_against_whole('q3_2x1x2', [1], 1)


@pytest.mark.parametrize('ksplit', [0, 2])
def test_phases_under_a_restriction(ksplit):
    """Phase 1 (own list) then phase 2 (side list) into the poisoned buffers: the whole pass (== phase 0) bit for bit."""
    restricted_against_whole('interior_3x3x3', [0, 13, 26], ksplit, exact=ksplit != 0, phases=True)
    import torch
    p, eng, V = engine_case('interior_3x3x3')
    Vd = eng.ctx.from_numpy(changed_basis(V, [0, 13, 26]))
    a, wa = whole_pass(eng, eng.ctx.from_numpy(V))
    b, wb = {k: x.clone() for k, x in a.items()}, wa.clone()
    eng.ctx.pass_set_subset([0, 13, 26])
    try:
        eng.ctx.project_estimate(eng.Q, Vd, eng.ops, wa, a, phase=0)
        eng.ctx.project_estimate(eng.Q, Vd, eng.ops, wb, b, phase=1)
        eng.ctx.project_estimate(eng.Q, Vd, eng.ops, wb, b, phase=2)
    finally:
        eng.ctx.pass_set_subset(None)
    torch.cuda.synchronize()
    assert torch.equal(wa, wb)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_a_lifted_restriction_and_refused_lists_leave_the_whole_pass():
    import ctypes
    import torch
    from pylrbms_amd._native import NativeError
    from pylrbms_amd._native3d import Native3DContext
    p, eng, V = engine_case('interior_3x3x3')
    Vd = eng.ctx.from_numpy(V)
    ref, ref_work = whole_pass(eng, Vd)

    def check_whole():
        out, work = whole_pass(eng, Vd)
        torch.cuda.synchronize()
        assert torch.equal(work, ref_work)
        for k in ref:
            assert torch.equal(out[k], ref[k]), k
    eng.ctx.pass_set_subset([13])
    eng.ctx.pass_set_subset(None)                                           # count = 0, changed = NULL
    check_whole()
    for bad in ([13, 4], [4, 4], [-1], [eng.S_ext], [0, 5, eng.S_ext]):   # descending, duplicate, out of range below / above
        with pytest.raises(NativeError, match=r'\(-1\): pass_set_subset: \w+'):      # LRBMS_E_INVALID with a message
            eng.ctx.pass_set_subset(bad)
        check_whole()
    one = (ctypes.c_int32 * 1)(3)
    rc = eng.ctx.lib.lrbms3_pass_set_subset(eng.ctx.handle, one, -1)
    assert rc == -1 and b'pass_set_subset' in eng.ctx.lib.lrbms3_last_error(eng.ctx.handle)
    check_whole()
    # a refused list does not replace a restriction that is in force
    eng.ctx.pass_set_subset([13])
    try:
        with pytest.raises(NativeError, match=r'\(-1\)'):
            eng.ctx.pass_set_subset([5, 5])
        out, work = whole_pass(eng, Vd, fill=0.0)
        torch.cuda.synchronize()
        v = views(eng, out, work, p['N'])
        assert float(v['G_nc'][13].abs().max()) > 0.0 and float(v['G_nc'][12].abs().max()) == 0.0
        assert float(v['Rb'][12].abs().max()) > 0.0 and float(v['Rb'][0].abs().max()) == 0.0
    finally:
        eng.ctx.pass_set_subset(None)
    check_whole()
    bare = Native3DContext(0)                                               # no mesh yet
    try:
        with pytest.raises(NativeError, match=r'\(-1\): pass_set_subset: mesh'):
            bare.pass_set_subset([0])
    finally:
        bare.close()


# ---------------------------------------------------------------------------------------------------------------- reductor
def problem_dict(p):
    return {'grid': p['grid'], 'lambda': {'functions': p['lambdas'], 'coefficients': p['thetas']}, 'lambda_bar': p['lambda_bar'],
            'lambda_hat': p['lambda_hat'], 'f': p['f'], 'mu_bar': p['mu_bar'], 'mu_hat': p['mu_hat']}


@functools.lru_cache(maxsize=None)
def case(name):
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import discretize
    p = c3.make_problem(name)
    d, _ = discretize(problem_dict(p), online_enrichment=True)
    return p, c3.oracle_of(p), d


def assert_same_model(rd, rd_ref, mus):
    """Outputs within the summation-order bound, solve and estimate within 1e-10 relative."""
    for k, want in rd_ref.out.items():
        if want is None:
            assert rd.out[k] is None
            continue
        err, scale = float((rd.out[k] - want).abs().max()), float(want.abs().max())
        assert err <= 1e-12 * max(scale, 1e-300), (k, err, scale)
    for mu in mus:
        u, u_ref = rd.solve(mu, rtol=1e-13), rd_ref.solve(mu, rtol=1e-13)
        assert float((u - u_ref).abs().max()) <= 1e-10 * float(u_ref.abs().max()), mu
        eta, eta_ref = rd.estimate(u, mu), rd_ref.estimate(u_ref, mu)
        assert abs(eta - eta_ref) <= 1e-10 * eta_ref, mu


def test_reductor_reserve_and_reduce_touched():
    from oracle.lrbms3d import Reductor3D
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    p, o, d = case('aniso_2x2x1')
    mu = p['mu']
    red = LRBMSReductor3D(d, order=0)
    red.extend_basis(d.solve(0.2, rtol=1e-12))
    assert red.reserve(3) == 4 and red.local_sizes() == [2] * o.S            # rounded to an even width; real vectors counted
    assert red.reserve(1000) == 64 // d.Q and red.reserve(2) == 64 // d.Q    # clamped to the limit of the pass; never shrinks
    red = LRBMSReductor3D(d, order=0)
    red.extend_basis(d.solve(0.2, rtol=1e-12))
    red.reserve(4)
    rd0 = red.reduce()
    assert red.last_reduce_info == {'incremental': False, 'own': o.S, 'side': o.S}
    assert rd0.solution_space.dim == 2 * o.S
    assert red.enrich_local_batch([0, 3], None, mu) == [0, 3]
    rd = red.reduce(touched=[0, 3])
    assert red.last_reduce_info == {'incremental': True, 'own': 2, 'side': 4}
    assert rd is not rd0 and rd.out['B_sys'] is rd0.out['B_sys'] and rd.out['G_bb'] is rd0.out['G_bb']      # shared arrays
    assert red.local_sizes() == [3, 2, 2, 3] and red.basis_size() == 4 and rd.solution_space.dim == 10
    fresh = LRBMSReductor3D(d, red.bases.clone())
    rd_f = fresh.reduce()
    assert fresh.last_reduce_info['incremental'] is False
    assert_same_model(rd, rd_f, (mu, 0.9))
    Vh = red.bases.cpu().numpy()
    ored = Reductor3D(o, [Vh[ii][:, :nl] for ii, nl in enumerate(red.local_sizes())])
    ord_ = ored.reduce()
    for m_ in (mu, 0.9):
        u, uo = rd.solve(m_, rtol=1e-13), ord_.solve(m_)
        assert c3.rel(red.reconstruct(u).cpu().numpy().ravel(), ored.reconstruct(uo)) < 1e-7
        eta_o = ord_.estimate(uo, m_)
        assert abs(rd.estimate(u, m_) - eta_o) < 1e-7 * eta_o
    # nothing changed: an incremental reduce that runs no kernel
    rd_same = red.reduce(touched=[])
    assert red.last_reduce_info == {'incremental': True, 'own': 0, 'side': 0}
    assert_same_model(rd_same, rd_f, (mu,))
    # a basis extended without telling reduce() is re-projected all the same (the reductor keeps track)
    assert red.enrich_local_batch([1], None, mu) == [1]
    rd_dirty = red.reduce(touched=[])
    assert red.last_reduce_info == {'incremental': True, 'own': 1, 'side': 3}
    assert_same_model(rd_dirty, LRBMSReductor3D(d, red.bases.clone()).reduce(), (mu,))
    # the slab grows past the reserved width: the whole pass, into fresh arrays
    for m_ in (0.9, 0.5, 1.2, 0.15):
        red.enrich_local_batch([0], None, m_)
        if red.basis_size() > 4:
            break
    assert red.basis_size() == 5
    rd_grown = red.reduce(touched=[0])
    assert red.last_reduce_info == {'incremental': False, 'own': o.S, 'side': o.S}
    assert rd_grown.out['B_sys'] is not rd.out['B_sys'] and rd_grown.N == 5
    assert_same_model(rd_grown, LRBMSReductor3D(d, red.bases.clone()).reduce(), (mu,))
    red.reduce()                                                             # reduce() with no argument: the whole pass, as ever
    assert red.last_reduce_info == {'incremental': False, 'own': o.S, 'side': o.S}


def test_affine_source_projections_are_updated_in_place():
    import torch
    import affine_source3d_ref as asr
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D, discretize
    p = c3.make_problem('aniso_2x2x1')
    d, _ = discretize(asr.problem_dict(p))
    eng = d.engine
    V = c3.make_bases3d(eng.S, eng.t.n, p['N'], seed=3)
    red = LRBMSReductor3D(d, V)
    red.reserve(6)
    rd0 = red.reduce()
    kept = rd0.rhs_red_K, rd0.r_fd_K
    rng = np.random.default_rng(5)
    red.extend_basis_local(1, eng.ctx.from_numpy(rng.standard_normal(eng.t.n)))
    rd = red.reduce(touched=[1])
    assert red.last_reduce_info == {'incremental': True, 'own': 1, 'side': 3}
    assert rd.rhs_red_K is kept[0] and rd.r_fd_K is kept[1] and rd.out['rhs_red'] is None and rd.out['r_fd'] is None
    rd_f = LRBMSReductor3D(d, red.bases.clone()).reduce()
    other = torch.as_tensor([0, 2, 3], device=rd.rhs_red_K.device)
    for got, want in ((rd.rhs_red_K, rd_f.rhs_red_K), (rd.r_fd_K, rd_f.r_fd_K)):
        assert tuple(got.shape) == tuple(want.shape) and got.shape[0] == 2
        assert torch.equal(got[:, other], want[:, other])
        assert float(got[:, 1].abs().max()) > 0.0
        assert float((got[:, 1] - want[:, 1]).abs().max()) <= 1e-12 * float(want.abs().max())
    assert_same_model(rd, rd_f, (0.3, 0.8))                                    # on both sides of the source's switch


def test_adaptive_enrichment_loop_re_projects_incrementally():
    """The loop of test_adaptive_enrichment_loop_in_3d twice: as it is (incremental from the round after the reserve on) and with a
    reductor forced to whole re-reduction.  Same sizes, eta and energy errors to 1e-9."""
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    from pylrbms_amd.online_enrichment import AdaptiveEnrichment
    p, o, d = case('interior_3x3x3')
    mu = p['mu']
    want = o.solve(mu)

    class WholeReductor(LRBMSReductor3D):
        def reduce(self, touched=None):
            return LRBMSReductor3D.reduce(self)

    def run(cls):
        red = cls(d, order=0)
        history = []

        def callback(rd, U, mu_, data):
            err = red.reconstruct(U).cpu().numpy().ravel() - want
            history.append(dict(data, energy_error=np.sqrt(o.energy_norm2(err, mu_)), info=dict(red.last_reduce_info)))
        loop = AdaptiveEnrichment(problem_dict(p), d, d.solution_space, red, red.reduce(), target_error=0.0,
                                  marking_doerfler_theta=0.5, marking_max_age=2)
        loop.solve(mu, enrichment_steps=3, callback=callback)
        return red, history
    red, inc = run(LRBMSReductor3D)
    _, whole = run(WholeReductor)
    assert len(inc) == len(whole) == 4
    print('reduce info per round', [h['info'] for h in inc])
    assert red.basis_size() == 4                                              # 1 + 3 reserved in front of the first round
    assert [h['info']['incremental'] for h in inc] == [False, False, True, True]      # round 1 widens the slab (the reserve)
    assert not any(h['info']['incremental'] for h in whole)
    for h in inc[2:]:
        assert 0 < h['info']['own'] <= h['info']['side'] <= o.S
    for a, b in zip(inc, whole):
        assert a['local RB sizes'] == b['local RB sizes'] and a['local_problem_solves'] == b['local_problem_solves']
        assert abs(a['eta'] - b['eta']) <= 1e-9 * b['eta']
        assert abs(a['energy_error'] - b['energy_error']) <= 1e-9 * b['energy_error']
    assert inc[-1]['global RB size'] > inc[0]['global RB size']
