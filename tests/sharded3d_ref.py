"""Rank views of a sharded 3D / P2 run in ONE process, for tests: every rank of a tiling is emulated one after the
other -- ``Engine3D`` on the grid as rank r sees it, ``V [S_ext, n, N]`` pre-filled on the host exactly as the halo exchange would
fill it -- and the CPU oracle on the global mesh is restricted and re-indexed to the view.  No ``torch.distributed``, no processes.

The contract under test (include/lrbms3d_hip.h): every kernel of the assembly and of the pass indexes neighbours through
``nbr [S][7]`` into the S_ext ordering, reads ``lam``, ``Cf`` and ``phys`` of halo subdomains, and of a halo slab of ``V`` only the
cube layer next to the shared side (``parallel.side_rows3d``); every other row of a halo slab stays NaN here."""
import numpy as np

import common3d as c3

SHIFTED_DOMAIN = ([-1.0, 0.5, 2.0], [1.0, 1.5, 2.75])        # shifted, non-cubic: a wrong halo origin samples other coefficients

_Q2 = ([c3._one, c3._lam1], [lambda mu: 1.0, lambda mu: mu])
_Q3 = ([c3._one, c3._lam1, c3._lam2], [lambda mu: 1.0, lambda mu: mu, lambda mu: mu * mu])

# name: domain (None = unit cube), P, k_c, {world: tile grid}, (lambdas, thetas), kappa, N, mu.  The smallest shapes that reach each
# index path of a view with S_ext > S:
CASES = {
    # halo across +-z alone (sides 0 and 5, slots 0 and 6)
    'z2': dict(domain=None, P=(1, 1, 2), kc=(2, 1, 2), worlds={2: (1, 1, 2)}, data=_Q2, kappa=np.eye(3), N=4, mu=0.3),
    # +-y, one cube off the split axis
    'y2': dict(domain=None, P=(1, 2, 1), kc=(1, 2, 1), worlds={2: (1, 2, 1)}, data=_Q2, kappa=np.eye(3), N=4, mu=0.7),
    # one cube ALONG the split axis: the exchanged layer is the whole slab
    'x2_thin': dict(domain=None, P=(2, 1, 1), kc=(1, 2, 2), worlds={2: (2, 1, 1)}, data=_Q2, kappa=np.eye(3), N=4, mu=0.45),
    # ranks 1 and 2: halo across both z sides and no local neighbour at all
    'z4_line': dict(domain=None, P=(1, 1, 4), kc=(1, 1, 2), worlds={4: (1, 1, 4)}, data=_Q2, kappa=np.eye(3), N=4, mu=0.8),
    # the tiling of config 5: S = 1, S_ext = 4 at 8 ranks; six side tables of three different sizes, anisotropic kappa
    'cube8': dict(domain=SHIFTED_DOMAIN, P=(2, 2, 2), kc=(3, 1, 2), worlds={8: (2, 2, 2), 2: (1, 1, 2), 4: (1, 2, 2)}, data=_Q3,
                  kappa=c3.KAPPA_ANISO, N=6, mu=0.6),
}
RUNS = [(name, world) for name, case in CASES.items() for world in case['worlds']]


def problem_of(name):
    """The case as a problem of ``common3d.make_problem`` (global grid, world size 1)."""
    case = CASES[name]
    lams, thetas = case['data']
    return c3.make_problem(name, domain=case['domain'], spec=(list(case['P']), case['kc'], lams, thetas, case['kappa'], case['N'],
                                                               case['mu']))


def rank_grids(domain, P, kc, world, kappa):
    """(grids, plans): the ``DDSubdomainsGrid3D`` and the ``HaloPlan`` of every rank of ``world``.  A plan carries its grid as
    ``plan.grid`` (the helper's own attribute; the plan itself is what production builds from the grid factory alone)."""
    from pylrbms_amd.grid3d import make_grid3d
    from pylrbms_amd.parallel import HaloPlan
    domain = c3.UNIT_DOMAIN if domain is None else domain
    grids = [make_grid3d(domain=domain, num_subdomains=P, cubes_per_subdomain_and_dim=kc, rank=r, world_size=world, kappa=kappa)
             for r in range(world)]
    plans = [HaloPlan(lambda q: grids[q], world, r) for r in range(world)]
    for r, plan in enumerate(plans):
        plan.grid = grids[r]
    return grids, plans


def view_of(grid):
    """(local, halo): the global ids behind the S_ext ordering of a rank (as ``Engine3D`` and ``HaloPlan`` derive them)."""
    local = list(grid.subdomains_on_rank)
    halo = sorted({int(j) for s in local for j in grid.neighboring_subdomains(s)} - set(local))
    return local, halo


def _send_buffer(plan, Vg, N):
    """What rank ``plan.rank`` hands to the all-to-all: the rows ``a2a_pack_index`` of its local slabs, ordered by peer."""
    local, _ = view_of(plan.grid)
    flat = np.ascontiguousarray(Vg[local]).reshape(len(local) * plan.n, N)
    assert plan.a2a_pack_index.size == 0 or int(plan.a2a_pack_index.max()) < flat.shape[0], 'the exchange packs a halo row'
    assert len(plan.a2a_pack_index) == sum(plan.a2a_send_splits)
    return flat[plan.a2a_pack_index]


def fill_view(plan_r, plans, Vg, N):
    """Host array [S_ext, n, N] of rank ``plan_r.rank``: the local slabs from the global ``Vg [S_global, n, N]``, the halo slabs all
    NaN and then filled as ``HaloExchange`` (all-to-all mode) fills them -- the receive buffer is the peers' send buffers' shares
    for this rank in rank order (``a2a_send_splits`` of the peer against ``a2a_recv_splits`` here), scattered by ``a2a_unpack_dst``."""
    r = plan_r.rank
    local, halo = view_of(plan_r.grid)
    assert (plan_r.S, plan_r.S_ext) == (len(local), len(local) + len(halo))
    V = np.full((plan_r.S_ext, plan_r.n, N), np.nan)
    V[:plan_r.S] = Vg[local]
    recv = []
    for q, peer in enumerate(plans):
        if q == r:
            assert plan_r.a2a_recv_splits[q] == 0 and peer.a2a_send_splits[q] == 0
            continue
        off = sum(peer.a2a_send_splits[:r])
        part = _send_buffer(peer, Vg, N)[off:off + peer.a2a_send_splits[r]]
        assert part.shape[0] == plan_r.a2a_recv_splits[q], 'rank {} sends {} rows to {}, which expects {}'.format(
            q, part.shape[0], r, plan_r.a2a_recv_splits[q])
        recv.append(part)
    recv = np.concatenate(recv) if recv else np.zeros((0, N))
    assert recv.shape[0] == len(plan_r.a2a_unpack_dst)
    dst = plan_r.a2a_unpack_dst
    assert dst.size == 0 or int(dst.min()) >= plan_r.S * plan_r.n, 'the exchange writes a local slab'
    V.reshape(-1, N)[dst] = recv
    return V


def halo_sides(grid):
    """Per halo subdomain (in the S_ext order behind the local ones): the sides of THAT subdomain which face a local one."""
    from pylrbms_amd.grid3d import SIDE_TO_SLOT
    local, halo = view_of(grid)
    return [[sd for sd in range(6) if int(grid.neighbor_slots[s, SIDE_TO_SLOT[sd]]) in local] for s in halo]


def local_halo_sides(grid):
    """The sides of the rank's LOCAL subdomains behind which a halo subdomain lies (a set of side indices 0 .. 5)."""
    from pylrbms_amd.grid3d import SIDE_TO_SLOT
    local, halo = view_of(grid)
    return {sd for s in local for sd in range(6) if int(grid.neighbor_slots[s, SIDE_TO_SLOT[sd]]) in halo}


def global_assembled(p, d):
    """``common3d.oracle_assembled`` of the global problem, computed once per problem."""
    if '_assembled' not in p:
        p['_assembled'] = c3.oracle_assembled(p, d)
    return p['_assembled']


def oracle_view(p, d, rd, eng):
    """The oracle of the global problem ``p`` (discretization ``d``, reduced model ``rd``) as rank ``eng`` sees it:
        ops     the assembled arrays of ``common3d.oracle_assembled`` restricted to ``eng.local`` -- ``Cf`` to ``eng.ext`` (the flux
                coefficients of a halo subdomain come from ``lam`` sampled at ITS origin: the check of the halo samples);
        dense  ``common3d.oracle_dense_blocks`` of every local subdomain (slots are geometric: the same in every view);
        rhs     the projected right-hand sides of the local subdomains."""
    full = global_assembled(p, d)
    loc, ext = list(eng.local), list(eng.ext)
    sub_axis = dict(A_diag=1, A_cpl=1, Aaa=2, Aab=1)
    ops = {k: np.take(v, ext if k == 'Cf' else loc, axis=1 if k == 'Cf' else sub_axis.get(k, 0)) for k, v in full.items()}
    return dict(ops=ops, dense=[c3.oracle_dense_blocks(p, d, rd, g) for g in loc], rhs=[rd.rhs[g] for g in loc])
