"""The rank views of tests/sharded3d_ref.py on the CPU: what ``fill_view`` puts into the halo slabs is what the exchange plan of
production moves -- per halo subdomain exactly the cube layers (``parallel.side_rows3d``) next to the sides that face a local
subdomain, the owner's rows, every other row NaN -- and the case list reaches what tests/test_sharded3d_views_gpu.py claims to
cover: every one of the six sides as a halo side, a rank with halo across both sides of one axis, and per axis a case in which rows
of a halo slab stay NaN (so that "the kernels read only the layer" is a check and not vacuous)."""
import numpy as np
import pytest

import sharded3d_ref as sr

from pylrbms_amd.grid3d import SIDE_AXIS, tile_grid3d
from pylrbms_amd.parallel import side_rows3d

N = 3


def _views(name, world):
    case = sr.CASES[name]
    grids, plans = sr.rank_grids(case['domain'], case['P'], case['kc'], world, case['kappa'])
    t = grids[0].template
    Vg = np.random.default_rng(17).standard_normal((grids[0].num_subdomains, t.n, N))
    return case, grids, plans, Vg


@pytest.mark.parametrize('name,world', sr.RUNS)
def test_tile_grid_of_the_case(name, world):
    case = sr.CASES[name]
    assert tile_grid3d(world, list(case['P'])) == case['worlds'][world]


@pytest.mark.parametrize('name,world', sr.RUNS)
def test_halo_slabs_hold_the_layers_the_plan_moves_and_nan_elsewhere(name, world):
    case, grids, plans, Vg = _views(name, world)
    owned = sorted(s for g in grids for s in g.subdomains_on_rank)
    assert owned == list(range(grids[0].num_subdomains))                       # a partition
    for r, grid in enumerate(grids):
        local, halo = sr.view_of(grid)
        V = sr.fill_view(plans[r], plans, Vg, N)
        S, t = len(local), grid.template
        assert V.shape == (S + len(halo), t.n, N) and len(halo) > 0, 'S_ext > S on every rank'
        assert np.array_equal(V[:S], Vg[local])
        rows = side_rows3d(t)
        sides = sr.halo_sides(grid)
        for h, s in enumerate(halo):
            assert len(sides[h]) >= 1
            want = np.zeros(t.n, dtype=bool)
            for sd in sides[h]:
                want[rows[sd]] = True
            filled = ~np.isnan(V[S + h]).any(axis=1)
            assert np.array_equal(filled, want), (name, world, r, s)
            assert np.isnan(V[S + h][~want]).all()                                # no half-written row
            assert np.array_equal(V[S + h][want], Vg[s][want]), (name, world, r, s)   # ... and the owner's values


def test_the_cases_reach_every_side_both_sides_of_an_axis_and_leave_rows_unfilled():
    seen, two_sided, nan_left = set(), [], {0: [], 1: [], 2: []}
    for name, world in sr.RUNS:
        case, grids, plans, Vg = _views(name, world)
        for r, grid in enumerate(grids):
            mine = sr.local_halo_sides(grid)
            seen |= mine
            for lo, hi in ((2, 3), (1, 4), (0, 5)):
                if lo in mine and hi in mine:
                    two_sided.append((name, world, r, SIDE_AXIS[lo]))
            V = sr.fill_view(plans[r], plans, Vg, N)
            S = plans[r].S
            for h, sides in enumerate(sr.halo_sides(grid)):
                left = int(np.isnan(V[S + h]).any(axis=1).sum())
                if left:
                    for sd in sides:
                        nan_left[SIDE_AXIS[sd]].append((name, world, r, left))
    assert seen == set(range(6)), seen
    assert two_sided, 'no rank with halo across both sides of one axis'
    assert ('z4_line', 4, 1, 2) in two_sided and ('z4_line', 4, 2, 2) in two_sided
    for axis in range(3):
        assert nan_left[axis], 'axis {}: every halo slab is exchanged whole'.format(axis)
    # one cube along the split axis: the layer is the whole slab, nothing stays NaN
    case, grids, plans, Vg = _views('x2_thin', 2)
    for r in range(2):
        assert not np.isnan(sr.fill_view(plans[r], plans, Vg, N)).any()


def test_unequal_side_tables_and_the_shifted_domain_of_cube8():
    case, grids, plans, Vg = _views('cube8', 8)
    t = grids[0].template
    assert len({len(rw) for rw in side_rows3d(t)}) == 3                            # layers of 2, 6 and 3 cubes
    assert all(len(sr.view_of(g)[0]) == 1 and len(sr.view_of(g)[1]) == 3 for g in grids)
    p = sr.problem_of('cube8')
    assert np.array_equal(p['grid'].lower_left, [-1.0, 0.5, 2.0]) and np.array_equal(p['grid'].upper_right, [1.0, 1.5, 2.75])
    import common3d as c3
    d = c3.oracle_of(p)
    assert np.array_equal(d.mesh.lower_left, p['grid'].lower_left) and np.allclose(d.mesh.vertices.max(axis=0), [1.0, 1.5, 2.75])
    assert d.Q == 3 and d.S == 8 and d.n == t.n
    # the default stays the unit cube
    q = c3.make_problem('q1_strip')
    assert np.array_equal(q['grid'].lower_left, [0.0] * 3) and np.array_equal(c3.oracle_of(q).mesh.upper_right, [1.0] * 3)
