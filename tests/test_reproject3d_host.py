"""Incremental re-projection on the 3D / P2 path, the parts that need no GPU: the side list of
``lrbms3_pass_set_subset`` (``grid3d.side_targets``) and the dependency structure it rests on -- which targets' projected
operators change when a local basis changes -- checked bit for bit on the CPU oracle."""
import functools
import os
import re

import numpy as np
import pytest

import common3d as c3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTRE = [4, 10, 12, 13, 14, 16, 22]
THREE = [0, 1, 3, 4, 9, 10, 12, 13, 14, 16, 17, 22, 23, 25, 26]


def test_side_targets_on_the_3x3x3_grid():
    from pylrbms_amd.grid3d import side_targets
    slots = c3.make_problem('interior_3x3x3')['grid'].neighbor_slots
    assert side_targets(slots, [13]) == CENTRE
    assert side_targets(slots, [0, 13, 26]) == THREE
    assert side_targets(slots, []) == []
    assert side_targets(slots, list(range(27))) == list(range(27))
    assert side_targets(slots, np.array([26, 0, 13])) == THREE            # any order, any integer sequence


def test_side_targets_of_a_changed_halo_slab():
    """A rank-local table [S, 7] whose entries index the S_ext ordering: a changed halo slab (index >= S) lists its local
    neighbours, never itself."""
    from pylrbms_amd.grid3d import side_targets
    nbr = np.full((2, 7), -1, dtype=np.int32)
    nbr[:, 3] = [0, 1]
    nbr[0, 4], nbr[1, 2] = 1, 0           # 0 | 1 along x
    nbr[1, 4] = 2                         # 1 | halo slab 2
    assert side_targets(nbr, [2]) == [1]
    assert side_targets(nbr, [0, 2]) == [0, 1]
    assert side_targets(nbr, [3]) == []


@functools.lru_cache(maxsize=None)
def _oracle_case():
    p = dict(c3.make_problem('interior_3x3x3'), N=3)
    d = c3.oracle_of(p)
    V = c3.make_bases3d(d.S, d.n, 3, seed=5)
    return p, d, V, _blocks(p, d, V)


def _blocks(p, d, V):
    rd = c3.reduce_with_oracle(p, d, V)
    return [dict(c3.oracle_dense_blocks(p, d, rd, ii), rhs=np.asarray(rd.rhs[ii])) for ii in range(d.S)]


@pytest.mark.parametrize('changed, side', [([13], CENTRE), ([0, 13, 26], THREE)], ids=['centre', 'corners_and_centre'])
def test_oracle_operators_change_on_the_side_list_only(changed, side):
    """The last basis column of the changed subdomains replaced: the oracle's projected operators and right-hand side of every
    target outside the side list are bit-identical before and after, those of every target inside it differ."""
    from pylrbms_amd.grid3d import side_targets
    p, d, V, before = _oracle_case()
    assert side_targets(p['grid'].neighbor_slots, changed) == side
    V2 = V.copy()
    rng = np.random.default_rng(17)
    for ii in changed:
        V2[ii, :, -1] = rng.standard_normal(d.n)
    after = _blocks(p, d, V2)
    differ = [ii for ii in range(d.S) if any(not np.array_equal(before[ii][k], after[ii][k]) for k in before[ii])]
    assert differ == side


def test_the_new_export_is_declared_exported_and_bound():
    import ctypes
    from pylrbms_amd._build import build_native
    from pylrbms_amd._native3d import SIGNATURES3, Native3DContext
    name = 'lrbms3_pass_set_subset'
    with open(os.path.join(ROOT, 'include', 'lrbms3d_hip.h')) as fh:
        m = re.search(r'\bint {}\(([^;]*)\);'.format(name), fh.read())
    assert m, '{} is not declared in include/lrbms3d_hip.h'.format(name)
    assert hasattr(ctypes.CDLL(build_native()), name), '{} is not exported'.format(name)
    assert name in SIGNATURES3 and len(SIGNATURES3[name][1]) == m.group(1).count(',') + 1
    assert hasattr(Native3DContext, 'pass_set_subset')


def test_the_reductor_offers_what_the_enrichment_loop_looks_for():
    import inspect
    from pylrbms_amd.discretize_elliptic_block_swipdg_3d import LRBMSReductor3D
    from pylrbms_amd.discretize_parabolic_block_swipdg_3d import ParabolicLRBMSReductor3D
    assert 'touched' in inspect.signature(LRBMSReductor3D.reduce).parameters and hasattr(LRBMSReductor3D, 'reserve')
    assert 'touched' not in inspect.signature(ParabolicLRBMSReductor3D.reduce).parameters      # keeps the whole re-reduction
