"""The cells of tests/test_dispatch_parity3d_gpu.py select every k3_pg instantiation of the 3D pass (CPU only).

``dispatch_pg`` in csrc/lrbms3d.hip lists its (RT, CT) tile shapes as PGCASE(R, C); ``launch_pg`` instantiates k3_pg<KIND, R, C,
EVEN> for both forms where R and C are even and picks EVEN = true when N is even too.  The timing names of the 3D kernels do not
carry the tile shape, so this mirror of the host's choice stands in for name assertions: a new instantiation, a dead one, or a
dropped cell fails here instead of going untested on the GPU."""
import re

from common3d import source3d
from test_dispatch_parity3d_gpu import CELLS

SQUARE = ('AAA', 'SYS', 'NC', 'CPL', 'BB')
KINDS = SQUARE + ('AB',)


def listed_cases():
    """{kind: [(R, C), ...]} from the PGCASE lists of dispatch_pg."""
    src = source3d()
    body = re.search(r'int dispatch_pg\(.*?\n}\n', src, re.S).group(0)
    lists = dict(re.findall(r'if constexpr \(KIND (==|!=) G_AB\) \{([^}]*)\}', body))
    assert set(lists) == {'==', '!='}, 'dispatch_pg: expected one PGCASE list for AB and one for the other kinds'

    def cases(text):
        return [(int(r), int(c)) for r, c in re.findall(r'PGCASE\((\d+),\s*(\d+)\)', text)]

    out = {k: cases(lists['!=']) for k in SQUARE}
    out['AB'] = cases(lists['=='])
    return out


def instantiations(kinds):
    """Every (kind, R, C, EVEN) template instance launch_pg compiles for the listed tile shapes."""
    return {(k, r, c, even) for k, rcs in kinds.items() for r, c in rcs for even in ((False, True) if r % 2 == 0 and c % 2 == 0 else (False,))}


def selected(Q, N):
    """The (kind, R, C, EVEN) instances one pass at (Q, N) launches: the host's tile counts and EVEN choice."""
    tn, tq = (N + 15) // 16, (Q * N + 15) // 16
    tiles = {k: (tn, tn) for k in ('AAA', 'SYS', 'NC', 'CPL')}
    tiles['AB'], tiles['BB'] = (tn, tq), (tq, tq)
    return {(k, r, c, r % 2 == 0 and c % 2 == 0 and N % 2 == 0) for k, (r, c) in tiles.items()}


def reachable():
    """Over every shape the pass takes (1 <= Q <= 8, 1 <= N, Q N <= 64)."""
    return set().union(*(selected(Q, N) for Q in range(1, 9) for N in range(1, 64 // Q + 1)))


def test_every_listed_instantiation_is_reachable():
    dead = instantiations(listed_cases()) - reachable()
    assert not dead, 'instantiations no (Q, N) the pass takes can select: {}'.format(sorted(dead))


def test_every_reachable_tile_shape_is_listed():
    listed = listed_cases()
    missing = {(k, r, c) for k, r, c, _ in reachable() if (r, c) not in listed[k]}
    assert not missing, 'tile shapes dispatch_pg would refuse: {}'.format(sorted(missing))


def test_the_cells_select_every_instantiation():
    for Q, N, P, kc in CELLS:
        assert 1 <= Q <= 8 and 1 <= N and Q * N <= 64, (Q, N)
        assert len(P) == 3 and sum(x > 1 for x in P) >= 2, P        # neighbours in more than one direction
    hit = set().union(*(selected(Q, N) for Q, N, _, _ in CELLS))
    missed = instantiations(listed_cases()) - hit
    assert not missed, 'no cell of test_dispatch_parity3d_gpu.py runs: {}'.format(sorted(missed))

