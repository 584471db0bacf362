"""pylrbms_amd._build.SOURCES and the files of csrc/ agree (CPU only): a translation unit that is not listed would be missing from
the library and fail at load time on the GPU; a listed one that does not exist fails the build."""
import os

from pylrbms_amd import _build


def test_sources_lists_every_translation_unit():
    on_disk = sorted(f for f in os.listdir(_build.CSRC) if f.endswith('.hip'))
    assert sorted(_build.SOURCES) == on_disk and len(set(_build.SOURCES)) == len(_build.SOURCES)


def test_source_reading_tests_see_every_3d_unit():
    """tests/common3d.py finds the 3D files by name: what the source-reading tests concatenate is every 3D unit of SOURCES."""
    from common3d import CSRC, sources3d
    names = sources3d()
    assert all(os.path.isfile(os.path.join(CSRC, f)) for f in names) and len(set(names)) == len(names)
    assert {f for f in _build.SOURCES if '3d' in f} == {f for f in names if f.endswith('.hip')}


def test_every_3d_kernel_has_one_home():
    """Every ``__global__ ... void k3...`` of the 3D files is defined in exactly one of them and none in the shared header: a second
    file reaches a kernel through the ``launch_*`` function of its home file ("Where what lives")."""
    import re
    from common3d import CSRC, sources3d
    homes, marks = {}, 0
    for f in sources3d():
        text = open(os.path.join(CSRC, f)).read()
        if f.endswith('.h'):
            assert '__global__' not in text, f
        marks += text.count('__global__')
        for name in re.findall(r'__global__[^;{\n]*?\bvoid\s+(k3\w*)\s*\(', text):
            homes.setdefault(name, []).append(f)
    assert sum(len(h) for h in homes.values()) == marks                      # the pattern has seen every kernel
    assert len(homes) > 50 and {f for h in homes.values() for f in h} == {f for f in sources3d() if f.endswith('.hip')}
    assert {k: h for k, h in homes.items() if len(h) != 1} == {}
