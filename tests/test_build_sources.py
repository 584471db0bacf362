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
