#!/bin/bash
# usage: [SRC=file.hip] tools/build_variant.sh NAME [extra hipcc flags...]  -> pylrbms_amd/_variants/NAME.so (git-ignored)
# Only SRC is recompiled with the extra flags (default fused.hip): a bare file name is taken from pylrbms_amd/csrc, a path is
# compiled as given (an edited copy) and stands in for the file of csrc with the same name.  Every other object of
# pylrbms_amd._build.SOURCES comes from the regular build.
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=${SRC:-fused.hip}
case "$SRC" in */*) ;; *) SRC=$ROOT/pylrbms_amd/csrc/$SRC ;; esac
[ -f "$SRC" ] || { echo "build_variant.sh: no such file: $SRC" >&2; exit 1; }
STEM=$(basename "$SRC" .hip)
python3 -c "import sys; sys.path.insert(0, '$ROOT'); from pylrbms_amd._build import build_native; build_native()"
mkdir -p $ROOT/pylrbms_amd/_variants /tmp/var_$NAME
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -DLRBMS_EXPERIMENT_BUILD "$@" -I$ROOT/pylrbms_amd/csrc -c "$SRC" -o /tmp/var_$NAME/$STEM.o
OBJS=$(python3 -c "import sys; sys.path.insert(0, '$ROOT'); from pylrbms_amd._build import SOURCES; assert '$STEM.hip' in SOURCES, '$STEM.hip is not in SOURCES'; print(' '.join('$ROOT/pylrbms_amd/csrc/_obj/' + s[:-4] + '.o' for s in SOURCES if s != '$STEM.hip'))")
hipcc --offload-arch=gfx950 -shared -fPIC -o $ROOT/pylrbms_amd/_variants/$NAME.so $OBJS /tmp/var_$NAME/$STEM.o -L/opt/rocm/lib -lrocsolver -lrocblas
echo built $ROOT/pylrbms_amd/_variants/$NAME.so
