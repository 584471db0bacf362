#!/bin/bash
# usage: [SRC=file.hip] tools/build_variant3d.sh NAME [extra hipcc flags...]  -> pylrbms_amd/_variants/NAME.so: the 3D counterpart of
# tools/build_variant.sh.  SRC defaults to lrbms3d.hip, the file that reads -DFLUX_LOOP / -DNODE_LOOP.
SRC=${SRC:-lrbms3d.hip} exec "$(dirname "$0")/build_variant.sh" "$@"
