#!/bin/bash
# Variant builds of the resident loop for same-box A/Bs (tools/ab_resident.sh
# with AB_GLOB=tools/micro/_var/*.so): tools/micro/_var/<name>.so per
# "name:flags" argument, e.g.
#   tools/micro/resident_variants.sh "slp:" "nobar:-fno-slp-vectorize -DPP2_RES_NOBAR"
# The flags replace the Makefile's EXTRA_pp2_resident.hip (-fno-slp-vectorize:
# repeat it unless the variant is about it).
# Only pp2_resident.hip is rebuilt per variant (the other objects are copied
# from the in-tree build, which must be current: run make there first).
set -eo pipefail
cd "$(dirname "$0")/../.."
CS=path_planning_2d_amd/csrc
V=tools/micro/_var
mkdir -p $V
for spec in "$@"; do
  name=${spec%%:*}
  flags=${spec#*:}
  obj=$PWD/$V/obj_$name
  rm -rf "$obj"
  cp -a $CS/build "$obj"
  rm -f "$obj/pp2_resident.hip.o"
  make -s -C $CS OBJDIR="$obj" OUT="$PWD/$V/$name.so" "EXTRA_pp2_resident.hip=$flags" "$PWD/$V/$name.so"
  echo "built $V/$name.so ($flags)"
done
