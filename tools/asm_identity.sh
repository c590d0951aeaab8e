#!/bin/sh
# asm_identity.sh REV [FILE...] [-D...]: is the gfx950 device assembly of the
# working tree's csrc files (default pp2_resident.hip) that of commit REV?
# Both trees are compiled with their own Makefile's command line (make -n) plus
# the given -D flags; the __hip_cuid_ symbol hashes the source text and is
# dropped.  Exits 1 at the first difference, naming the kernel it falls in.
# Prints one line per file.  Needs no GPU.
set -eu
rev=$1; shift
files= defs=
for a; do case $a in -D*) defs="$defs $a" ;; *) files="$files $a" ;; esac; done
root=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
mkdir "$tmp/rev"
git -C "$root" archive "$rev" path_planning_2d_amd/csrc include | tar -x -C "$tmp/rev"

asm() {  # asm TREE FILE OUT: the Makefile's compile line, to device assembly
  cmd=$(make -n -B -C "$1/path_planning_2d_amd/csrc" OBJDIR="$tmp/obj" EXTRA_FLAGS="$defs" \
          "$tmp/obj/$2.o" | grep -e ' -c -o ')
  cmd=$(printf '%s' "$cmd" | sed "s| -c -o [^ ]*| --cuda-device-only -S -o $3.raw|")
  (cd "$1/path_planning_2d_amd/csrc" && eval "$cmd")
  grep -v __hip_cuid_ "$3.raw" > "$3"
}

for f in ${files:-pp2_resident.hip}; do
  asm "$tmp/rev" "$f" "$tmp/$f.rev.s" & asm "$root" "$f" "$tmp/$f.new.s"; wait $!
  lines=$(wc -l < "$tmp/$f.new.s")
  kernels=$(grep -c '^[[:space:]]*\.amdhsa_kernel ' "$tmp/$f.new.s" || true)
  if n=$(cmp "$tmp/$f.rev.s" "$tmp/$f.new.s" | sed 's/.* line //'); [ -z "$n" ]; then
    echo "$f$defs: identical to $rev ($lines lines, $kernels kernels)"
  else
    k=$(awk -v n="$n" 'NR > n { exit } /^[_A-Za-z][A-Za-z0-9_$.]*:/ { k = $1 } END { print k }' \
          "$tmp/$f.new.s")
    echo "$f$defs: DIFFERS from $rev at line $n, in ${k%:}"; exit 1
  fi
done
