#!/bin/bash
# Build the library of a git revision next to the working tree's, for a same-box A/B (the revision must speak the
# working tree's ABI):   bash tools/build_rev_variant.sh <rev> <name>  ->  tools/variants/libsmart_amd_<name>.so
# then on the GPU box:   bash tools/ab_variants.sh tools/variants/libsmart_amd_<name>.so
REV=${1:-HEAD}; NAME=${2:-prev}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
TMP=$(mktemp -d)
git -C $ROOT archive $REV smartpy_amd/csrc smartpy_amd/build.py smartpy_amd/isa_lint.py include | tar -x -C $TMP
mkdir -p $ROOT/tools/variants
# (build.py imports its sibling isa_lint: the revision's two files as a package of their own, under another name)
mv $TMP/smartpy_amd $TMP/rev_pkg && touch $TMP/rev_pkg/__init__.py
python3 - <<PY
import shutil, sys
sys.path.insert(0, '$TMP')
from rev_pkg import build as b
out = b.build(force=True, lib_path=b.LIB)
shutil.copy(out, '$ROOT/tools/variants/libsmart_amd_$NAME.so')
print('$ROOT/tools/variants/libsmart_amd_$NAME.so')
PY
rm -rf $TMP
