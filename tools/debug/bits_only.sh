export TMPDIR=/tmp
OUT=${OUT:-out}          # where the log goes
mkdir -p "$OUT"
( SMART_AMD_LIB=$PWD/smartpy_amd/csrc/libsmart_amd_oldsteps.so timeout 900 python tools/debug/steps_bits.py dump /tmp/b_old.npz
  SMART_AMD_LIB=$PWD/smartpy_amd/csrc/libsmart_amd_wetasm0.so timeout 900 python tools/debug/steps_bits.py dump /tmp/b_wet0.npz
  timeout 900 python tools/debug/steps_bits.py dump /tmp/b_new.npz
  echo "== -DSMART_STEP_ARMS=0 (compiled step loop of round 2) against the shipped library"
  python tools/debug/steps_bits.py compare /tmp/b_old.npz /tmp/b_new.npz
  echo "== -DSMART_WET_ASM=0 (hipcc's wet-interval loop) against the shipped library"
  python tools/debug/steps_bits.py compare /tmp/b_wet0.npz /tmp/b_new.npz ) > "$OUT"/r03_steps_bits.txt 2>&1
grep -c . "$OUT"/r03_steps_bits.txt; grep "differ\|==" "$OUT"/r03_steps_bits.txt
