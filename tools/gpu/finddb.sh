# NORMAL-mode MIOpen search for the bench step's convolutions under AMP fp16 (and bf16 / fp32 entries kept),
# seeded with the shipped find-db, then the full bench line (its bf16 / fp32 modes too) on the grown db (FAST mode).
#   bash tools/gpu/finddb.sh OUTDIR   -> OUTDIR/db/*.ufdb.txt, OUTDIR/bench.json
set -o pipefail
out=$(mkdir -p "${1:?usage: finddb.sh OUTDIR}/db" && cd "$1" && pwd) || exit 1
cd "$(dirname "$0")/../.." && export TMPDIR=/tmp
cp bm2f_amd/miopen_db/*.ufdb.txt "$out/db/"
( while sleep 45; do echo "[finddb] $(date +%T) db lines: $(cat "$out"/db/*.txt | wc -l)"; done ) &
HB=$!
trap 'kill $HB 2>/dev/null' EXIT
MIOPEN_FIND_MODE=NORMAL MIOPEN_USER_DB_PATH="$out/db" timeout -k 10 700 python -u bench.py --amp fp16 \
  --steps 1 --warmup 1 > "$out/db_fp16.log" 2>&1 && \
echo "[finddb] fp16 search done" && \
MIOPEN_USER_DB_PATH="$out/db" timeout -k 10 400 python -u bench.py --full --no-cpu-baseline \
  > "$out/bench.json" 2> "$out/bench.err"
