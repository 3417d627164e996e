# The full bench line (bench.py --full at its default steps: the timed steps, then roofline_all, the AMP bf16 /
# fp32 modes, the achievable peaks, the op-level MSDA timing and the CPU baseline) -> OUTDIR/bench.json
#   bash tools/gpu/bench.sh OUTDIR
set -o pipefail
out=$(mkdir -p "${1:?usage: bench.sh OUTDIR}" && cd "$1" && pwd) || exit 1
cd "$(dirname "$0")/../.." && export TMPDIR=/tmp
timeout -k 10 800 python -u bench.py --full 2> "$out/bench.err" | tee "$out/bench.json"
