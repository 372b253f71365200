# Round profile, part 1 (on an MI355X): tests, the full bench line, rocprofv3 kernel stats of the same command, HBM traffic counters
# (FETCH_SIZE / WRITE_SIZE in separate --pmc passes, MI355X_MICROARCH.md) at the bench's default step count, f32 and bf16 configurations.
#   tools/run_round_profile.sh [round tag, default r03] [output directory, default profile_out]
set -e
cd "$(dirname "$0")/.."
export TMPDIR=${TMPDIR:-/tmp}
R=${1:-r03}
OUT=${2:-profile_out}
mkdir -p "$OUT"
python -m pytest tests -m gpu -x -q > "$OUT/${R}_pytest_gpu.txt" 2>&1; tail -3 "$OUT/${R}_pytest_gpu.txt"
python bench.py --full > "$OUT/${R}_bench.json" 2> "$OUT/${R}_bench.err"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_stats" -- python3 bench.py --full --no-cpu-baseline > "$OUT/${R}_bench_under_rocprof.json" 2> "$OUT/prof.err"
cp $(find "$OUT/prof_stats" -name "*kernel_stats.csv" | head -1) "$OUT/${R}_kernel_stats.csv"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_fetch" -- python3 bench.py --no-cpu-baseline --no-e2e > /dev/null 2> "$OUT/pmc1.err"
rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc_write" -- python3 bench.py --no-cpu-baseline --no-e2e > /dev/null 2> "$OUT/pmc2.err"
python bench.py --full --precision bf16 --no-cpu-baseline > "$OUT/${R}_bench_bf16_config.json" 2> "$OUT/bf16.err"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_stats_bf16" -- python3 bench.py --precision bf16 --no-cpu-baseline --no-e2e > /dev/null 2> "$OUT/prof_bf16.err"
cp $(find "$OUT/prof_stats_bf16" -name "*kernel_stats.csv" | head -1) "$OUT/${R}_bf16_kernel_stats.csv"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_fetch_bf16" -- python3 bench.py --precision bf16 --no-cpu-baseline --no-e2e > /dev/null 2> "$OUT/pmc3.err"
rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc_write_bf16" -- python3 bench.py --precision bf16 --no-cpu-baseline --no-e2e > /dev/null 2> "$OUT/pmc4.err"
python tools/pmc_traffic.py "$OUT/pmc_fetch" "$OUT/pmc_write" "$OUT/pmc_fetch_bf16" "$OUT/pmc_write_bf16" > "$OUT/${R}_pmc_traffic.json"
head -c 600 "$OUT/${R}_bench.json"
