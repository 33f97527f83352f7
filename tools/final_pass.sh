set -o pipefail
R=${1:-r03}
O=${FINAL_PASS_OUT:-out/final}
mkdir -p "$O"
bash tools/collect_profiles.sh yolo608_b32 ${R}_608b32 > "$O/cp_608.log" 2>&1 && echo cp608 ok &&
bash tools/collect_profiles.sh darknet19_448_b128_f16 ${R}_d19f16 > "$O/cp_d19.log" 2>&1 && echo cpd19 ok &&
bash tools/collect_profiles.sh yolo416_b8 ${R}_416b8 > "$O/cp_416.log" 2>&1 && echo cp416 ok &&
bash tools/collect_profiles.sh yolo9000_544_b8 ${R}_9k544b8 > "$O/cp_9k.log" 2>&1 && echo cp9k ok &&
python bench.py --full > "$O/bench_default.json" 2> "$O/bench_default.err" && echo bench ok &&
for w in darknet19_448_b128_f16 yolo416_b8 yolo9000_544_b8 tiny416_b1; do python bench.py --full --workload $w --cpu-iters 0 --latency-iters 0 > "$O/bench_$w.json" 2>/dev/null || exit 1; done
cat "$O/bench_default.json" | cut -c1-600
