# round-3 measurement, part A (run through gpurun from the repo root): kernel-trace stats + HBM-traffic passes of the training and inference bench
export OUT=${1:?usage: bash tools/round3_measure_a.sh <output directory>}
mkdir -p $OUT/r3
bash tools/profile_round.sh $OUT/prof_r03 > $OUT/r3/profile_round.log 2>&1; tail -n 1 $OUT/r3/profile_round.log
cp $OUT/prof_r03/traffic.json profiles/traffic.json
python bench.py --full > $OUT/r3/bench_line.json 2> $OUT/r3/bench.err
python - <<'PY'
import json, os
d = json.load(open(os.environ['OUT'] + '/r3/bench_line.json'))
print('default', d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['all_conv_tflops'], d['roofline']['traffic'], d['cpu_baseline']['value'], d['cpu_baseline']['iterations'])
PY
