# round-4 measurement, part A (run through gpurun from the repo root): the default bench line (with its configs[4] leg), kernel-trace stats +
# HBM-traffic + MFMA-busy / clock passes of the training bench, the inference profile, DCNv3 backward A/B (coloured vs slab form)
export OUT=${1:?usage: bash tools/round4_measure_a.sh <output directory>}
mkdir -p $OUT/r4
python bench.py --full > $OUT/r4/bench_line.json 2> $OUT/r4/bench.err
python - <<'PY'
import json, os
d = json.load(open(os.environ['OUT'] + '/r4/bench_line.json'))
print('default', d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['all_conv_tflops'], d.get('configs4'), d['roofline_dcnv3']['kernels'])
PY
python tools/dcn_bwd_probe.py > $OUT/r4/dcn_bwd_probe.jsonl 2>&1; SOMI_DCN_SLAB=1 python tools/dcn_bwd_probe.py >> $OUT/r4/dcn_bwd_probe.jsonl 2>&1; cat $OUT/r4/dcn_bwd_probe.jsonl
bash tools/profile_round.sh $OUT/prof_r04 > $OUT/r4/profile_round.log 2>&1; tail -n 1 $OUT/r4/profile_round.log
