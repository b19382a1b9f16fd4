# round-3 measurement, part B: the other bench lines, DCNv3 kernel bench + counter passes, the north-star backbone figure
export OUT=${1:?usage: bash tools/round3_measure_b.sh <output directory>}
mkdir -p $OUT/r3
python bench.py --full --amp bf16x3 --no-cpu-baseline > $OUT/r3/bench_amp_bf16x3.json 2> $OUT/r3/bench_b.err
python bench.py --full --amp bf16 --no-cpu-baseline > $OUT/r3/bench_amp_bf16.json 2>> $OUT/r3/bench_b.err
python bench.py --full --model somi --no-cpu-baseline > $OUT/r3/bench_somi.json 2>> $OUT/r3/bench_b.err
python bench.py --full --mode infer --batch 128 > $OUT/r3/bench_infer128.json 2>> $OUT/r3/bench_b.err
python bench.py --full --size 1280 --batch 8 --nc 3 --no-cpu-baseline > $OUT/r3/bench_uavdt1280_b8.json 2>> $OUT/r3/bench_b.err
python bench.py --full --model yolov5s --batch 2 > $OUT/r3/bench_yolov5s_b2.json 2>> $OUT/r3/bench_b.err
for f in bench_amp_bf16x3 bench_amp_bf16 bench_somi bench_infer128 bench_uavdt1280_b8 bench_yolov5s_b2; do python -c "import json;d=json.load(open('$OUT/r3/$f.json'));print('$f',d['value'],d['ms_per_step'],d['roofline']['frac'],d['roofline']['all_conv_tflops'],d.get('latency_ms_per_image'))"; done
python tools/kernel_bench.py dcn backbone > $OUT/r3/kernel_bench.jsonl 2> $OUT/r3/kernel_bench.err; tail -n 2 $OUT/r3/kernel_bench.jsonl | cut -c1-300
bash tools/pmc_dcn.sh > $OUT/r3/pmc_dcn.log 2>&1; echo pmc done
