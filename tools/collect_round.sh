# Runs ON THE GPU BOX: the round's evidence at HEAD -- full GPU suite, rocprofv3 stats + PMC passes of the default bench command
# (tools/collect_profiles.sh), the secondary bench lines.   bash tools/collect_round.sh OUTDIR
OUT=${1:?usage: bash tools/collect_round.sh OUTDIR}
mkdir -p $OUT; export TMPDIR=/tmp
timeout -k 10 900 python -m pytest tests -q -m gpu > $OUT/pytest_gpu.log 2>&1; tail -3 $OUT/pytest_gpu.log
bash tools/collect_profiles.sh final > $OUT/collect_final.log 2>&1
for w in c0 notebook c1; do python bench.py --full --workload $w --steps 300 --warmup 30 > $OUT/bench_$w.json 2> $OUT/bench_$w.err || exit 1; done
python bench.py --full --workload c1dense --steps 10 --warmup 2 > $OUT/bench_c1dense.json 2> $OUT/bench_c1dense.err
python bench.py --full --workload c3 --steps 5 --warmup 1 > $OUT/bench_c3.json 2> $OUT/bench_c3.err
python bench.py --full --workload c3 --proj bf16 --steps 5 --warmup 1 > $OUT/bench_c3_bf16proj.json 2> $OUT/bench_c3_bf16.err
python bench.py --full --steps 10 --warmup 2 > $OUT/bench_c2.json 2> $OUT/bench_c2.err
python bench.py --full --workload c4 --dtype f32 --steps 2 --warmup 1 > $OUT/bench_c4_f32.json 2> $OUT/bench_c4_f32.err
python - "$OUT" <<'PY'
import json,glob,sys
for f in sorted(glob.glob(sys.argv[1] + "/*.json")):
    try:
        d=json.load(open(f)); print(f.split("/")[-1], round(d["ms_per_step"],4), round(d["value"],4), (d.get("roofline") or {}).get("frac"), (d.get("cpu_baseline") or {}).get("value"), (d.get("share_of_8gpu_job") or {}).get("ms_per_eval"))
    except Exception as e: print(f, "ERR", e)
PY
