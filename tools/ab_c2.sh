# Same-box A/B of the default bench (C2): the older tree in _ab_old/ against the working tree.   bash tools/ab_c2.sh OUTDIR
OUT=$(realpath -m "${1:?usage: bash tools/ab_c2.sh OUTDIR}"); mkdir -p "$OUT"
OLD_FULL=$(cd _ab_old && python bench.py --help | grep -m1 -o -- --full)    # a tree older than --full runs the roofline pass by default
for i in 1 2; do
  (cd _ab_old && python bench.py $OLD_FULL --steps 5 --warmup 2 --no-cpu-baseline > "$OUT/old_$i.json" 2>/dev/null)
  python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > "$OUT/new_$i.json" 2>/dev/null
  LMM_FUSE_BULK=0 python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > "$OUT/new_nofuse_$i.json" 2>/dev/null
done
python - "$OUT" <<'PY'
import json,glob,sys
for f in sorted(glob.glob(sys.argv[1] + "/*.json")):
    d=json.load(open(f)); print(f.split("/")[-1], round(d["ms_per_step"],2), d["roofline"]["frac"], d["roofline"]["avg_launch_ms"], d["share_of_8gpu_job"]["ms_per_eval"])
PY
