"""Per-level kernel times of the int8-emulated updates from a rocprofv3 kernel trace (CSV) of ONE batch on ONE stream
(`LMM_F64_EMUL_MINK=1024 rocprofv3 --kernel-trace -f csv -- python bench.py --full --steps 0 --no-cpu-baseline`).

    python tools/emul_level_times.py TRACE_kernel_trace.csv

A level is recognised by the K of the emul_rowmax_kernel launch that opens every update (grid y = K / 64); the three kernels after
it belong to the same update.  Prints ms summed over the launches of a level, per kernel, and the totals of every other kernel."""
import collections
import csv
import sys


def main(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = collections.defaultdict(lambda: collections.defaultdict(float))
    other = collections.defaultdict(float)
    K = None
    for r in rows:
        name = r["Kernel_Name"]
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        hit = next((k for k in ("emul_rowmax", "emul_convert", "emul_gemm", "emul_combine") if k + "_kernel" in name), None)
        if hit is None:
            other[name.split("(")[0][:60]] += ms
            continue
        if hit == "emul_rowmax":
            K = 64 * int(r["Grid_Size_Y"]) // int(r["Workgroup_Size_Y"])
        per[hit][K] += ms
    levels = sorted({k for d in per.values() for k in d})
    for kern in ("emul_rowmax", "emul_convert", "emul_gemm", "emul_combine"):
        print(f"{kern}: " + str({k: round(per[kern][k], 2) for k in levels}))
    print("emulated total: " + str({k: round(sum(per[kern][k] for kern in per), 2) for k in levels}))
    print("other kernels ms: " + str({k: round(v, 2) for k, v in sorted(other.items(), key=lambda kv: -kv[1])[:10]}))


if __name__ == "__main__":
    main(sys.argv[1])
