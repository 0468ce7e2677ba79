"""Per-level kernel times of the int8-emulated updates from a rocprofv3 kernel trace (CSV) of ONE batch on ONE stream
(`LMM_F64_EMUL_MINK=1024 rocprofv3 --kernel-trace -f csv -- python bench.py --full --steps 0 --no-cpu-baseline`).

    python tools/emul_level_times.py TRACE_kernel_trace.csv [--f64 NR NC]

A level is recognised by the K of the update's emul_convert_kernel launches (grid y = K / 128): the row-maximum kernels that open
an update scan only the columns no earlier update has scanned (emul_amax_fold_kernel, counted with emul_rowmax, starts them from the
kept maxima), so their grid does not tell.  Prints ms summed over the launches of a level, per kernel, and the totals of every other
kernel.  emul_live is the kernel in front of a convert that decides the live blocks and pieces of a group from the block maxima; a
trace from before it has zeros there, and the kernel it made unnecessary, emul_zero_fill (zero residues into the pieces the convert left
unwritten), has zeros in a trace with it.  `fill` is the stream's memsets inside an update: before emul_live, the masks and the
unwritten-piece bitmap of a group were one of them.  emul_screen marks the tiles whose update cannot change a bit of C and
emul_compact lists the GEMM's work ids of the others; a trace from before them has zeros there.

Then one line per emulated UPDATE, in launch order: an update is a maximal run of emulation kernels and the fills between them
(two emulated updates are never neighbours: the factorisation of the columns between them lies in between).  Its key is (K, Mp,
nb): Mp = the rows padded to the GEMM tile (convert's grid), nb = the matrices of all its groups.  `span` is first start to last end,
the leaf128_kernel launch that follows an emulated update included (the f64 update runs that leaf inside its own launch).

A screened f64 update ("the same screen on the f64 kernel") opens with the same scan kernels, then f64_screen_kernel
and its potrf_node_kernel launch: those are kept apart from the emulated updates and listed after them, one line per update in launch
order -- the node launch's template arguments, grid and ms, the scan's and the screen's ms, and the screen's grid (tile rows x tile
columns - 1 x matrices).

--f64 NR NC: the trace is of the f64 path (LMM_F64_EMUL=0) of matrices with NR rows and NC columns; the potrf_node_kernel<2>
launches (the updates with K >= 1024) are named by walking the factorisation's recursion, evaluation after evaluation."""
import collections
import csv
import sys

EMUL = ("emul_rowmax", "emul_live", "emul_convert", "emul_zero_fill", "emul_screen", "emul_compact", "emul_gemm", "emul_combine")
ALIAS = {"emul_amax_fold": "emul_rowmax"}


def grid(r, ax):
    return int(r["Grid_Size_" + ax]) // max(1, int(r["Workgroup_Size_" + ax]))


def split(w):
    return (w // 2 + 127) // 128 * 128 if w >= 256 else (128 if w == 192 else 64)


def updates(NR, j0, w, out):
    """(M, N, K) of the trailing updates with N >= 128 of the columns [j0, j0 + w), in launch order"""
    if w < 256:
        return
    h = split(w)
    updates(NR, j0, h, out)
    if w - h >= 128:
        out.append((NR - j0 - h, w - h, h))
    updates(NR, j0 + h, w - h, out)


def main(argv):
    path = argv[0]
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cv_rows = 64 if any("emul_live_kernel" in r["Kernel_Name"] for r in rows) else 16      # panel rows per workgroup of the convert
    per = collections.defaultdict(lambda: collections.defaultdict(float))
    other = collections.defaultdict(float)
    runs, cur, last_k = [], None, 0      # last_k: a run cut in two by another kernel continues the level of its first part
    screened, scr = [], None             # screened f64 updates: scan ms, screen ms and grid, then the node launch

    def close(u):
        for k in EMUL:
            per[k][u["K"]] += u[k]
        runs.append(u)
    for r in rows:
        name = r["Kernel_Name"]
        t0, t1 = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        ms = (t1 - t0) * 1e-6
        hit = next((ALIAS.get(k, k) for k in EMUL + tuple(ALIAS) if k + "_kernel" in name), None)
        if "f64_screen_kernel" in name:      # the run so far was this update's scan, not an emulated update
            scr = dict(scan=cur["emul_rowmax"] if cur is not None else 0.0, screen=ms, grid=f"{grid(r, 'X')} x {grid(r, 'Y')} x {grid(r, 'Z')}")
            cur = None
            continue
        if scr is not None and "potrf_node_kernel" in name:
            scr.update(node=ms, kind=name[name.index("<"):name.index(">") + 1] if "<" in name else "", items=grid(r, "X"))
            screened.append(scr)
            scr = None
        if hit is None:
            other[name.split("(")[0][:60]] += ms
            if cur is not None and "fillBuffer" in name:
                cur["fill"] += ms
                continue
            if cur is not None:
                if "leaf128_kernel" in name:
                    cur["leaf"] = ms
                    cur["t1"] = t1
                close(cur)
                cur = None
            continue
        if cur is None:
            cur = collections.defaultdict(float, t0=t0, K=last_k, nb=0, groups=0)
        if hit == "emul_convert":
            cur["K"] = last_k = 128 * grid(r, "Y")
            cur["Mp"] = cv_rows * grid(r, "X")
            cur["nb"] += grid(r, "Z")
            cur["groups"] += 1
        cur[hit] += ms
        cur["t1"] = t1
    if cur is not None:
        close(cur)
    levels = sorted({k for d in per.values() for k in d})
    for kern in EMUL:
        print(f"{kern}: " + str({k: round(per[kern][k], 2) for k in levels}))
    print("emulated total: " + str({k: round(sum(per[kern][k] for kern in per), 2) for k in levels}))
    print("other kernels ms: " + str({k: round(v, 2) for k, v in sorted(other.items(), key=lambda kv: -kv[1])[:10]}))
    if runs:
        print("emulated updates in launch order: K Mp nb groups | " + " ".join(k[5:] for k in EMUL) + " fill leaf | kernel sum, span (ms)")
    for u in runs:
        tot = sum(u[k] for k in EMUL) + u["fill"] + u["leaf"]
        print(f"  K={u['K']:5d} Mp={int(u['Mp']):5d} nb={u['nb']:2d} groups={u['groups']:2d} | " + " ".join(f"{u[k]:7.3f}" for k in EMUL)
              + f" {u['fill']:6.3f} {u['leaf']:6.3f} | {tot:8.3f} {(u['t1'] - u['t0']) * 1e-6:8.3f}")
    if screened:
        print(f"screened f64 updates in launch order ({len(screened)}): node kernel, items | node ms, scan ms, screen ms | screen grid")
        for u in screened:
            print(f"  {u['kind']:10s} {u['items']:7d} | {u['node']:8.3f} {u['scan']:7.3f} {u['screen']:7.3f} | {u['grid']}")
        print("screened f64 updates, totals: node %.2f ms, scan %.2f ms, screen %.2f ms" % tuple(sum(u[k] for u in screened) for k in ("node", "scan", "screen")))
    if "--f64" in argv:
        NR, NC = int(argv[argv.index("--f64") + 1]), int(argv[argv.index("--f64") + 2])
        seq = []
        updates(NR, 0, NC, seq)
        seq = [u for u in seq if u[2] >= 1024]
        node = [r for r in rows if "potrf_node_kernel<2" in r["Kernel_Name"]]
        print(f"f64 updates with K >= 1024 ({len(seq)} per evaluation), in launch order: evaluation M N K | grid | ms")
        for i, r in enumerate(node):
            M, N, Kk = seq[i % len(seq)]
            ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
            print(f"  eval={i // len(seq):2d} M={M:5d} N={N:5d} K={Kk:5d} | {grid(r, 'X')} x {grid(r, 'Y')} x {grid(r, 'Z')} | {ms:8.3f}")


if __name__ == "__main__":
    main(sys.argv[1:])
