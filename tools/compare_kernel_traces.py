"""Compare the rocprofv3 --kernel-trace CSVs under two output directories: python tools/compare_kernel_traces.py DIR_A DIR_B
Equal means the same multiset of (kernel, grid, workgroup, LDS bytes) and, queue by queue, the same sequence of them.
--rename REGEX=REPL (repeatable, behind the directories): a kernel name of DIR_A is read as re.sub(REGEX, REPL, name), for kernels
that DIR_B's build renamed or merged.  --ignore REGEX: dispatches whose kernel name matches are counted and left out of both
comparisons (the HIP runtime's own copy kernels, __amd_rocclr_*: how it splits a copy from pageable host memory is not the library's doing)."""
import collections, csv, glob, re, sys

RENAMES = [tuple(sys.argv[i + 1].split("=", 1)) for i in range(3, len(sys.argv) - 1) if sys.argv[i] == "--rename"]
IGNORE = [sys.argv[i + 1] for i in range(3, len(sys.argv) - 1) if sys.argv[i] == "--ignore"]


def load(d):
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    assert len(f) == 1, f
    rows = list(csv.DictReader(open(f[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return rows, f[0]


def key(r):
    return (r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["Workgroup_Size_Y"],
            r["Workgroup_Size_Z"], r["LDS_Block_Size"])


a, fa = load(sys.argv[1]); b, fb = load(sys.argv[2])
for r in a:
    for rx, repl in RENAMES:
        r["Kernel_Name"] = re.sub(rx, repl, r["Kernel_Name"])
for rx in IGNORE:
    na, nb = len(a), len(b)
    a, b = [r for r in a if not re.search(rx, r["Kernel_Name"])], [r for r in b if not re.search(rx, r["Kernel_Name"])]
    print(f"ignored {rx}: {na - len(a)} dispatches of the parent, {nb - len(b)} of this build")
print("columns:", ", ".join(a[0].keys()))
ok = True
ca, cb = collections.Counter(map(key, a)), collections.Counter(map(key, b))
print(f"parent: {len(a)} dispatches, {len(ca)} distinct (kernel, grid, workgroup, LDS); this build: {len(b)} dispatches, {len(cb)} distinct")
if ca != cb:
    ok = False
    for k in sorted(set(ca) | set(cb)):
        if ca[k] != cb[k]:
            print("  MULTISET DIFFERS:", ca[k], cb[k], k[0][:90], k[1:])
else:
    print("multisets equal")
qcol = "Queue_Id" if "Queue_Id" in a[0] else None
if qcol:
    # queue ids are handles that differ between processes: name each queue by the order of its first dispatch
    def per_queue(rows):
        order, seqs = [], collections.defaultdict(list)
        for r in rows:
            q = r[qcol]
            if q not in order:
                order.append(q)
            seqs[order.index(q)].append(key(r))
        return seqs
    sa, sb = per_queue(a), per_queue(b)
    print("queues:", {q: len(v) for q, v in sa.items()}, "|", {q: len(v) for q, v in sb.items()})
    for q in sorted(set(sa) | set(sb)):
        if sa.get(q) != sb.get(q):
            ok = False
            la, lb = sa.get(q, []), sb.get(q, [])
            i = next((i for i, (u, v) in enumerate(zip(la, lb)) if u != v), min(len(la), len(lb)))
            print(f"  QUEUE {q} DIFFERS at dispatch {i} of {len(la)} / {len(lb)}:", la[i][0][:80] if i < len(la) else None, "|", lb[i][0][:80] if i < len(lb) else None)
    if ok:
        print("per-queue sequences equal")
else:
    print("the trace names no queue: per-stream sequences not compared")
print("RESULT:", "EQUAL" if ok else "DIFFERENT")
