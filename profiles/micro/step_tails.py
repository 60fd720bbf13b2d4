"""per steady pipelined step of a rocprofv3 --kernel-trace CSV: when the level-1 FPS, stage S and stage G end, and how long every kernel
of the step's second phase ran, as medians over the steps: python step_tails.py <kernel_trace.csv> [steps to skip at either end]"""
import csv, statistics, sys
rows = list(csv.DictReader(open(sys.argv[1])))
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 3
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
name = lambda r: r["Kernel_Name"].replace("epnet::", "").replace("void ", "").split("(")[0]
anchors = [i for i, r in enumerate(rows) if "fps_indexed_kernel<8, 32" in r["Kernel_Name"]]
steps = []
for a, b in zip(anchors[skip:-skip - 1], anchors[skip + 1:-skip]):
    t0, t1 = int(rows[a]["Start_Timestamp"]), int(rows[b]["Start_Timestamp"])
    fps_end = int(rows[a]["End_Timestamp"])
    s_queue = rows[a]["Queue_Id"]
    inside = [r for r in rows[a:b] if int(r["Start_Timestamp"]) < t1]
    s_end = max(int(r["End_Timestamp"]) for r in inside if r["Queue_Id"] == s_queue)
    g = [r for r in inside if r["Queue_Id"] != s_queue and "bq_index_kernel<1024" not in r["Kernel_Name"]]
    g_end = max(int(r["End_Timestamp"]) for r in g if int(r["Start_Timestamp"]) > fps_end - 500000)
    q1 = [r for r in g if "bq_query2_kernel<8" in r["Kernel_Name"]]
    d = {"step": t1 - t0, "fps L1": fps_end - t0, "S tail (fps end -> S end)": s_end - fps_end, "S end": s_end - t0, "G end": g_end - t0}
    if q1:
        d["L1 query start - fps end"] = int(q1[0]["Start_Timestamp"]) - fps_end
    for r in inside:
        if int(r["Start_Timestamp"]) >= fps_end - 300000 and "gather_rows" not in r["Kernel_Name"]:
            k = ("S " if r["Queue_Id"] == s_queue else "G ") + name(r)
            d[k] = d.get(k, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    steps.append(d)
print("%d steady steps" % len(steps))
for k in steps[0]:
    v = [s[k] / 1e6 for s in steps if k in s]
    print("%-58s median %7.3f  min %7.3f  max %7.3f ms" % (k[:58], statistics.median(v), min(v), max(v)))
