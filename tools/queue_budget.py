#!/usr/bin/env python3
"""tools/queue_budget.py <kernel_trace.csv>: how the streams of a `rocprofv3 --kernel-trace` run of bench.py share hardware queues (one JSON
object on stdout; tools/queue_timeline.py prints the timeline itself).  A geometry lane's main stream is one that launches k_job_clear, an
auxiliary stream one that launches k_eb_valence and no k_job_clear, a texture stream one that launches k_vq_stats.  A group is what a main
stream runs from a k_job_clear to the next k_gather.  Reported:
  queues_geometry / queues_texture   distinct queue ids of those streams, and which streams sit on each
  lanes_sharing_a_queue              main streams that share their queue id with another main stream
  overlaps_on_one_queue              pairs of kernels of two main streams on ONE queue id that overlap in time (a queue runs its streams one after the other: 0)
  groups                             of the last third of the trace, per main stream: span (first to last kernel) and kernel time in ms, idle share = 1 - kernel time / span,
                                     gap_before = from the last kernel of the lane's previous group to the first of this one.  The span starts at the group's
                                     first KERNEL, so a lane that waits for its queue before a group shows that in gap_before and in lanes_busy_mean, not in idle share
  lanes_busy_mean                    main-stream kernel time per wall time while any main stream runs a kernel, same part of the trace
Diagnostic."""
import csv, json, re, sys, collections

rows = []
for r in csv.DictReader(open(sys.argv[1])):
    n = re.sub(r"<.*", "", re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", ""))
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), n, str(r["Queue_Id"]), str(r.get("Stream_Id", r["Queue_Id"]))))
rows.sort()
by_stream = collections.defaultdict(list)
for s, e, n, q, st in rows: by_stream[st].append((s, e, n, q))
names = {st: {k[2] for k in ks} for st, ks in by_stream.items()}
main = sorted(st for st, ns in names.items() if "k_job_clear" in ns)
aux = sorted(st for st, ns in names.items() if "k_eb_valence" in ns and "k_job_clear" not in ns)
tex = sorted(st for st, ns in names.items() if "k_vq_stats" in ns)
queue_of = {st: sorted({k[3] for k in ks}) for st, ks in by_stream.items()}


def queues(sts):
    out = collections.defaultdict(list)
    for st in sts:
        for q in queue_of[st]: out[q].append(st)
    return dict(sorted(out.items()))


qm = queues(main)
sharing = sorted(st for q, sts in qm.items() if len(sts) > 1 for st in sts)
overlaps = 0
for q, sts in qm.items():
    ks = sorted((s, e, st) for st in sts for s, e, n, qq in by_stream[st] if qq == q)
    end, who = 0, None
    for s, e, st in ks:
        if who is not None and st != who and s < end: overlaps += 1
        if e > end: end, who = e, st
t_lo = rows[len(rows) * 2 // 3][0]
groups = collections.defaultdict(list)
for st in main:
    cur, prev_end = None, None
    for s, e, n, q in by_stream[st]:
        if n == "k_job_clear" and cur is None: cur = [s, e, 0]
        if cur is None: continue
        cur[1] = max(cur[1], e); cur[2] += e - s
        if n == "k_gather":
            if cur[0] >= t_lo: groups[st].append(dict(span_ms=round((cur[1] - cur[0]) / 1e6, 1), kernels_ms=round(cur[2] / 1e6, 1), idle_share=round(1 - cur[2] / max(1, cur[1] - cur[0]), 3),
                                                      gap_before_ms=None if prev_end is None else round((cur[0] - prev_end) / 1e6, 1)))
            prev_end = cur[1]; cur = None
allg = [g for gs in groups.values() for g in gs]
# main-stream kernel time per wall time during which ANY main stream runs a kernel (gaps > 20 ms - between the passes of the bench - left out)
ks = sorted((s, e) for st in main for s, e, n, q in by_stream[st] if s >= t_lo)
wall, end = 0, None
for s_, e_ in ks:
    if end is None or s_ > end + 20_000_000: wall += e_ - s_; end = e_
    elif e_ > end: wall += e_ - end; end = e_
lanes_busy = round(sum(e - s for s, e in ks) / max(1, wall), 2)
print(json.dumps(dict(
    streams=dict(geometry_main=len(main), geometry_aux=len(aux), texture=len(tex)),
    queues_geometry=queues(main + aux), queues_geometry_main=qm, queues_texture=queues(tex),
    n_queue_ids_geometry=len(queues(main + aux)), n_queue_ids_texture=len(queues(tex)), n_queue_ids_all=len({r[3] for r in rows}),
    lanes_sharing_a_queue=sharing, overlaps_on_one_queue=overlaps,
    groups={st: gs for st, gs in sorted(groups.items())},
    gap_before_ms_median=(sorted(g["gap_before_ms"] for g in allg if g["gap_before_ms"] is not None) or [None])[sum(1 for g in allg if g["gap_before_ms"] is not None) // 2],
    lanes_busy_mean=lanes_busy, idle_share_mean=round(sum(g["idle_share"] for g in allg) / max(1, len(allg)), 3),
    span_ms_mean=round(sum(g["span_ms"] for g in allg) / max(1, len(allg)), 1), kernels_ms_mean=round(sum(g["kernels_ms"] for g in allg) / max(1, len(allg)), 1))))
