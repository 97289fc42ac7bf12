#!/usr/bin/env python3
"""tools/replay_queue_wait.py <kernel_trace.csv>: what the valence replay (k_eb_valence, k_eb_ctx) and the main-stream kernels cost each
other where they share a hardware queue, from a `rocprofv3 --kernel-trace` run of bench.py (one JSON object on stdout; streams are told
apart as in tools/queue_budget.py).  A queue runs the kernels of its streams one after the other, so a kernel whose predecessors are done
may still stand behind another stream's kernel on its queue.  Reported:
  aux_streams                      per auxiliary stream: its queue id(s) and the main streams on the same queue id
  replay                           per replay kernel name: launches, mean / total run time, and the wait: from `ready` (the later of the end of the
                                   stream's previous kernel and the end of the group's k_valence_init, matched by dispatch order) to its start;
                                   wait_behind_main_ms = the part of that wait during which a main-stream kernel of the SAME queue id was running
  main_on_shared_queue             for the main streams on an auxiliary stream's queue: total wait of their kernels (from the end of the stream's
                                   previous kernel to the start) and the part of it during which a replay kernel of that queue was running
  traverse                         k_traverse_wave_f16: launches, mean, min, max in ms
With no auxiliary stream in the trace (the fused replay), `aux_streams` is empty and only `traverse` and the queue ids are of interest.
Diagnostic."""
import csv, json, re, sys, collections

rows = []
for r in csv.DictReader(open(sys.argv[1])):
    n = re.sub(r"<.*", "", re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", ""))
    rows.append(dict(s=int(r["Start_Timestamp"]), e=int(r["End_Timestamp"]), n=n, q=str(r["Queue_Id"]), st=str(r.get("Stream_Id", r["Queue_Id"])),
                     d=int(r.get("Dispatch_Id", 0) or 0)))
rows.sort(key=lambda k: (k["s"], k["d"]))
by_stream = collections.defaultdict(list)
for k in rows: by_stream[k["st"]].append(k)
names = {st: {k["n"] for k in ks} for st, ks in by_stream.items()}
main = sorted(st for st, ns in names.items() if "k_job_clear" in ns)
aux = sorted(st for st, ns in names.items() if "k_eb_valence" in ns and "k_job_clear" not in ns)
REPLAY = ("k_eb_valence", "k_eb_ctx")


def covered(lo, hi, spans):
    """length of [lo, hi] covered by the union of spans (sorted by start)"""
    tot, pos = 0, lo
    for s, e in spans:
        if e <= pos: continue
        if s >= hi: break
        a, b = max(s, pos), min(e, hi)
        if b > a: tot += b - a; pos = b
    return tot


ms = lambda ns: round(ns / 1e6, 2)
out = dict(aux_streams={}, replay={}, main_on_shared_queue={}, queue_ids_main={st: sorted({k["q"] for k in by_stream[st]}) for st in main})
inits = sorted((k for st in main for k in by_stream[st] if k["n"] == "k_valence_init"), key=lambda k: k["d"])
for a in aux:
    qs = sorted({k["q"] for k in by_stream[a]})
    mates = sorted(st for st in main if any(k["q"] in qs for k in by_stream[st]))
    out["aux_streams"][a] = dict(queue_ids=qs, main_streams_on_them=mates)
    main_spans = sorted((k["s"], k["e"]) for st in mates for k in by_stream[st] if k["q"] in qs)
    ks = sorted(by_stream[a], key=lambda k: k["d"])
    vals = [k for k in ks if k["n"] == "k_eb_valence"]
    ready_of = {v["d"]: inits[i]["e"] for i, v in enumerate(vals) if i < len(inits)} if len(vals) == len(inits) else {}
    acc = {n: dict(launches=0, run=0, wait=0, behind=0) for n in REPLAY}
    prev_end = None
    for k in ks:
        if k["n"] in acc:
            ready = max(prev_end or 0, ready_of.get(k["d"], 0)) or k["s"]
            w = max(0, k["s"] - ready)
            A = acc[k["n"]]; A["launches"] += 1; A["run"] += k["e"] - k["s"]; A["wait"] += w; A["behind"] += covered(ready, k["s"], main_spans) if w else 0
        prev_end = k["e"]
    for n, A in acc.items():
        R = out["replay"].setdefault(n, dict(launches=0, run_ms_total=0, wait_ms_total=0, wait_behind_main_ms=0))
        R["launches"] += A["launches"]; R["run_ms_total"] = round(R["run_ms_total"] + ms(A["run"]), 2)
        R["wait_ms_total"] = round(R["wait_ms_total"] + ms(A["wait"]), 2); R["wait_behind_main_ms"] = round(R["wait_behind_main_ms"] + ms(A["behind"]), 2)
    rep_spans = sorted((k["s"], k["e"]) for k in ks if k["n"] in REPLAY)
    for st in mates:
        wait = behind = run = 0; prev_end = None
        for k in by_stream[st]:
            if prev_end is not None and k["s"] > prev_end and k["n"] != "k_job_clear":      # (a group's first kernel waits for the host, not for the queue)
                wait += k["s"] - prev_end; behind += covered(prev_end, k["s"], rep_spans)
            run += k["e"] - k["s"]; prev_end = max(prev_end or 0, k["e"])
        out["main_on_shared_queue"][st] = dict(kernels_ms_total=ms(run), wait_ms_total=ms(wait), wait_behind_replay_ms=ms(behind))
for n, R in out["replay"].items(): R["run_ms_mean"] = round(R["run_ms_total"] / max(1, R["launches"]), 2)
tr = [k["e"] - k["s"] for k in rows if k["n"] == "k_traverse_wave_f16"]
out["traverse"] = dict(launches=len(tr), mean_ms=ms(sum(tr) / max(1, len(tr))), min_ms=ms(min(tr)) if tr else None, max_ms=ms(max(tr)) if tr else None)
print(json.dumps(out))
