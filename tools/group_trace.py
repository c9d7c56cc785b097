#!/usr/bin/env python3
"""Where the launches of the group path sat before they started: a rocprofv3 kernel trace of a bench.py run set
against the library's own ISL_GROUP_TRACE lines (host clocks of every arrival, launch and poll).

    ISL_GROUP_TRACE=1 ISL_BENCH_TRACE=1 rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- \\
        python3 bench.py --gpus 1 --steps 20 --warmup 5 2> run.err
    python tools/group_trace.py DIR-or-kernel_trace.csv run.err --steps 20 --out profiles/NAME.json

Per dispatch of the timed region (search, gather, scatter, publish and exact kernels): start, end, Queue_Id, Stream_Id,
grid.  Two figures:
  launch_ms_lost_to_placement: over the search dispatches, the time between "some hardware queue had no search
      dispatch running" and the dispatch's own start, counted only while its launch was already submitted.  With
      F(t) = the time up to t during which fewer than Q queues ran a search dispatch, that is
      sum F(start of dispatch) - sum F(submission of launch): no pairing of launches and dispatches is needed.
  late launches: for every launch of several calls, what the host's polls saw of its members' markers on the
      caller's stream (pending or reached) and when, against the start of the gather kernels and the end of the
      kernel in front of each in its own queue."""
import argparse
import csv
import glob
import json
import os
import re
import sys

PRODUCT = re.compile(r"leann_search|group_gather|group_scatter|publish|classify|exact|zero_u32")


def short(name):
    m = re.search(r"(leann_search_\w+|group_gather_kernel|group_scatter_kernel|\w*publish\w*|\w*exact\w*|\w*classify\w*|zero_u32_kernel)", name)
    return m.group(1) if m else name[:40]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("stderr")
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--queues", type=int, default=4)
    ap.add_argument("--out", default="-")
    ap.add_argument("--note", default="")
    a = ap.parse_args()
    files = [a.trace] if os.path.isfile(a.trace) else glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    # ---- the library's lines: the timed region is the last --steps arrivals
    ev = []
    for line in open(a.stderr, errors="replace"):
        m = re.search(r"isl group-trace boot_ns=(\d+) mono_ns=(\d+) (\w+) (.*)", line)
        if m:
            kv = dict(p.split("=", 1) for p in m.group(4).split())
            ev.append({"boot": int(m.group(1)), "mono": int(m.group(2)), "what": m.group(3), **kv})
    arrivals = [i for i, e in enumerate(ev) if e["what"] == "arrive"]
    if len(arrivals) < a.steps:
        sys.exit(f"{len(arrivals)} arrivals in {a.stderr}, expected at least {a.steps}")
    ev = ev[arrivals[-a.steps]:]
    launches = [e for e in ev if e["what"] == "launch"]
    # ---- the dispatches: product kernels from the first timed arrival on (whichever host clock the trace is on)
    prod = [r for r in rows if PRODUCT.search(r["Kernel_Name"])]
    for r in prod:
        r["_s"], r["_e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        r["_grid"] = int(r["Grid_Size_X"]) * max(1, int(r["Grid_Size_Y"])) * max(1, int(r["Grid_Size_Z"]))
        r["_wg"] = int(r["Workgroup_Size_X"]) * max(1, int(r["Workgroup_Size_Y"])) * max(1, int(r["Workgroup_Size_Z"]))
    last_end = max(r["_e"] for r in prod)
    clock = min(("boot", "mono"), key=lambda c: abs(last_end - ev[-1][c]))
    t0 = ev[0][clock]
    inside = sorted((r for r in prod if r["_s"] >= t0), key=lambda r: r["_s"])
    ms = lambda t: round((t - t0) / 1e6, 3)
    # (one traversal dispatch per launch; the heap-exact and publish kernels behind it are short and follow it)
    search = [r for r in inside if "leann_search_fast" in r["Kernel_Name"] and r["_grid"] > r["_wg"]]
    if len(search) != len(launches):
        sys.exit(f"{len(search)} traversal dispatches against {len(launches)} launches")
    # ---- F(t): time up to t with fewer than Q queues running a search dispatch
    edges = sorted([(r["_s"], 1, r["Queue_Id"]) for r in search] + [(r["_e"], -1, r["Queue_Id"]) for r in search])

    def idle_time(until):
        busy, t, total = {}, t0, 0
        for when, step, q in edges:
            if when > until:
                break
            if sum(1 for v in busy.values() if v > 0) < a.queues:
                total += when - t
            t = when
            busy[q] = busy.get(q, 0) + step
        if sum(1 for v in busy.values() if v > 0) < a.queues:
            total += until - t
        return total

    lost = sum(idle_time(r["_s"]) for r in search) - sum(idle_time(e[clock]) for e in launches)
    # ---- the launches of several calls: the markers as the polls saw them
    late = []
    for L in launches:
        polls = [e for e in ev if e["what"] == "poll" and e["launch"] == L["id"]]
        pend = [e for e in polls if int(e["markers_pending"]) > 0]
        clear = [e for e in polls if int(e["markers_pending"]) == 0]
        late.append({"launch": int(L["id"]), "lanes": L["lanes"], "queries": int(L["queries"]), "workspace": int(L["workspace"]),
                     "submitted_ms": ms(L[clock]), "markers": int(L["markers"]),
                     "markers_last_seen_pending_ms": ms(pend[-1][clock]) if pend else None,
                     "markers_first_seen_reached_ms": ms(clear[0][clock]) if clear else None,
                     "polls": len(polls)})
    by_queue = {}
    disp = []
    for r in inside:
        prev = by_queue.get(r["Queue_Id"])
        disp.append({"kernel": short(r["Kernel_Name"]), "start_ms": ms(r["_s"]), "end_ms": ms(r["_e"]), "queue": r["Queue_Id"],
                     "stream": r.get("Stream_Id"), "grid": [int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"])],
                     "previous_in_queue_ended_ms": ms(prev) if prev else None})
        by_queue[r["Queue_Id"]] = max(prev or 0, r["_e"])
    out = {"what": "kernel trace of the timed region against the library's ISL_GROUP_TRACE lines; times in ms after the "
                   "first timed call's arrival (host clock: %s)" % clock,
           "note": a.note,
           "timed_region_span_ms": ms(max(r["_e"] for r in inside)),
           "launch_ms_lost_to_placement": round(lost / 1e6, 3),
           "queues_used_by_search_dispatches": sorted({r["Queue_Id"] for r in search}),
           "streams_used_by_search_dispatches": sorted({r.get("Stream_Id") for r in search}),
           "launches": late, "dispatches": disp}
    text = json.dumps(out, indent=1)
    if a.out == "-":
        print(text)
    else:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
        print(f"{len(inside)} dispatches, {len(launches)} launches, lost {lost / 1e6:.3f} launch-ms -> {a.out}")


if __name__ == "__main__":
    main()
