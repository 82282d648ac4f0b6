#!/usr/bin/env python3
"""What a round of bubble popping costs (dskgpu_graph_bubbles, dskgpu_filter_rows, dskgpu_pop_bubbles) next to what it rebuilds, and what
dskgpu_simplify costs as a whole.

Counts a workload (default c2_10Mx150, abundance_min = 2; "reads100k" = the 100 000 x 150 bp synthetic reads of the tests) at every --k
(default 31), clips its tips (dskgpu_clip_tips, max_nodes = k) and pops its bubbles round by round, max_nodes = 2 k, max_diff = 4: every
round is graph_bubbles (which builds the index, the compaction and the edges of the current rows when they are stale) -> filter_rows of the
rows that are on no popped unitig.  Per round the tool records the stage times the library reports (DSKGPU_F_TIMING: "bubbles", "filter
rows", and the rebuilds "query index", "graph", "unitigs", "unitig edges") as the difference of dskgpu_stage_times before and after, with
rows, unitigs and edges before -- so "bubbles" stands next to the rebuilds of the same result.  Then, on a fresh count each, --reps
repetitions of ONE dskgpu_graph_bubbles call on a graph that is already built (the rule alone), and of ONE dskgpu_simplify call (the whole
job: tips and bubbles in turn), the median of the device-event time around the call.  The tool asserts that clip_tips + the rounds and
pop_bubbles leave the same rows, that simplify's counts add up and that the stream of the cleaned graph holds rows + k * unitigs bytes,
and exits non-zero otherwise.  One JSON line on stdout, the same line appended to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("bubbles", "tips", "filter rows", "query index", "graph", "unitigs", "unitig edges")


def timed(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def stage_delta(kc, before):
    now = dict(kc.stage_times())
    return now, {n: round(now.get(n, 0.0) - before.get(n, 0.0), 3) for n in STAGES}


def shape(kc):
    return dict(rows=kc.result_device()[2], unitigs=kc.unitigs()["n_unitigs"], edges=kc.unitig_edges()["n_edges"])


def median_of(ms):
    return round(statistics.median(ms), 3), [round(x, 3) for x in ms]


def bench_k(args, dev, reads, k):
    import torch
    from dsk_amd import KmerCounter
    stream = torch.cuda.Stream(dev)
    res = {"k": k, "tip_max_nodes": k, "bubble_max_nodes": 2 * k, "max_diff": 4}
    with torch.cuda.stream(stream), KmerCounter(kmer_size=k, abundance_min=args.abundance_min, stream=stream.cuda_stream, timing=True) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.count()
        n0 = kc.result_device()[2]
        res["clip_tips"] = kc.clip_tips(k)
        rounds = []
        while True:
            seen = dict(kc.stage_times())
            before = shape(kc)                                                # builds whatever is stale: its time is this round's rebuild
            row_pop, _, st = kc.graph_bubbles_tensor(2 * k, 4)
            if st["n_popped"]:
                kc.filter_rows_tensor(row_pop == 0)
            seen, ms = stage_delta(kc, seen)
            rounds.append(dict(before=before, stats=st, stage_ms=ms))
            if st["n_popped"] == 0 or len(rounds) == 64:
                break
        after = shape(kc)
        res.update(rounds=rounds, after_tips_and_bubbles=after)
        rows_by_rounds = kc.rows()[0]

        kc.count()
        kc.clip_tips(k)
        totals = kc.pop_bubbles(2 * k, 4)
        rows_by_pop = kc.rows()[0]
        ok = rows_by_pop.shape == rows_by_rounds.shape and bool((rows_by_pop == rows_by_rounds).all())
        ok = ok and totals["n_rows_left"] == after["rows"] and shape(kc) == after
        res["pop_bubbles"] = totals

        kc.count()
        kc.clip_tips(k)
        kc.unitig_edges()                                                     # the graph is built: what follows is the rule alone
        round_ms = []
        for rep in range(args.reps + 1):
            stream.synchronize()
            ms, _ = timed(stream, lambda: kc.graph_bubbles(2 * k, 4))
            if rep:
                round_ms.append(ms)                                           # (rep 0: warm-up, first allocations)
        res["graph_bubbles_ms_median"], res["graph_bubbles_ms_all"] = median_of(round_ms)

        simplify_ms, seen = [], None
        for rep in range(args.reps + 1):
            kc.count()
            stream.synchronize()
            seen = dict(kc.stage_times())
            ms, totals = timed(stream, kc.simplify)
            if rep:
                simplify_ms.append(ms)
        res["simplify_stage_ms"] = stage_delta(kc, seen)[1]                   # (of the last repetition)
        left = shape(kc)
        ok = ok and totals["n_rows_left"] == left["rows"] == n0 - totals["tips"]["n_rows_clipped"] - totals["bubbles"]["n_rows_popped"]
        ok = ok and kc.unitigs()["stream_bytes"] == left["rows"] + k * left["unitigs"]
        ok = ok and kc.graph_bubbles(2 * k, 4)["n_popped"] == 0 and kc.graph_tips(k)["n_tips"] == 0
        res.update(simplify=totals, after_simplify=left, consistent=bool(ok))
        res["simplify_ms_median"], res["simplify_ms_all"] = median_of(simplify_ms)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c2_10Mx150", help="a workload of dsk_amd.synth, or reads100k")
    ap.add_argument("--k", default="31", help="comma-separated k")
    ap.add_argument("--abundance-min", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bubbles.jsonl"), help="file the JSON line is appended to ('' = none)")
    args = ap.parse_args()
    if args.reps < 3:
        ap.error("--reps must be >= 3")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_bubbles.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import synth
    dev = torch.device("cuda", 0)
    if args.workload == "reads100k":
        reads, nr, rl = synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150), 100_000, 150
    else:
        reads, _, nr, rl = synth.make_workload(args.workload, dev)
    torch.cuda.synchronize()
    result = {"bench": "bubbles", "workload": args.workload, "device": torch.cuda.get_device_name(0), "reads": nr, "read_len": rl,
              "abundance_min": args.abundance_min, "results": [bench_k(args, dev, reads, int(k)) for k in args.k.split(",") if k]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if not all(r["consistent"] for r in result["results"]):
        sys.exit("bench_bubbles.py: the rounds, dskgpu_pop_bubbles and dskgpu_simplify do not agree")


if __name__ == "__main__":
    main()
