#!/usr/bin/env python3
"""What a round of the erroneous-connection rule costs (dskgpu_graph_connections, dskgpu_filter_rows, dskgpu_remove_connections) next to a
round of the bubble rule and to what a round rebuilds, and what dskgpu_simplify_all costs next to dskgpu_simplify.

Counts a workload (default c2_10Mx150, abundance_min = 2; "reads100k" = the 100 000 x 150 bp synthetic reads of the tests) at every --k
(default 31), runs dskgpu_simplify (tips max_nodes = k, bubbles max_nodes = 2 k, max_diff = 4) and removes the erroneous connections of what
is left round by round, max_nodes = 2 k, min_ratio = 4: every round is graph_connections (which builds the index, the compaction and the
edges of the current rows when they are stale) -> filter_rows of the rows that are on no removed unitig.  Per round the tool records the
stage times the library reports (DSKGPU_F_TIMING: "connections", "filter rows", and the rebuilds "query index", "graph", "unitigs", "unitig
edges") as the difference of dskgpu_stage_times before and after, with rows, unitigs and edges before.  Then, on a fresh count and
simplify, --reps repetitions, in turn, of ONE dskgpu_graph_connections and ONE dskgpu_graph_bubbles call on the same built graph (the two
rules alone, side by side), --reps repetitions of ONE dskgpu_remove_connections call, and, on a fresh count each and in turn, of ONE
dskgpu_simplify_all and ONE dskgpu_simplify call; the median of the device-event time around the call.  The tool asserts that the rounds
and remove_connections leave the same rows, that simplify_all's counts add up, that without connections it leaves the rows of simplify, and
that the stream of the cleaned graph holds rows + k * unitigs bytes, and exits non-zero otherwise.  One JSON line on stdout, the same line
appended to --out.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_bubbles import median_of, shape, timed      # noqa: E402

STAGES = ("connections", "bubbles", "tips", "filter rows", "query index", "graph", "unitigs", "unitig edges")


def stage_delta(kc, before):
    now = dict(kc.stage_times())
    return now, {n: round(now.get(n, 0.0) - before.get(n, 0.0), 3) for n in STAGES}


def bench_k(args, dev, reads, k):
    import torch
    from dsk_amd import KmerCounter
    stream = torch.cuda.Stream(dev)
    res = {"k": k, "tip_max_nodes": k, "bubble_max_nodes": 2 * k, "max_diff": 4, "connection_max_nodes": 2 * k, "min_ratio": 4}
    with torch.cuda.stream(stream), KmerCounter(kmer_size=k, abundance_min=args.abundance_min, stream=stream.cuda_stream, timing=True) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.count()
        n0 = kc.result_device()[2]
        res["simplify_before"] = kc.simplify()
        rounds = []
        while True:
            seen = dict(kc.stage_times())
            before = shape(kc)                                                # builds whatever is stale: its time is this round's rebuild
            row_rem, _, st = kc.graph_connections_tensor(2 * k, 4)
            if st["n_removed"]:
                kc.filter_rows_tensor(row_rem == 0)
            seen, ms = stage_delta(kc, seen)
            rounds.append(dict(before=before, stats=st, stage_ms=ms))
            if st["n_removed"] == 0 or len(rounds) == 64:
                break
        after = shape(kc)
        res.update(rounds=rounds, after_connections=after)
        rows_by_rounds = kc.rows()[0]

        remove_ms, seen = [], None
        for rep in range(args.reps + 1):
            kc.count()
            kc.simplify()
            stream.synchronize()
            seen = dict(kc.stage_times())
            ms, totals = timed(stream, lambda: kc.remove_connections(2 * k, 4))
            if rep:
                remove_ms.append(ms)                                          # (rep 0: warm-up, first allocations)
        res["remove_connections_stage_ms"] = stage_delta(kc, seen)[1]         # (of the last repetition)
        rows_by_remove = kc.rows()[0]
        ok = rows_by_remove.shape == rows_by_rounds.shape and bool((rows_by_remove == rows_by_rounds).all())
        ok = ok and totals["n_rows_left"] == after["rows"] and shape(kc) == after
        res["remove_connections"] = totals
        res["remove_connections_ms_median"], res["remove_connections_ms_all"] = median_of(remove_ms)

        kc.count()
        kc.simplify()
        kc.unitig_edges()                                                     # the graph is built: what follows are the two rules alone, in turn
        conn_ms, bubble_ms = [], []
        for rep in range(args.reps + 1):
            stream.synchronize()
            c, _ = timed(stream, lambda: kc.graph_connections(2 * k, 4))
            b, _ = timed(stream, lambda: kc.graph_bubbles(2 * k, 4))
            if rep:
                conn_ms.append(c); bubble_ms.append(b)
        res["graph_connections_ms_median"], res["graph_connections_ms_all"] = median_of(conn_ms)
        res["graph_bubbles_ms_median"], res["graph_bubbles_ms_all"] = median_of(bubble_ms)

        all_ms, simplify_ms = [], []
        for rep in range(args.reps + 1):
            kc.count()
            stream.synchronize()
            s, plain = timed(stream, kc.simplify)
            rows_plain, left_plain = kc.rows()[0], shape(kc)
            kc.count()
            stream.synchronize()
            _, without = timed(stream, lambda: kc.simplify_all(connections=False))
            ok = ok and {n: without[n] for n in plain} == plain and bool((kc.rows()[0] == rows_plain).all()) and shape(kc) == left_plain
            kc.count()
            stream.synchronize()
            seen = dict(kc.stage_times())
            a, totals = timed(stream, kc.simplify_all)
            if rep:
                all_ms.append(a); simplify_ms.append(s)
        res["simplify_all_stage_ms"] = stage_delta(kc, seen)[1]               # (of the last repetition)
        left = shape(kc)
        removed = totals["tips"]["n_rows_clipped"] + totals["bubbles"]["n_rows_popped"] + totals["connections"]["n_rows_removed"]
        ok = ok and totals["n_rows_left"] == left["rows"] == n0 - removed
        ok = ok and kc.unitigs()["stream_bytes"] == left["rows"] + k * left["unitigs"]
        ok = ok and kc.graph_connections(2 * k, 4)["n_removed"] == 0 and kc.graph_bubbles(2 * k, 4)["n_popped"] == 0 and kc.graph_tips(k)["n_tips"] == 0
        res.update(simplify=plain, after_simplify=left_plain, simplify_all=totals, after_simplify_all=left, consistent=bool(ok))
        res["simplify_all_ms_median"], res["simplify_all_ms_all"] = median_of(all_ms)
        res["simplify_ms_median"], res["simplify_ms_all"] = median_of(simplify_ms)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c2_10Mx150", help="a workload of dsk_amd.synth, or reads100k")
    ap.add_argument("--k", default="31", help="comma-separated k")
    ap.add_argument("--abundance-min", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "connections.jsonl"), help="file the JSON line is appended to ('' = none)")
    args = ap.parse_args()
    if args.reps < 3:
        ap.error("--reps must be >= 3")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_connections.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import synth
    dev = torch.device("cuda", 0)
    if args.workload == "reads100k":
        reads, nr, rl = synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150), 100_000, 150
    else:
        reads, _, nr, rl = synth.make_workload(args.workload, dev)
    torch.cuda.synchronize()
    result = {"bench": "connections", "workload": args.workload, "device": torch.cuda.get_device_name(0), "reads": nr, "read_len": rl,
              "abundance_min": args.abundance_min, "results": [bench_k(args, dev, reads, int(k)) for k in args.k.split(",") if k]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if not all(r["consistent"] for r in result["results"]):
        sys.exit("bench_connections.py: the rounds, dskgpu_remove_connections, dskgpu_simplify and dskgpu_simplify_all do not agree")


if __name__ == "__main__":
    main()
