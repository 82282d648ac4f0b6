#!/usr/bin/env python3
"""What a round of tip clipping costs (dskgpu_graph_tips, dskgpu_filter_rows, dskgpu_clip_tips) next to what it rebuilds.

Counts a workload (default c2_10Mx150, abundance_min = 2; "reads100k" = the 100 000 x 150 bp synthetic reads of the tests) at every --k
(default 31) and clips its tips round by round, max_nodes = k: every round is graph_tips (which builds the index, the compaction and the
edges of the current rows when they are stale) -> filter_rows of the rows that are on no tip.  Per round the tool records the stage times
the library reports (DSKGPU_F_TIMING: "tips", "filter rows", and the rebuilds "query index", "graph", "unitigs", "unitig edges") as the
difference of dskgpu_stage_times before and after, with rows, unitigs and edges before and after -- so "tips" and "filter rows" stand next
to the "unitig edges" stage on the same result.  Then the same job as ONE dskgpu_clip_tips call on a fresh count: --reps repetitions, the
median of the device-event time around the call.  The tool asserts that both ways leave the same rows and that the stream of the cleaned
graph holds rows + k * unitigs bytes, and exits non-zero otherwise.  One JSON line on stdout, the same line appended to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("tips", "filter rows", "query index", "graph", "unitigs", "unitig edges")


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


def bench_k(args, dev, reads, k):
    import torch
    from dsk_amd import KmerCounter
    stream = torch.cuda.Stream(dev)
    res = {"k": k, "max_nodes": k}
    with torch.cuda.stream(stream), KmerCounter(kmer_size=k, abundance_min=args.abundance_min, stream=stream.cuda_stream, timing=True) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.count()
        rounds = []
        while True:
            seen = dict(kc.stage_times())
            before = shape(kc)                                                # builds whatever is stale: its time is this round's rebuild
            row_tip, _, st = kc.graph_tips_tensor(k)
            if st["n_tips"]:
                kc.filter_rows_tensor(row_tip == 0)
            seen, ms = stage_delta(kc, seen)
            rounds.append(dict(before=before, stats=st, stage_ms=ms))
            if st["n_tips"] == 0 or len(rounds) == 64:
                break
        seen = dict(kc.stage_times())
        after = shape(kc)
        res.update(rounds=rounds, after=after, last_rebuild_stage_ms=stage_delta(kc, seen)[1])
        text_bytes = kc.unitigs()["stream_bytes"]
        ok = text_bytes == after["rows"] + k * after["unitigs"]
        rows_by_rounds = kc.rows()[0]

        clip_ms, totals = [], None
        for rep in range(args.reps + 1):
            kc.count()
            stream.synchronize()
            ms, totals = timed(stream, lambda: kc.clip_tips(k))
            if rep:
                clip_ms.append(ms)                                            # (rep 0: warm-up, first allocations)
        rows_by_clip = kc.rows()[0]
        ok = ok and rows_by_clip.shape == rows_by_rounds.shape and bool((rows_by_clip == rows_by_rounds).all())
        ok = ok and totals["n_rows_left"] == after["rows"] and shape(kc) == after
        res.update(clip_tips=totals, clip_tips_ms_median=round(statistics.median(clip_ms), 3), clip_tips_ms_all=[round(x, 3) for x in clip_ms], consistent=bool(ok))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c2_10Mx150", help="a workload of dsk_amd.synth, or reads100k")
    ap.add_argument("--k", default="31", help="comma-separated k")
    ap.add_argument("--abundance-min", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tip_clipping.jsonl"), help="file the JSON line is appended to ('' = none)")
    args = ap.parse_args()
    if args.reps < 3:
        ap.error("--reps must be >= 3")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_tips.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import synth
    dev = torch.device("cuda", 0)
    if args.workload == "reads100k":
        reads, nr, rl = synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150), 100_000, 150
    else:
        reads, _, nr, rl = synth.make_workload(args.workload, dev)
    torch.cuda.synchronize()
    result = {"bench": "tip_clipping", "workload": args.workload, "device": torch.cuda.get_device_name(0), "reads": nr, "read_len": rl,
              "abundance_min": args.abundance_min, "results": [bench_k(args, dev, reads, int(k)) for k in args.k.split(",") if k]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if not all(r["consistent"] for r in result["results"]):
        sys.exit("bench_tips.py: the rounds and dskgpu_clip_tips do not leave the same graph")


if __name__ == "__main__":
    main()
