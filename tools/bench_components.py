#!/usr/bin/env python3
"""What the connected components of the compacted graph cost (dskgpu_components) next to the stages that build what they read, with the table
kernel in both forms.

Counts a workload (default c2_10Mx150, abundance_min = 2; "reads100k" = the 100 000 x 150 bp synthetic reads of the tests) at every --k
(default 31) in TWO contexts of one process: one whose component table is built by one add per unitig and column (DSKGPU_CC_PLAIN), one with
the wave-combined kernel the library ships.  Both mark the three steps of the build apart (DSKGPU_CC_STAGES: "component labelling" = set the
parents + hook + flatten, "component numbering" = scan + number, "component table" = the table kernel + its stats).  A repetition is, for
each context in turn (interleaved, so that both forms see the same clocks): dskgpu_filter_rows keeping every row -- which marks the index,
the compaction, the edges and the components stale -- and dskgpu_components, which builds them all again; the stage times the library
reports (DSKGPU_F_TIMING) are recorded as the difference of dskgpu_stage_times before and after, so the three steps stand next to "unitigs"
and "unitig edges" of the same repetition.  --reps repetitions after one warm-up; per stage the median, the minimum and every value.  Then
dskgpu_graph_small_components and dskgpu_drop_components (min_rows = 2 k) once, timed by device events.  The tool asserts that both forms
give the same table, that its columns add up to the unitigs, the rows and the edges, and that a second drop removes nothing, and exits
non-zero otherwise.  One JSON line on stdout, the same line appended to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("component labelling", "component numbering", "component table", "unitig edges", "unitigs", "graph", "query index")


def timed(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def summary(ms):
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), all=[round(x, 4) for x in ms])


def make_counter(k, args, stream, reads, plain):
    from dsk_amd import KmerCounter
    os.environ["DSKGPU_CC_STAGES"] = "1"                                      # (the switches are read once, when a context is created)
    if plain:
        os.environ["DSKGPU_CC_PLAIN"] = "1"
    try:
        kc = KmerCounter(kmer_size=k, abundance_min=args.abundance_min, stream=stream.cuda_stream, timing=True)
    finally:
        os.environ.pop("DSKGPU_CC_PLAIN", None)
        os.environ.pop("DSKGPU_CC_STAGES", None)
    kc.set_reads_device(reads.data_ptr(), reads.numel())
    kc.count()
    return kc


def bench_k(args, dev, reads, k):
    import torch
    stream = torch.cuda.Stream(dev)
    res = {"k": k, "min_rows": 2 * k}
    with torch.cuda.stream(stream):
        forms = {"plain": make_counter(k, args, stream, reads, True), "combined": make_counter(k, args, stream, reads, False)}
        try:
            n = forms["plain"].result_device()[2]
            keep = torch.ones(n, dtype=torch.uint8, device=dev)
            per = {name: {s: [] for s in STAGES} for name in forms}
            for rep in range(args.reps + 1):
                for name, kc in forms.items():
                    stream.synchronize()
                    kc.filter_rows_tensor(keep)
                    seen = dict(kc.stage_times())
                    st = kc.components()
                    now = dict(kc.stage_times())
                    if rep:                                                   # (rep 0: warm-up, first allocations)
                        for s in STAGES:
                            per[name][s].append(now.get(s, 0.0) - seen.get(s, 0.0))
            kc = forms["combined"]
            res["shape"] = dict(rows=n, unitigs=kc.unitigs()["n_unitigs"], edges=kc.unitig_edges()["n_edges"], **st)
            res["stage_ms"] = {name: {s: summary(v) for s, v in per[name].items()} for name in forms}
            tables = {name: [t.cpu() for t in c.components_table_tensor()] for name, c in forms.items()}
            ok = all(bool((a == b).all()) for a, b in zip(tables["plain"], tables["combined"])) and forms["plain"].components() == st
            _, unitigs, rows, _, edges = tables["combined"]
            ok = ok and int(unitigs.sum()) == res["shape"]["unitigs"] and int(rows.sum()) == n and int(edges.sum()) == res["shape"]["edges"]
            ok = ok and int(unitigs.max()) == st["max_unitigs"] and int(rows.max()) == st["max_rows"]
            res["small_components_ms"], small = timed(stream, lambda: kc.small_components(2 * k))
            res["drop_components_ms"], dropped = timed(stream, lambda: kc.drop_components(2 * k))
            again = kc.drop_components(2 * k)
            after = kc.components()
            ok = ok and small == dropped and again["n_small"] == 0 and again["n_rows_left"] == dropped["n_rows_left"] == kc.result_device()[2]
            ok = ok and after["n_components"] == st["n_components"] - dropped["n_small"]
            res.update(drop=dropped, after_drop=after, consistent=bool(ok))
            res["small_components_ms"], res["drop_components_ms"] = round(res["small_components_ms"], 3), round(res["drop_components_ms"], 3)
        finally:
            for kc in forms.values():
                kc.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c2_10Mx150", help="a workload of dsk_amd.synth, or reads100k")
    ap.add_argument("--k", default="31", help="comma-separated k")
    ap.add_argument("--abundance-min", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components.jsonl"), help="file the JSON line is appended to ('' = none)")
    args = ap.parse_args()
    if args.reps < 3:
        ap.error("--reps must be >= 3")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_components.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import synth
    dev = torch.device("cuda", 0)
    if args.workload == "reads100k":
        reads, nr, rl = synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150), 100_000, 150
    else:
        reads, _, nr, rl = synth.make_workload(args.workload, dev)
    torch.cuda.synchronize()
    result = {"bench": "components", "workload": args.workload, "device": torch.cuda.get_device_name(0), "reads": nr, "read_len": rl,
              "abundance_min": args.abundance_min, "results": [bench_k(args, dev, reads, int(k)) for k in args.k.split(",") if k]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if not all(r["consistent"] for r in result["results"]):
        sys.exit("bench_components.py: the two forms of the table, its sums or the drop do not agree")


if __name__ == "__main__":
    main()
