#!/usr/bin/env python3
"""Time of the compaction of the rows' de Bruijn graph into unitigs (dskgpu_unitigs / dskgpu_unitigs_stream).

Counts a workload (default c2_10Mx150, abundance_min = 2) at every --k (default 31, 63).  The compaction lives and dies with a result, so
every repetition is count -> query_prepare (the index is there before anything is timed) -> unitigs -> unitigs_stream; one warm-up
repetition, then the median of --reps.  The context runs with DSKGPU_UNITIG_STAGES set, so the build's device events split it into
  graph (the adjacency bytes, k_graph_rows) / unitig links / unitig ranking (all pointer-jumping rounds with their read-backs) /
  unitig numbering (first nodes, scan, numbers, offsets, abundance sums)
and "unitig stream" is the emission.  The yardstick is dskgpu_graph_adjacency on the same result (8 probes per row; the links need at most
2, the ranking a few random 8-byte accesses per node and round), timed the same way.  HBM held per row: what the device's free memory lost
between before and after the build (the build's scratch is freed when it returns) and the formula 8 + 17 * unitigs / rows.
The tool asserts the recount identity: the stream, counted at abundance_min = 1 by a second context, gives back exactly the rows, each
once -- and exits non-zero on a mismatch.  One JSON line on stdout.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["DSKGPU_UNITIG_STAGES"] = "1"          # read when a context is created

STAGES = [("adjacency", "graph"), ("links", "unitig links"), ("ranking", "unitig ranking"), ("numbering", "unitig numbering"), ("stream", "unitig stream")]


def timed(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def med(xs):
    return round(statistics.median(xs), 3)


def bench_k(args, dev, reads, k):
    import numpy as np
    import torch
    from dsk_amd import KmerCounter
    stream = torch.cuda.Stream(dev)
    res = {"k": k}
    with torch.cuda.stream(stream), KmerCounter(kmer_size=k, abundance_min=args.abundance_min, stream=stream.cuda_stream, timing=True) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        per_stage = {name: [] for name, _ in STAGES}
        build_ms, stream_ms, held = [], [], []
        text = None
        for rep in range(args.reps + 1):
            kc.count()
            kc.query_prepare()
            stream.synchronize()
            free0 = torch.cuda.mem_get_info(dev)[0]
            ms_b, st = timed(stream, kc.unitigs)
            free1 = torch.cuda.mem_get_info(dev)[0]
            if text is None:
                text = torch.zeros(st["stream_bytes"], dtype=torch.uint8, device=dev)
                stream.synchronize()
            ms_s, _ = timed(stream, lambda: kc.unitigs_stream(text.data_ptr(), text.numel()))
            times = dict(kc.stage_times())
            if rep == 0:
                continue                                                      # warm-up: first allocations
            build_ms.append(ms_b); stream_ms.append(ms_s); held.append(free0 - free1)
            for name, stage in STAGES:
                per_stage[name].append(times.get(stage, 0.0))
        rows = kc.result_device()[2]
        res.update(rows=rows, n_unitigs=st["n_unitigs"], n_cycles=st["n_cycles"], n_single=st["n_single"], max_nodes=st["max_nodes"],
                   n_rounds=st["n_rounds"], stream_bytes=st["stream_bytes"],
                   build_ms_median=med(build_ms), build_ms_all=[round(x, 3) for x in build_ms],
                   stream_call_ms_median=med(stream_ms), stream_call_ms_all=[round(x, 3) for x in stream_ms],
                   stage_ms_median={name: med(v) for name, v in per_stage.items()},
                   hbm_held_bytes_per_row_measured=round(statistics.median(held) / max(rows, 1), 2),
                   hbm_held_bytes_per_row_formula=round((8 * rows + 17 * st["n_unitigs"] + 8) / max(rows, 1), 2))

        # the yardstick: the adjacency call on the same result
        adj = torch.zeros(rows, dtype=torch.uint8, device=dev)
        stream.synchronize()
        kc.graph_adjacency(adj.data_ptr())
        gms = [timed(stream, lambda: kc.graph_adjacency(adj.data_ptr()))[0] for _ in range(args.reps)]
        res.update(graph_adjacency_ms_median=med(gms), graph_adjacency_ms_all=[round(x, 3) for x in gms],
                   build_over_graph_adjacency=round(statistics.median(build_ms) / statistics.median(gms), 3))

        # the recount identity
        k1, a1 = kc.rows()
        with KmerCounter(kmer_size=k, abundance_min=1, stream=stream.cuda_stream) as again:
            again.set_reads_device(text.data_ptr(), text.numel())
            again.count()
            k2, a2 = again.rows()
            s2 = again.stats()
        same = bool(len(k2) == len(k1) and np.array_equal(k2, k1) and (a2 == 1).all() and s2["n_kmers"] == rows)      # (both in the global order)
        res["recount_identity"] = same
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c2_10Mx150")
    ap.add_argument("--k", default="31,63", help="comma-separated k")
    ap.add_argument("--abundance-min", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be >= 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_unitigs.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import synth
    dev = torch.device("cuda", 0)
    reads, gl, nr, rl = synth.make_workload(args.workload, dev)
    torch.cuda.synchronize()
    result = {"bench": "unitigs", "workload": args.workload, "device": torch.cuda.get_device_name(0), "reads": nr, "read_len": rl,
              "abundance_min": args.abundance_min, "results": [bench_k(args, dev, reads, int(k)) for k in args.k.split(",") if k]}
    print(json.dumps(result))
    if not all(r["recount_identity"] for r in result["results"]):
        sys.exit("bench_unitigs.py: the unitig stream did not count back to the rows")


if __name__ == "__main__":
    main()
