#!/usr/bin/env python3
"""Time of the edges between the unitigs (dskgpu_unitig_edges) on a built compaction.

Counts a workload (default c2_10Mx150, abundance_min = 2) at every --k (default 31, 63).  The edges live and die with a result, so every
repetition is count -> query_prepare -> unitigs (the index and the compaction are there before the edges are timed) -> unitig_edges; one
warm-up repetition, then the median of --reps.  "edges" is a device-event pair on the context's stream around the synchronous first
dskgpu_unitig_edges call of the repetition: k_unitig_ends (one pass over the rows), k_unitig_edges (at most 8 probes per unitig), the scan
of the degrees and the fill of the targets.  Two yardsticks from the same process on the same result, timed the same way: the build's own
"unitig links" stage (DSKGPU_UNITIG_STAGES, which the tool sets; at most 2 probes per ROW) and the whole build of the compaction.
The tool asserts on the full workload that the edges are the successors of the last nodes -- the degree of every oriented unitig U is the
popcount of the out-nibble of graph_adjacency()[ends[U] >> 1] (low nibble for an even ends[U], high for an odd one) and they sum to
n_edges -- and exits non-zero on a mismatch.  One JSON line on stdout, the same line appended to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["DSKGPU_UNITIG_STAGES"] = "1"          # read when a context is created


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
    import torch
    from dsk_amd import KmerCounter
    stream = torch.cuda.Stream(dev)
    res = {"k": k}
    with torch.cuda.stream(stream), KmerCounter(kmer_size=k, abundance_min=args.abundance_min, stream=stream.cuda_stream, timing=True) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        edges_ms, build_ms, links_ms, edges_stage_ms, held = [], [], [], [], []
        for rep in range(args.reps + 1):
            kc.count()
            kc.query_prepare()
            stream.synchronize()
            ms_b, ust = timed(stream, kc.unitigs)
            links = dict(kc.stage_times()).get("unitig links", 0.0)
            free0 = torch.cuda.mem_get_info(dev)[0]
            ms_e, est = timed(stream, kc.unitig_edges)
            free1 = torch.cuda.mem_get_info(dev)[0]
            stage = dict(kc.stage_times()).get("unitig edges", 0.0)
            if rep == 0:
                continue                                                      # warm-up: first allocations
            edges_ms.append(ms_e); build_ms.append(ms_b); links_ms.append(links); edges_stage_ms.append(stage); held.append(free0 - free1)
        rows, nu = kc.result_device()[2], ust["n_unitigs"]
        off, targets, ends = kc.unitig_edges_tensor()
        deg = off[1:] - off[:-1]
        res.update(rows=rows, n_unitigs=nu, **est,
                   degree_histogram=torch.bincount(deg, minlength=5).tolist(),
                   edges_ms_median=med(edges_ms), edges_ms_all=[round(x, 3) for x in edges_ms],
                   edges_stage_ms_median=med(edges_stage_ms),
                   links_stage_ms_median=med(links_ms), links_stage_ms_all=[round(x, 3) for x in links_ms],
                   build_ms_median=med(build_ms), build_ms_all=[round(x, 3) for x in build_ms],
                   edges_over_links=round(statistics.median(edges_ms) / max(statistics.median(links_ms), 1e-9), 3),
                   edges_over_build=round(statistics.median(edges_ms) / statistics.median(build_ms), 3),
                   hbm_held_bytes_measured=int(statistics.median(held)), hbm_held_bytes_formula=12 * 2 * nu + 8 + 4 * est["n_edges"])

        # the identity: the edges of U are the successors of last(U) that are rows
        adj = kc.graph_adjacency_tensor()[0]
        a = adj[(ends >> 1).long()].to(torch.int64)
        nib = torch.where((ends & 1) == 1, a >> 4, a & 15)
        pop = torch.tensor([bin(x).count("1") for x in range(16)], dtype=torch.int64, device=dev)[nib]
        res["adjacency_identity"] = bool((pop == deg).all().item() and int(pop.sum().item()) == est["n_edges"] == targets.numel())
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c2_10Mx150")
    ap.add_argument("--k", default="31,63", help="comma-separated k")
    ap.add_argument("--abundance-min", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unitig_edges.jsonl"), help="file the JSON line is appended to ('' = none)")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be >= 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_unitig_edges.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import synth
    dev = torch.device("cuda", 0)
    reads, gl, nr, rl = synth.make_workload(args.workload, dev)
    torch.cuda.synchronize()
    result = {"bench": "unitig_edges", "workload": args.workload, "device": torch.cuda.get_device_name(0), "reads": nr, "read_len": rl,
              "abundance_min": args.abundance_min, "results": [bench_k(args, dev, reads, int(k)) for k in args.k.split(",") if k]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if not all(r["adjacency_identity"] for r in result["results"]):
        sys.exit("bench_unitig_edges.py: the edges are not the successors of the last nodes")


if __name__ == "__main__":
    main()
