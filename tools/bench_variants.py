#!/usr/bin/env python3
"""What variant reporting costs (dskgpu_variants, dskgpu_variants_table, dskgpu_variants_stream) next to what a user would run on the
device today for the same data: dskgpu_graph_bubbles plus dskgpu_unitigs_stream on the same built graph.

Counts a workload (default c2_10Mx150, abundance_min = 2; "reads100k" = the 100 000 x 150 bp synthetic reads of the tests) at every --k
(default 31), clips its tips (dskgpu_clip_tips, max_nodes = k) and builds the edges, so that nothing below pays for a rebuild.  Then --reps
repetitions (after one warm-up) of each of: ONE dskgpu_variants call (max_nodes = 2 k, max_diff = 4), the two copy calls into tensors that
exist, ONE dskgpu_graph_bubbles call and ONE dskgpu_unitigs_stream call; the median of the device-event time around the call, and for
dskgpu_variants the "variants" stage time the library reports (DSKGPU_F_TIMING), which leaves out the final read-back.  Reported with them:
n_variants by kind, the unitigs flagged and their fraction of all unitigs, the letters of the flagged unitigs next to the bytes of the
whole unitig stream.  The tool asserts that n_unitigs equals n_in_bubbles of dskgpu_graph_bubbles, that the kinds add up, that the stream
holds sum(L[a] + L[b]) + 2 n k bytes and that the rows did not change, and exits non-zero otherwise.  One JSON line on stdout, the same
line appended to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def median_of(ms):
    return round(statistics.median(ms), 3), [round(x, 3) for x in ms]


def repeat(args, stream, fn):
    ms = []
    for rep in range(args.reps + 1):
        stream.synchronize()
        t, _ = timed(stream, fn)
        if rep:
            ms.append(t)                                                      # (rep 0: warm-up, first allocations)
    return median_of(ms)


def bench_k(args, dev, reads, k):
    import torch
    from dsk_amd import KmerCounter
    stream = torch.cuda.Stream(dev)
    res = {"k": k, "tip_max_nodes": k, "max_nodes": 2 * k, "max_diff": 4}
    with torch.cuda.stream(stream), KmerCounter(kmer_size=k, abundance_min=args.abundance_min, stream=stream.cuda_stream, timing=True) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.count()
        res["clip_tips"] = kc.clip_tips(k)
        un, ed = kc.unitigs(), kc.unitig_edges()                              # the graph is built: what follows pays for no rebuild
        n_rows = kc.result_device()[2]
        res["graph"] = dict(rows=n_rows, unitigs=un["n_unitigs"], edges=ed["n_edges"], unitig_stream_bytes=un["stream_bytes"])

        stage = []
        def variants():
            before = dict(kc.stage_times()).get("variants", 0.0)
            st = kc.variants(2 * k, 4)
            stage.append(dict(kc.stage_times())["variants"] - before)
            return st
        res["variants_ms_median"], res["variants_ms_all"] = repeat(args, stream, variants)
        res["variants_stage_ms_median"], res["variants_stage_ms_all"] = median_of(stage[1:])
        st = kc.variants(2 * k, 4)
        res["variants"] = st

        n, nb = st["n_variants"], st["stream_bytes"]
        rec = torch.zeros((max(n, 1), 8), dtype=torch.int32, device=dev)
        off, text = torch.zeros(2 * n + 1, dtype=torch.int64, device=dev), torch.zeros(max(nb, 1), dtype=torch.uint8, device=dev)
        whole = torch.zeros(max(un["stream_bytes"], 1), dtype=torch.uint8, device=dev)
        stream.synchronize()
        res["variants_table_ms_median"], res["variants_table_ms_all"] = repeat(args, stream, lambda: kc.variants_table(rec.data_ptr()))
        res["variants_stream_ms_median"], res["variants_stream_ms_all"] = repeat(args, stream, lambda: kc.variants_stream(off.data_ptr(), text.data_ptr(), nb))
        res["graph_bubbles_ms_median"], res["graph_bubbles_ms_all"] = repeat(args, stream, lambda: kc.graph_bubbles(2 * k, 4))
        res["unitigs_stream_ms_median"], res["unitigs_stream_ms_all"] = repeat(args, stream, lambda: kc.unitigs_stream(whole.data_ptr(), un["stream_bytes"]))

        bub = kc.graph_bubbles(2 * k, 4)
        r = rec[:n].cpu().numpy().astype("int64")
        nodes = (kc.unitigs_table_tensor()[0].cpu().numpy()[1:] - kc.unitigs_table_tensor()[0].cpu().numpy()[:-1]) - k
        flagged = set((r[:, 0] >> 1).tolist()) | set((r[:, 1] >> 1).tolist())
        letters = int(sum(int(nodes[u]) + k - 1 for u in flagged))
        res["flagged"] = dict(unitigs=st["n_unitigs"], fraction_of_unitigs=round(st["n_unitigs"] / max(un["n_unitigs"], 1), 6), letters=letters,
                              fraction_of_unitig_stream=round(letters / max(un["stream_bytes"], 1), 6))
        ok = st["n_unitigs"] == bub["n_in_bubbles"] == len(flagged)
        ok = ok and st["n_snps"] + st["n_multi"] + st["n_indels"] + st["n_complex"] == n
        ok = ok and nb == int(off[-1]) == int(nodes[r[:, 0] >> 1].sum() + nodes[r[:, 1] >> 1].sum()) + 2 * n * k
        ok = ok and kc.result_device()[2] == n_rows and kc.unitigs() == un
        res["consistent"] = bool(ok)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c2_10Mx150", help="a workload of dsk_amd.synth, or reads100k")
    ap.add_argument("--k", default="31", help="comma-separated k")
    ap.add_argument("--abundance-min", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variants.jsonl"), help="file the JSON line is appended to ('' = none)")
    args = ap.parse_args()
    if args.reps < 3:
        ap.error("--reps must be >= 3")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_variants.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import synth
    dev = torch.device("cuda", 0)
    if args.workload == "reads100k":
        reads, nr, rl = synth.make_reads(synth.make_genome(300_000, dev), 100_000, 150), 100_000, 150
    else:
        reads, _, nr, rl = synth.make_workload(args.workload, dev)
    torch.cuda.synchronize()
    result = {"bench": "variants", "workload": args.workload, "device": torch.cuda.get_device_name(0), "reads": nr, "read_len": rl,
              "abundance_min": args.abundance_min, "results": [bench_k(args, dev, reads, int(k)) for k in args.k.split(",") if k]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if not all(r["consistent"] for r in result["results"]):
        sys.exit("bench_variants.py: dskgpu_variants, dskgpu_graph_bubbles and the unitig tables do not agree")


if __name__ == "__main__":
    main()
