#!/usr/bin/env python3
"""Rate of the rows' de Bruijn adjacency (dskgpu_graph_adjacency) against two baselines that are NOT the code under test.

Counts a workload (default c2_10Mx150, abundance_min = 2) at every --k (default 31, 63, 96), builds the lookup index, then times, with
device events on the stream the context runs on (one warm-up call, then the median of --reps calls, all values in the JSON line):
  * graph_adjacency: one byte per row + the 5 x 5 degree table; 8 probes per row;
  * (B) dskgpu_query_kmers on the SAME index with 8 * rows keys of the same hit fraction as the neighbour probes (set bits / (8 * rows),
    from the degree table): rows drawn at random for the hits, random values for the rest -- the probe rate the index gives without the
    neighbour arithmetic;
  * (A) k <= 31 only (the values stay below 2^63 in torch): what a caller had before -- the eight neighbour values built in torch from word 0 of dskgpu_result_device,
    canonicalised, eight dskgpu_query_kmers calls, the bits packed.  It must give the same byte at every row; the tool asserts that
    before it prints a time.  (No such baseline above k = 32: the rows' higher words are not on the device for a caller.)
One JSON line on stdout.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def summary(prefix, ms, work):
    med = statistics.median(ms)
    return {prefix + "_ms_median": round(med, 3), prefix + "_ms_all": [round(x, 3) for x in ms],
            prefix + "_per_s": round(work / (med * 1e-3), 1), prefix + "_spread": round((max(ms) - min(ms)) / med, 4)}


def rev_pairs(x):
    """reverse the 32 two-bit groups of every int64 bit pattern (the masks clear what the arithmetic shifts bring in)"""
    for sh, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        x = ((x >> sh) & m) | ((x & m) << sh)
    return ((x >> 32) & 0xFFFFFFFF) | (x << 32)


def caller_path(kc, x, k, out32, adj):
    """(A): adj <- the adjacency bytes of the one-word rows x (int64 tensor, k <= 31: the values and their neighbours stay below 2^63)"""
    import torch
    mask = (1 << (2 * k)) - 1
    rc = ((rev_pairs(x) >> (64 - 2 * k)) & mask) ^ (0x2AAAAAAAAAAAAAAA & mask)
    top = 2 * k - 2
    adj.zero_()
    for b in range(4):
        for j, f, r in ((b, ((x << 2) | b) & mask, (rc >> 2) | ((b ^ 2) << top)), (4 + b, (x >> 2) | (b << top), ((rc << 2) | (b ^ 2)) & mask)):
            q = torch.minimum(f, r)
            kc.query_kmers(q.data_ptr(), q.numel(), out32.data_ptr())
            adj |= (out32 != 0).to(adj.dtype) << j
    return adj


def bench_k(args, dev, reads, k):
    import torch
    from dsk_amd import KmerCounter
    stream = torch.cuda.Stream(dev)
    res = {"k": k}
    with torch.cuda.stream(stream), KmerCounter(kmer_size=k, abundance_min=args.abundance_min, stream=stream.cuda_stream, timing=True) as kc:
        kc.set_reads_device(reads.data_ptr(), reads.numel())
        kc.count()
        kp, _, rows = kc.result_device()
        ms_index, _ = timed(stream, kc.query_prepare)
        adj = torch.zeros(rows, dtype=torch.uint8, device=dev)
        stream.synchronize()
        deg = kc.graph_adjacency(adj.data_ptr())                              # warm-up (allocates the degree counters)
        ms = [timed(stream, lambda: kc.graph_adjacency(adj.data_ptr()))[0] for _ in range(args.reps)]
        ms_deg = [timed(stream, kc.graph_adjacency)[0] for _ in range(args.reps)]      # the degree table alone: no byte leaves
        set_bits = sum(int(deg[i, o]) * (i + o) for i in range(5) for o in range(5))
        popcount = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int64, device=dev)
        assert int(deg.sum()) == rows and set_bits == int(popcount[adj.long()].sum()), "the degree table and the bytes disagree"
        probes = 8 * rows
        frac = set_bits / probes
        res.update(rows=rows, index_ms=round(ms_index, 3), probes=probes, set_bits=set_bits, hit_fraction=round(frac, 4),
                   degrees=[[int(v) for v in r] for r in deg], **summary("graph", ms, probes), **summary("graph_degrees_only", ms_deg, probes))
        res["stage_graph_ms"] = round(dict(kc.stage_times()).get("graph", 0.0), 3)

        # (B) query_kmers on the same index, the same number of probes, the same hit fraction
        w = kc.words
        g = torch.Generator(device=dev)
        g.manual_seed(1234 + k)
        if w == 1:
            hip = ctypes.CDLL("libamdhip64.so")
            rk = torch.empty((rows, 1), dtype=torch.int64, device=dev)
            assert hip.hipMemcpy(ctypes.c_void_p(rk.data_ptr()), ctypes.c_void_p(kp), ctypes.c_size_t(rows * 8), 3) == 0
        else:
            rk = torch.from_numpy(kc.rows()[0].view("int64")).to(dev)          # the higher words: through the host, as any caller
        keys = rk[torch.randint(0, rows, (probes,), generator=g, device=dev)]
        absent = torch.rand(probes, generator=g, device=dev) >= frac
        top_bits = 2 * k - 64 * (w - 1)
        rnd = (torch.randint(0, 1 << 32, (probes, w), generator=g, device=dev, dtype=torch.int64) << 32) | torch.randint(0, 1 << 32, (probes, w), generator=g, device=dev, dtype=torch.int64)
        if top_bits < 64:
            rnd[:, w - 1] &= (1 << top_bits) - 1
        keys = torch.where(absent[:, None], rnd, keys)
        del rnd
        n_hit = probes - int(absent.sum())
        del absent
        out32 = torch.zeros(probes, dtype=torch.int32, device=dev)
        stream.synchronize()
        kc.query_kmers(keys.data_ptr(), probes, out32.data_ptr())            # warm-up
        found = int((out32 != 0).sum())
        assert abs(found - n_hit) <= 8, (found, n_hit)                        # (a random value is a row with probability ~ rows / 4^k)
        bms = [timed(stream, lambda: kc.query_kmers(keys.data_ptr(), probes, out32.data_ptr()))[0] for _ in range(args.reps)]
        del keys
        res.update(lookup_hits=found, **summary("lookup", bms, probes))
        res["graph_over_lookup_rate"] = round(statistics.median(bms) / statistics.median(ms), 3)

        # (A) the composition a caller had before
        if k <= 31 and not args.no_caller_path:
            x = rk[:, 0].contiguous()
            out_r = out32[:rows]
            ref = torch.zeros(rows, dtype=torch.uint8, device=dev)
            caller_path(kc, x, k, out_r, ref)                                  # warm-up
            same = bool((ref == adj).all())
            assert same, "the caller's composition and graph_adjacency disagree"
            ams = [timed(stream, lambda: caller_path(kc, x, k, out_r, ref))[0] for _ in range(args.reps)]
            res.update(caller_agrees=same, **summary("caller", ams, probes))
            res["caller_over_graph_time"] = round(statistics.median(ams) / statistics.median(ms), 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c2_10Mx150")
    ap.add_argument("--k", default="31,63,96", help="comma-separated k")
    ap.add_argument("--abundance-min", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-caller-path", action="store_true", help="skip baseline (A)")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be >= 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_graph.py needs a HIP device: there is no CPU path to time")
    from dsk_amd import synth
    dev = torch.device("cuda", 0)
    reads, gl, nr, rl = synth.make_workload(args.workload, dev)
    torch.cuda.synchronize()
    result = {"bench": "graph_adjacency", "workload": args.workload, "device": torch.cuda.get_device_name(0), "reads": nr, "read_len": rl,
              "abundance_min": args.abundance_min, "results": [bench_k(args, dev, reads, int(k)) for k in args.k.split(",") if k]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
